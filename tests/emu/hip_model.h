/* A model of the HIP runtime for the CPU tier (tests/test_host_model.py): the host layer of the library -- nrq_device.hip's host
 * code, planner_host.cpp, nanorq_api.c, io.c, compiled from the same sources -- runs against it instead of against the runtime.
 * The model tracks the ORDER the runtime would give the operations (streams, events, synchronisations) and the LIFETIME of
 * every allocation, and reports what the real runtime would not have ordered or what falls outside a live allocation.  It is
 * test support: nothing of it is linked into libnanorq_hip.so.
 *
 * This header has two halves.
 *   1. The C interface of the model (hm_*), for the tests (ctypes) and for tests/emu/model_exercise.cpp.
 *   2. The launch hook.  nrq_device.hip is compiled host-only with this header force-included (-include): it pulls in
 *      <hip/hip_runtime.h> first and then re-defines hipLaunchKernelGGL as a typed call into the model.  No launch site is
 *      edited.  Kernels do NOT run; a launch is an operation on its stream whose footprint comes from its typed arguments.
 *
 * MODELLING ASSUMPTIONS ("Stream order and lifetimes of the host layer")
 *   - Streams are hipStreamNonBlocking: the null stream is an ordinary stream to them.  Happens-before comes from stream
 *     order, hipEventRecord -> hipStreamWaitEvent / hipEventSynchronize, hipStreamSynchronize, hipDeviceSynchronize and the
 *     blocking hipMemcpy; an operation is enqueued after everything the host has synchronised with.  Waiting for an event
 *     that was never recorded orders nothing, as in HIP.
 *   - hipFree is a device-wide synchronisation (the library's comments rely on that).
 *   - hipHostFree and hipHostUnregister do NOT synchronise.  This is a deliberately conservative assumption, not a measured
 *     fact about the runtime: a host allocation released under a pending operation is reported (H3) whether or not a given
 *     runtime version would have waited.
 *   - Copies between device memory and PAGEABLE host memory (host memory the model has no allocation for) are staged by the
 *     runtime: a device -> pageable copy returns when the bytes have arrived (the host has then synchronised with the stream),
 *     a pageable -> device copy has read its source on return.  Only page-locked host memory (hipHostMalloc, hipHostRegister)
 *     is touched asynchronously.
 *   - Device -> page-locked copies are the only deferred byte movement: the destination is filled with HM_POISON at enqueue and
 *     the bytes (as they were at enqueue) arrive when the host synchronises behind the copy.  Every other copy and memset moves
 *     its bytes at enqueue, so that control arrays are in place when the next launch's footprint is taken.
 *   - Kernels do not run.  Three kernels whose whole effect is a copy have that effect and an exact footprint (hm_set_effect):
 *     nrq_ctl_copy_kernel (control arrays: job records, address lists, whose pointers the footprint of a later launch follows),
 *     nrq_scatter_kernel and nrq_move_rows_kernel (rows by address list).  The decode planner and the kernels that run a batch of
 *     job records (solve, back-substitution, collect) have exact footprints too (tests/emu/model_effects.cpp): the records and what
 *     each record's addresses name, not every word of those allocations one level further.  Every other kernel is a no-op whose
 *     footprint is what its arguments can reach.
 *   - A plain hipMemcpy is an operation on stream 0 -- whatever stream the context of the caller is on -- that the host then
 *     waits for: it is ordered behind what the host has synchronised with and behind stream 0, and behind nothing else.
 *   - No guard pages and no signal handler: a range that is not inside a live allocation is reported and NOT touched.  "Device"
 *     and page-locked memory are carved from two reserved address ranges and addresses are never handed out twice, so a 64-bit
 *     word can be recognised as a device pointer and a stale pointer never names a newer allocation.
 *
 * HAZARDS
 *   H1  two operations touch one allocation (overlapping ranges), at least one writes, neither happens before the other
 *   H2  a range outside any live allocation (out of bounds, freed, unknown) in a copy, a memset or a launch argument
 *   H3  a host allocation released or unregistered while a pending operation touches it
 *   H4  the source of an asynchronous page-locked -> device copy changed before the host synchronised behind the copy
 */
#ifndef NRQ_HIP_MODEL_H
#define NRQ_HIP_MODEL_H

#include <stddef.h>
#include <stdint.h>

#define HM_POISON 0xDB

#ifdef __cplusplus
extern "C" {
#endif

/* one argument of a launch, as the hook hands it over */
typedef struct hm_arg {
  const void *p; /* HM_ARG_PTR / HM_ARG_CONST_PTR: the pointer's value; HM_ARG_BYTES / HM_ARG_SCALAR: the address of the argument */
  size_t n;      /* HM_ARG_BYTES (a struct or a 64-bit word: scanned) / HM_ARG_SCALAR (any other value: for the effects): its size */
  int kind;
} hm_arg;
enum { HM_ARG_PTR = 0, HM_ARG_CONST_PTR = 1, HM_ARG_BYTES = 2, HM_ARG_SCALAR = 3 };

/* a launch: `fn` is the kernel's host-side handle (what __hipRegisterFunction was given), `stream` a hipStream_t */
void hm_model_launch(const void *fn, const char *file, int line, void *stream, const unsigned grid[3], const hm_arg *args, int nargs);
/* the same for a hand-built scenario: `name` instead of a registered kernel */
void hm_launch_named(const char *name, void *stream, const hm_arg *args, int nargs);

/* An effect for the kernels registered under a (mangled) device name that CONTAINS `name_part`, called at enqueue.
 * exact = 0: after the footprint was taken from the arguments.  exact = 1: INSTEAD of it -- the effect says what the launch
 * touches, range by range (hm_effect_touch: 1 = inside a live allocation and recorded, 0 = reported as H2), and may move bytes
 * between ranges that were accepted.  The model brings exact effects for the three kernels of the library that only move bytes:
 * nrq_ctl_copy_kernel, nrq_scatter_kernel, nrq_move_rows_kernel (their lists hold addresses they never dereference, or
 * dereference row by row); tests/emu/model_effects.cpp adds the decode planner's.  The device-resident receivers, senders and
 * sets need more of them (their host flow reads counts their kernels write). */
typedef void (*hm_effect_fn)(const hm_arg *args, int nargs);
void hm_set_effect(const char *name_part, hm_effect_fn fn, int exact);
int hm_effect_touch(const void *p, size_t n, int write);
int hm_effect_touch_tail(const void *p, int write); /* from p to the end of its allocation (a buffer whose size the launch does not say) */
uint64_t hm_effect_base(const void *p);             /* the base of the live allocation that holds p (0: none), to touch an allocation once */
void hm_effect_wrote(const void *p, size_t n);       /* the effect has put bytes there itself: they may hold addresses a later launch follows */
void hm_effect_grid(unsigned out[3]);               /* the grid of the launch whose effect is running */

/* reports */
uint64_t hm_hazard_count(void);
/* the hazards so far as a JSON list into buf (at most cap bytes, always terminated); returns the length needed */
size_t hm_hazards_json(char *buf, size_t cap);
void hm_hazards_clear(void);
/* counters: [0] operations, [1] launches, [2] copies and memsets, [3] waits for a never-recorded event, [4] live allocations,
 * [5] words of the device ranges that scans found pointing at no live allocation (stale: counted, no hazard),
 * [6] deferred copies still pending, [7] launches of kernels no registration names */
void hm_counters(uint64_t out[8]);
/* the live allocation that holds p: 1 and its base / size / kind (0 device, 1 hipHostMalloc, 2 hipHostRegister), or 0 */
int hm_block_of(const void *p, uint64_t *base, uint64_t *size, int *kind);
/* operations touching the allocation of p (any byte of it) that the host has not synchronised behind; -1: no live allocation */
int hm_pending_on(const void *p);
/* the same over every live allocation */
int hm_pending_total(void);

#ifdef __cplusplus
}
#endif

/* ------------------------------------------------------------------------------------------------------------------------
 * The launch hook (only where the translation unit is HIP: nrq_device.hip, host-only)
 * ---------------------------------------------------------------------------------------------------------------------- */
#if defined(__cplusplus) && defined(__HIPCC__) && defined(NRQ_HIP_MODEL_HOOK)
#include <hip/hip_runtime.h>
#include <tuple>
#include <type_traits>

namespace hm_hook {
template <typename P>
inline void put(hm_arg *a, int &n, const P &v) {
  if constexpr (std::is_pointer<P>::value) {
    a[n].p = (const void *)v;
    a[n].n = 0;
    a[n].kind = std::is_const<typename std::remove_pointer<P>::type>::value ? HM_ARG_CONST_PTR : HM_ARG_PTR;
    n++;
  } else if constexpr (std::is_class<P>::value || (std::is_integral<P>::value && sizeof(P) == 8)) {
    a[n].p = (const void *)&v; /* a struct (ing_rx, tx_src, rq_params, ...) or a 64-bit word: scanned for device addresses */
    a[n].n = sizeof(P);
    a[n].kind = HM_ARG_BYTES;
    n++;
  } else {
    a[n].p = (const void *)&v;
    a[n].n = sizeof(P);
    a[n].kind = HM_ARG_SCALAR;
    n++;
  }
}
/* the kernel's parameter types KArgs give each argument its type (the call's own expressions may be of other, convertible types) */
template <typename... KArgs, typename... Args>
inline void launch(const char *file, int line, void (*kernel)(KArgs...), dim3 grid, dim3, size_t, hipStream_t st, Args &&...args) {
  static_assert(sizeof...(KArgs) == sizeof...(Args), "a launch passes every parameter of its kernel");
  hm_arg a[sizeof...(KArgs) + 1];
  int n = 0;
  auto one = [&](const auto &typed) { put(a, n, typed); };
  /* (the typed copies stay in this tuple until the model has read them) */
  std::tuple<typename std::decay<KArgs>::type...> typed{static_cast<typename std::decay<KArgs>::type>(args)...};
  std::apply([&](const auto &...t) { (one(t), ...); }, typed);
  const unsigned g[3] = {grid.x, grid.y, grid.z};
  hm_model_launch((const void *)kernel, file, line, (void *)st, g, a, n);
}
} // namespace hm_hook

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, shmem, stream, ...) \
  hm_hook::launch(__FILE__, __LINE__, kernel, dim3(grid), dim3(block), (size_t)(shmem), (hipStream_t)(stream), ##__VA_ARGS__)
#endif

#endif
