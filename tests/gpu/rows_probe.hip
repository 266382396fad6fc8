/*
 * rows_probe.hip -- the row pipelines of solve_body.h on LDS images of the caller's (TEST SUPPORT ONLY).
 *
 * fwd_rows / fwd_rows_half / fwd_rows_third / fwd_rows_two_thirds, rev_rows and fwd_rows_wide exist on the device only (the
 * CPU tier has a row loop of its own, tests/emu/strip_emu.h emu_forward).  This library runs them, as compiled from the
 * product's header, on op streams and images that tests/rows_support.py builds, and hands the whole LDS back: the test
 * compares it byte for byte with a plain replay of the stream (tests/test_gpu_rows.py).  It is built on its own
 * (nanorq_amd.build.build_rows_probe) and is no part of libnanorq_hip.so.
 *
 * One workgroup of 256 threads is one case: copy the case's image into the dynamic LDS, barrier, the wave(s) of the form run
 * the pipeline the way the kernels call it, barrier, copy the whole dynamic LDS back.  There is no static LDS here: the
 * pipelines form LDS addresses from image indices alone, so the image must start at LDS address 0, as in the product.
 *
 * rows_probe_run checks every op word against the LDS size before it launches: a stream that names an index outside the image
 * is refused (-2), never run.
 */
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "solve_body.h"
#include "solve_roles.h"

#define PROBE_NT 256u
#define PROBE_LDS_MAX 163840u

struct DevCase {
  uint64_t ops;   /* u32[NRQ_STREAM_ROWS(nrows + NRQ_PAD_ROWS) * NRQ_ROW], quad-interleaved (plan.h) */
  uint64_t in;    /* u8[lds_bytes] */
  uint64_t out;   /* u8[lds_bytes] */
  uint32_t nrows;
  uint32_t pad;
};

/* ---- the forms, called as their call sites call them ---- */
/* nrq_solve_kernel, one forward wave: `if (tid < NRQ_ROW) fwd_rows<WB, RU>(ops, nrows, tid)`, U = the instance's ring (solve_roles.h
 * RU).  Also PL_WFAST_RUN of the planner kernels (fwd_rows<16 / 8 / 4>) and nrq_wpass_kernel (fwd_rows<2>), both U = NRQ_RING. */
template <int WB, uint32_t U> struct FormFwd {
  static __device__ __forceinline__ void run(const NRQ_GAS uint32_t *ops, uint32_t nrows, uint32_t tid) {
    if (tid < NRQ_ROW) fwd_rows<WB, U>(ops, nrows, tid);
  }
};
/* nrq_solve_kernel, 768 threads, 16- and 8-byte strips: waves 0 and 1, half the strip each */
template <int WB, uint32_t U> struct FormHalf {
  static __device__ __forceinline__ void run(const NRQ_GAS uint32_t *ops, uint32_t nrows, uint32_t tid) {
    const uint32_t wv = tid >> 6;
    if (wv == 0u) fwd_rows_half<WB, 0, U>(ops, nrows, tid);
    else if (wv == 1u) fwd_rows_half<WB, WB / 2, U>(ops, nrows, tid & 63u);
  }
};
/* nrq_solve_kernel, 768 threads, 12-byte strips (NRQ_W12_FW = 3): waves 0, 1 and 2, a dword each */
template <uint32_t U> struct FormThird {
  static __device__ __forceinline__ void run(const NRQ_GAS uint32_t *ops, uint32_t nrows, uint32_t tid) {
    const uint32_t wv = tid >> 6;
    if (wv == 0u) fwd_rows_third<0, U>(ops, nrows, tid);
    else if (wv == 1u) fwd_rows_third<4, U>(ops, nrows, tid & 63u);
    else if (wv == 2u) fwd_rows_third<8, U>(ops, nrows, tid & 63u);
  }
};
/* nrq_solve_kernel, 768 threads, 12-byte strips in a build with NRQ_W12_FW = 2: not what the library ships, kept because the
 * source keeps it */
template <uint32_t U> struct FormTwoThirds {
  static __device__ __forceinline__ void run(const NRQ_GAS uint32_t *ops, uint32_t nrows, uint32_t tid) {
    const uint32_t wv = tid >> 6;
    if (wv == 0u) fwd_rows_two_thirds<U>(ops, nrows, tid);
    else if (wv == 1u) fwd_rows_third<8, U>(ops, nrows, tid & 63u);
  }
};
/* PL_MHREV_RUN of the planner kernels: `if (tid < NRQ_ROW) rev_rows<16 / 8 / 4>(ops, rows, tid)` */
template <int WB> struct FormRev {
  static __device__ __forceinline__ void run(const NRQ_GAS uint32_t *ops, uint32_t nrows, uint32_t tid) {
    if (tid < NRQ_ROW) rev_rows<WB>(ops, nrows, tid);
  }
};
/* nrq_solve_kernel on wide strips: `if (tid < NRQ_ROW) fwd_rows_wide<G>(ops, nrows, tid)`, lane = op * G + sub */
template <int G> struct FormWide {
  static __device__ __forceinline__ void run(const NRQ_GAS uint32_t *ops, uint32_t nrows, uint32_t tid) {
    if (tid < NRQ_ROW) fwd_rows_wide<G>(ops, nrows, tid);
  }
};

template <class F> __global__ __launch_bounds__(PROBE_NT) void rows_probe_kernel(const DevCase *__restrict__ cases, uint32_t lds_bytes) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const uint32_t tid = threadIdx.x;
  const DevCase c = cases[blockIdx.x];
  const NRQ_GAS uint4 *in = gptr<uint4>(c.in);
  NRQ_GAS uint4 *out = gptr_w<uint4>(c.out);
  uint4 *lds = reinterpret_cast<uint4 *>(smem);
  for (uint32_t i = tid; i < lds_bytes / 16u; i += PROBE_NT) lds[i] = in[i];
  __syncthreads();
  F::run(gptr<uint32_t>(c.ops), c.nrows, tid);
  __syncthreads();
  for (uint32_t i = tid; i < lds_bytes / 16u; i += PROBE_NT) out[i] = lds[i];
}

/* ---- the address helpers on their own: every 16-bit field value, in both halves of the op word ---- */
#define ADDR_NWB 5u /* WB = 16, 12, 8, 4, 2 */
#define ADDR_FORMS 3u /* op words x | x << 16, x, x << 16 */
/* out[((form * 65536 + x) * ADDR_NWB + w) * 2 + {0: hi, 1: lo}] */
__global__ __launch_bounds__(PROBE_NT) void rows_addr_kernel(uint32_t *__restrict__ out) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t i = blockIdx.x * PROBE_NT + threadIdx.x;
  if (i >= ADDR_FORMS * 65536u) return;
  const uint32_t x = i & 0xFFFFu, form = i >> 16, op = form == 0u ? (x | x << 16) : form == 1u ? x : x << 16;
  uint32_t *o = out + (size_t)i * ADDR_NWB * 2u;
  o[0] = row_addr_hi<16>(op); o[1] = row_addr_lo<16>(op);
  o[2] = row_addr_hi<12>(op); o[3] = row_addr_lo<12>(op);
  o[4] = row_addr_hi<8>(op); o[5] = row_addr_lo<8>(op);
  o[6] = row_addr_hi<4>(op); o[7] = row_addr_lo<4>(op);
  o[8] = row_addr_hi<2>(op); o[9] = row_addr_lo<2>(op);
#endif
}
/* out[i * 4 + byte] = t4_addr(base[i], x[i], byte) */
__global__ __launch_bounds__(PROBE_NT) void rows_t4_kernel(const uint32_t *__restrict__ base, const uint32_t *__restrict__ x, uint32_t n,
                                                            uint32_t *__restrict__ out) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t i = blockIdx.x * PROBE_NT + threadIdx.x;
  if (i >= n) return;
  out[i * 4u] = t4_addr(base[i], x[i], 0);
  out[i * 4u + 1u] = t4_addr(base[i], x[i], 1);
  out[i * 4u + 2u] = t4_addr(base[i], x[i], 2);
  out[i * 4u + 3u] = t4_addr(base[i], x[i], 3);
#endif
}

/* ---- the instance table: what the kernels instantiate (nrq_device.hip) ---- */
typedef void (*probe_fn)(const DevCase *, uint32_t);
struct Instance {
  const char *form; /* the name, with %u for `ring` where the form has one */
  uint32_t ring;
  probe_fn fn;
  uint32_t slot_bytes; /* LDS bytes per image index */
};
/* the op-word ring of the solve workgroup of NT threads built for WV waves per SIMD (solve_roles.h) */
#define RING(WB, NT, WV) solve_roles(WB, NT, WV, 1, false).RU
#define FWD(WB, U) {"fwd_rows<" #WB ",%u>", U, rows_probe_kernel<FormFwd<WB, U>>, WB}
/* the 64-thread solve; the 256-thread solve, five / four workgroups per CU (NRQ_RING: also PL_WFAST_RUN and nrq_wpass_kernel) */
#define FWD_SMALL(WB) FWD(WB, RING(WB, 64, 1)), FWD(WB, RING(WB, 256, 5)), FWD(WB, RING(WB, 256, 4))
static const Instance g_inst[] = {
    FWD_SMALL(16), FWD_SMALL(8), FWD_SMALL(4), FWD_SMALL(2),
    /* the 768-thread solve on strips too narrow for two forward waves */
    FWD(4, RING(4, 768, 1)), FWD(2, RING(2, 768, 1)),
    /* the 768-thread solve: two waves on halves, three on the dwords of the 12-byte strip */
    {"fwd_rows_half<16,%u>", RING(16, 768, 1), rows_probe_kernel<FormHalf<16, RING(16, 768, 1)>>, 16},
    {"fwd_rows_half<8,%u>", RING(8, 768, 1), rows_probe_kernel<FormHalf<8, RING(8, 768, 1)>>, 8},
    {"fwd_rows_third<%u>", RING(12, 768, 1), rows_probe_kernel<FormThird<RING(12, 768, 1)>>, 12},
    /* a build with NRQ_W12_FW = 2 only */
    {"fwd_rows_two_thirds<%u>", RING(12, 768, 1), rows_probe_kernel<FormTwoThirds<RING(12, 768, 1)>>, 12},
    /* PL_MHREV_RUN */
    {"rev_rows<16>", 0, rows_probe_kernel<FormRev<16>>, 16},
    {"rev_rows<8>", 0, rows_probe_kernel<FormRev<8>>, 8},
    {"rev_rows<4>", 0, rows_probe_kernel<FormRev<4>>, 4},
    /* wide strips */
    {"fwd_rows_wide<2>", 0, rows_probe_kernel<FormWide<2>>, 32},
    {"fwd_rows_wide<4>", 0, rows_probe_kernel<FormWide<4>>, 64},
    {"fwd_rows_wide<8>", 0, rows_probe_kernel<FormWide<8>>, 128},
};
static const uint32_t g_ninst = sizeof(g_inst) / sizeof(g_inst[0]);

/* what the caller hands over, one per case (host pointers) */
struct rows_probe_case {
  const uint32_t *ops;
  uint64_t ops_words;
  const uint8_t *image_in; /* lds_bytes */
  uint8_t *image_out;      /* lds_bytes */
  uint32_t nrows;
  uint32_t pad;
};

namespace {
struct DevBuf { /* freed on every path */
  void *p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t n) { return hipMalloc(&p, n ? n : 16); }
};
}

extern "C" {

uint32_t rows_probe_ninstances(void) { return g_ninst; }
const char *rows_probe_name(uint32_t i) { /* "fwd_rows<16,24>": the form with its ring filled in */
  static char names[sizeof(g_inst) / sizeof(g_inst[0])][40];
  if (i < g_ninst) snprintf(names[i], sizeof(names[i]), g_inst[i].form, g_inst[i].ring);
  return i < g_ninst ? names[i] : nullptr;
}
uint32_t rows_probe_slot_bytes(uint32_t i) { return i < g_ninst ? g_inst[i].slot_bytes : 0u; }

/* All cases of one instance in one launch.  Returns the HIP status (0 = hipSuccess), or -1 for arguments that make no sense,
 * -2 for a stream that is too short for the pipelines' reads ahead or names an index outside the LDS: nothing is launched then. */
int rows_probe_run(uint32_t inst, const rows_probe_case *cases, uint32_t ncases, uint32_t lds_bytes) {
  if (inst >= g_ninst || !cases || !ncases || !lds_bytes || lds_bytes % 16u || lds_bytes > PROBE_LDS_MAX) return -1;
  const uint32_t nidx = lds_bytes / g_inst[inst].slot_bytes;
  size_t total_words = 0;
  for (uint32_t k = 0; k < ncases; k++) {
    const rows_probe_case &c = cases[k];
    if (!c.ops || !c.image_in || !c.image_out) return -1;
    const uint64_t need = (uint64_t)NRQ_STREAM_ROWS((uint64_t)c.nrows + NRQ_PAD_ROWS) * NRQ_ROW;
    if (c.ops_words < need || c.ops_words % 4u) return -2;
    for (uint64_t w = 0; w < c.ops_words; w++) {
      const uint32_t op = c.ops[w];
      if ((op & 0xFFFFu) >= nidx || (op >> 16) >= nidx) return -2;
      /* behind the stream: padding, whatever the caller meant (the pipelines run into these rows) */
      const uint64_t row = (w / (4u * NRQ_ROW)) * 4u + (w & 3u);
      if (row >= c.nrows && op != NRQ_NOP_AT(NRQ_OP_LANE_OF_INDEX(w))) return -2;
    }
    total_words += (size_t)c.ops_words;
  }
  DevBuf d_ops, d_in, d_out, d_cases;
  hipError_t e;
  if ((e = d_ops.alloc(total_words * 4u)) != hipSuccess) return (int)e;
  if ((e = d_in.alloc((size_t)ncases * lds_bytes)) != hipSuccess) return (int)e;
  if ((e = d_out.alloc((size_t)ncases * lds_bytes)) != hipSuccess) return (int)e;
  if ((e = d_cases.alloc((size_t)ncases * sizeof(DevCase))) != hipSuccess) return (int)e;
  std::vector<DevCase> dc(ncases);
  size_t at = 0;
  for (uint32_t k = 0; k < ncases; k++) {
    const rows_probe_case &c = cases[k];
    uint8_t *o = static_cast<uint8_t *>(d_ops.p) + at * 4u;
    uint8_t *i = static_cast<uint8_t *>(d_in.p) + (size_t)k * lds_bytes;
    if ((e = hipMemcpy(o, c.ops, (size_t)c.ops_words * 4u, hipMemcpyHostToDevice)) != hipSuccess) return (int)e;
    if ((e = hipMemcpy(i, c.image_in, lds_bytes, hipMemcpyHostToDevice)) != hipSuccess) return (int)e;
    dc[k].ops = (uint64_t)(uintptr_t)o;
    dc[k].in = (uint64_t)(uintptr_t)i;
    dc[k].out = (uint64_t)(uintptr_t)(static_cast<uint8_t *>(d_out.p) + (size_t)k * lds_bytes);
    dc[k].nrows = c.nrows;
    dc[k].pad = 0;
    at += (size_t)c.ops_words; /* (a multiple of 4 words: every stream starts on 16 bytes) */
  }
  if ((e = hipMemset(d_out.p, 0xEE, (size_t)ncases * lds_bytes)) != hipSuccess) return (int)e;
  if ((e = hipMemcpy(d_cases.p, dc.data(), (size_t)ncases * sizeof(DevCase), hipMemcpyHostToDevice)) != hipSuccess) return (int)e;
  const void *fn = reinterpret_cast<const void *>(g_inst[inst].fn);
  if ((e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PROBE_LDS_MAX)) != hipSuccess) return (int)e;
  const DevCase *arg0 = static_cast<const DevCase *>(d_cases.p);
  uint32_t arg1 = lds_bytes;
  void *args[] = {&arg0, &arg1};
  if ((e = hipLaunchKernel(fn, dim3(ncases), dim3(PROBE_NT), args, lds_bytes, nullptr)) != hipSuccess) return (int)e;
  if ((e = hipDeviceSynchronize()) != hipSuccess) return (int)e;
  for (uint32_t k = 0; k < ncases; k++)
    if ((e = hipMemcpy(cases[k].image_out, static_cast<uint8_t *>(d_out.p) + (size_t)k * lds_bytes, lds_bytes, hipMemcpyDeviceToHost)) != hipSuccess)
      return (int)e;
  return 0;
}

/* hi_lo: u32[ADDR_FORMS * 65536 * ADDR_NWB * 2] (rows_addr_kernel's layout); t4: u32[n * 4] for the n words of base[] and x[] */
int rows_probe_addr(uint32_t *hi_lo, const uint32_t *base, const uint32_t *x, uint32_t n, uint32_t *t4) {
  if (!hi_lo || !base || !x || !t4 || !n || n > (1u << 20)) return -1;
  const size_t nhl = (size_t)ADDR_FORMS * 65536u * ADDR_NWB * 2u;
  DevBuf d_hl, d_base, d_x, d_t4;
  hipError_t e;
  if ((e = d_hl.alloc(nhl * 4u)) != hipSuccess) return (int)e;
  if ((e = d_base.alloc((size_t)n * 4u)) != hipSuccess) return (int)e;
  if ((e = d_x.alloc((size_t)n * 4u)) != hipSuccess) return (int)e;
  if ((e = d_t4.alloc((size_t)n * 16u)) != hipSuccess) return (int)e;
  if ((e = hipMemset(d_hl.p, 0xEE, nhl * 4u)) != hipSuccess) return (int)e;
  if ((e = hipMemset(d_t4.p, 0xEE, (size_t)n * 16u)) != hipSuccess) return (int)e;
  if ((e = hipMemcpy(d_base.p, base, (size_t)n * 4u, hipMemcpyHostToDevice)) != hipSuccess) return (int)e;
  if ((e = hipMemcpy(d_x.p, x, (size_t)n * 4u, hipMemcpyHostToDevice)) != hipSuccess) return (int)e;
  hipLaunchKernelGGL(rows_addr_kernel, dim3(ADDR_FORMS * 65536u / PROBE_NT), dim3(PROBE_NT), 0, nullptr, static_cast<uint32_t *>(d_hl.p));
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  hipLaunchKernelGGL(rows_t4_kernel, dim3((n + PROBE_NT - 1u) / PROBE_NT), dim3(PROBE_NT), 0, nullptr, static_cast<const uint32_t *>(d_base.p),
                     static_cast<const uint32_t *>(d_x.p), n, static_cast<uint32_t *>(d_t4.p));
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  if ((e = hipDeviceSynchronize()) != hipSuccess) return (int)e;
  if ((e = hipMemcpy(hi_lo, d_hl.p, nhl * 4u, hipMemcpyDeviceToHost)) != hipSuccess) return (int)e;
  if ((e = hipMemcpy(t4, d_t4.p, (size_t)n * 16u, hipMemcpyDeviceToHost)) != hipSuccess) return (int)e;
  return 0;
}

} /* extern "C" */
