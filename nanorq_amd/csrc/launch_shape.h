/*
 * launch_shape.h -- what a launch will look like, decided before anything is launched.
 *
 *   Tuning / NRQ_KNOBS      every tuning and test knob of the host, one row each
 *   (solve_roles.h)         what an instance of nrq_solve_kernel decides about itself: its compile-time knobs, wave roles, phase forms
 *   NRQ_SOLVE_INSTANCES     every compiled nrq_solve_kernel instance, once (NRQ_PLAN_INSTANCES: nrq_plan_kernel)
 *   solve_lists()           which blocks of a batch are solved at which strip width (one launch or two)
 *   solve_shape()           one solve launch: instance, workgroups per CU, grid, work slots, staging strides, the split
 *   plan_shape()            one planner run: instance, LDS sizing, the parts and their helper kernels
 *
 * Values in, a record out: no context, no runtime call, no allocation.  nrq_device.hip does what the records say; this
 * header has no HIP include, so the host compiler builds it too (tests/emu/shape_emu.cpp, tests/test_launch_shape_emu.py).
 */
#ifndef NRQ_LAUNCH_SHAPE_H
#define NRQ_LAUNCH_SHAPE_H

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "plan.h"
#include "rq_math.h"
#include "solve_body.h"
#include "solve_roles.h"
#include "planner_body.h"

#define NRQ_LDS_MAX 163840u /* 160 KiB per workgroup on gfx950 */
/* ... handed out in pieces of 320 dwords (LLVM getLdsDwGranularity for the 160 KiB parts): what a workgroup asks for is rounded
 * up to that, and how many workgroups share a CU follows from the rounded size.  (The HIP occupancy query divides the bytes:
 * it said nine 18 016-byte workgroups fit, eight were resident, and the ninth of every CU ran as a second round -- K=500.) */
#define NRQ_LDS_GRANULE 1280u
static inline uint32_t lds_alloc(uint32_t bytes) { return (bytes + NRQ_LDS_GRANULE - 1u) / NRQ_LDS_GRANULE * NRQ_LDS_GRANULE; }
#ifndef NRQ_WG
#define NRQ_WG 768 /* threads of the solve workgroup: 3 waves per SIMD.  One workgroup owns the CU (LDS), and its phases are
                    * bound by instruction issue and LDS latency: measured 256 -> 512 -> 768 -> 1024 threads = 673 / 796 / 835 /
                    * 807 Gbit/s on the headline workload */
#endif
#ifndef NRQ_TINY_WV
#define NRQ_TINY_WV 3   /* the single-wave variant: waves per SIMD it is built for (170 registers), */
#endif
#ifndef NRQ_TINY_OCC
#define NRQ_TINY_OCC 12u /* and workgroups per compute unit it runs with.  Round 4, K=100 T=1024 x 8192 blocks: 5 / 18 (96 registers,
                          * 151 of them spilled: every phase reloads its pointers from scratch) 370 Gbit/s, 4 / 16 ~385, 3 / 12 419,
                          * 2 / 8 358; K=256 527 / 547 / 569 / 533 */
#endif
#ifndef NRQ_SMALL_WV
#define NRQ_SMALL_WV 4   /* the 256-thread variant: workgroups per compute unit = waves per SIMD it is built for */
#endif

/* with many blocks in the launch all line groups of a block go to workgroups of one XCD (nrq_map_group in solve_body.h) */
static inline bool nrq_map_by_block(uint32_t nblk) { return nblk >= 64u || (nblk >= 8u && (nblk & 7u) == 0u); }

/* ============================================================================================
 * Knobs.  One row each: type, field, default, environment name, option name (nrq_ctx_set_option; 0 = none), kind.
 * The environment is read ONCE, when the context is created (the launch path does not call getenv).
 *   KNOB_FLAG    set by the environment name being present, or by an option value != 0
 *   KNOB_NFLAG   on by default: CLEARED by the environment name being present; the option sets it directly (value != 0)
 *   KNOB_NUM     a number, cast to the field's type (environment: unset or empty = the default)
 *   KNOB_BOOLNUM a bool given as a number (environment: unset or empty = the default)
 *   KNOB_WIDEG   2, 4 or 8; anything else 0
 *   KNOB_LDSMAX  1 .. NRQ_LDS_MAX; anything else NRQ_LDS_MAX
 * ========================================================================================== */
enum KnobKind { KNOB_FLAG, KNOB_NFLAG, KNOB_NUM, KNOB_BOOLNUM, KNOB_WIDEG, KNOB_LDSMAX };
#define NRQ_KNOBS(K)                                                                                                                                    \
  K(bool, map_spread, false, "NRQ_MAP_SPREAD", "map_spread", KNOB_FLAG) /* deal line groups round-robin instead of block octets per XCD */              \
  K(bool, big_wg, false, "NRQ_BIG_WG", "big_wg", KNOB_FLAG) /* never use the 256-thread solve variants */                                               \
  /* cleared: the 256-thread variant compiled for 5 workgroups per CU (96 registers per thread) is used where five images fit;                          \
   * since the row pipeline forms its addresses ahead of the LDS wait the 4-workgroup one (128 registers) is faster there:                              \
   * K=1000 930 -> 980 Gbit/s */                                                                                                                        \
  K(bool, small_waves4, true, "NRQ_SMALL_WAVES5", "small_waves4", KNOB_NFLAG)                                                                           \
  K(bool, prof, false, "NRQ_PROF", 0, KNOB_FLAG) /* per-phase shader-clock marks, printed to stderr */                                                  \
  K(bool, diag, false, "NRQ_DIAG", 0, KNOB_FLAG) /* why a block was reported not decodable, to stderr */                                                \
  K(bool, plan_lds_max, false, "NRQ_PLAN_LDS_MAX", 0, KNOB_FLAG) /* planner always takes the whole LDS */                                               \
  K(bool, plan_big_wg, false, "NRQ_PLAN_BIG_WG", "plan_big_wg", KNOB_FLAG) /* planner always 1024 threads */                                            \
  K(uint32_t, small_div, 2, "NRQ_SMALL_DIV", 0, KNOB_NUM) /* LDS images per CU from which the 256-thread variant is used (measured: 2 beats 3) */       \
  K(uint64_t, solve_grid, 0, "NRQ_SOLVE_GRID", "solve_grid", KNOB_NUM) /* persistent workgroups of the solve launch (0 = fill the device) */            \
  K(uint32_t, max_wb, 16, "NRQ_MAX_WB", "max_wb", KNOB_NUM) /* widest strip considered */                                                               \
  K(bool, no_wb12, false, "NRQ_NO_WB12", "no_wb12", KNOB_FLAG) /* strip widths 16, 8, 4, 2 only (round 5's set) */                                      \
  /* the solve's throughput forms whatever the launch size (tests): single-wave workgroups also for a few hundred strips,                               \
   * 256-thread ones also for a lone mid-size block */                                                                                                  \
  K(bool, tiny_any, false, "NRQ_TINY_ANY", "tiny_any", KNOB_FLAG)                                                                                       \
  K(bool, plan_pack, false, "NRQ_PLAN_PACK", "plan_pack", KNOB_FLAG) /* small blocks' planner workgroups share a CU whatever the block count */         \
  /* 0: a call of one or two small blocks is planned by the planner kernel like any other */                                                            \
  K(bool, host_plan_auto, true, "NRQ_HOST_PLAN_AUTO", "host_plan_auto", KNOB_BOOLNUM)                                                                   \
  K(int, prof_base, 2, "NRQ_PROF_BASE", 0, KNOB_NUM) /* stamp the free-form marks of the profile are measured from */                                   \
  /* from this many intermediate symbols on, encode plans are built by the device planner, asynchronously (the host planner                             \
   * takes 25 ms at K=27000, 95 ms at K'=56403) */                                                                                                      \
  K(uint32_t, encplan_dev_min_l, 12000, "NRQ_ENCPLAN_DEV_MIN_L", "encplan_dev_min_l", KNOB_NUM)                                                         \
  K(uint32_t, wide_g, 0, "NRQ_WIDE_G", "wide_g", KNOB_WIDEG) /* wide strips of G = 2, 4, 8 lanes per element where two such images fit a CU */          \
  /* big blocks' entry pass by the planner workgroup itself, not by nrq_wentry_kernel */                                                                \
  K(bool, no_wentry, false, "NRQ_NO_WENTRY", "no_wentry", KNOB_FLAG)                                                                                    \
  K(bool, no_tiny, false, "NRQ_NO_TINY", "no_tiny", KNOB_FLAG) /* no single-wave workgroups for tiny strip images */                                    \
  /* LDS images per CU from which the single-wave variant is used (launches with ONE plan: encode).  (Twelve until the                                  \
   * workgroups per CU were counted by allocated LDS, lds_alloc(): between eight and eleven images the ninth.. workgroup of a CU                        \
   * had run as a second round and the variant looked slow; with the count right it wins from seven on -- K=450 +22 %,                                  \
   * K=500 +14 %, K=600 +12 %, K=700 +2 %.) */                                                                                                          \
  K(uint32_t, tiny_div, 7, "NRQ_TINY_DIV", "tiny_div", KNOB_NUM)                                                                                        \
  /* the same for launches with a plan per block (decode): every strip walks a plan of its own through L2 / HBM, and more                               \
   * independent strips in flight hide more of those trips.  (Seven: at six images per CU -- K=1000 once its plans have a few                           \
   * inactive columns fewer -- the single waves lose to the 256-thread workgroups, decode 11.1 against 7.4 ms per 2048 blocks;                          \
   * at seven, K=700, they win 5.2 : 6.2.) */                                                                                                           \
  K(uint32_t, tiny_div_dec, 7, "NRQ_TINY_DIV_DEC", "tiny_div_dec", KNOB_NUM)                                                                            \
  K(bool, no_split, false, "NRQ_NO_SPLIT", "no_split", KNOB_FLAG) /* narrow strips also do their back-substitution in the solve kernel */               \
  K(bool, no_balance, false, "NRQ_NO_BALANCE", "no_balance", KNOB_FLAG) /* keep whole-line work slots even when the rounds come out uneven */           \
  /* (tests) LDS bytes a strip image may take when the batch's block lists are formed (solve_lists) */                                                  \
  K(uint32_t, lds_max, NRQ_LDS_MAX, 0, "lds_max", KNOB_LDSMAX)                                                                                          \
  /* one solve launch per batch at the width EVERY block fits (round 5), no second list */                                                              \
  K(bool, no_lists, false, "NRQ_NO_LISTS", "no_lists", KNOB_FLAG)                                                                                       \
  K(int, reserve_cus, -1, "NRQ_RESERVE_CUS", "reserve_cus", KNOB_NUM) /* compute units a big-block solve launch leaves to the planner (-1 = automatic) */ \
  /* cleared: small blocks' planner workgroups keep the full-size queues */                                                                             \
  K(bool, plan_small_state, true, "NRQ_PLAN_BIG_STATE", "plan_small_state", KNOB_NFLAG)                                                                 \
  K(bool, plan_split_force, false, 0, "plan_split_force", KNOB_FLAG) /* (tests) every block planned in two parts + helper kernels */                    \
  /* big blocks planned by one kernel (no helper kernels for the HDPC fold / W transposition) */                                                        \
  K(bool, no_plan_split, false, "NRQ_NO_PLAN_SPLIT", "no_plan_split", KNOB_FLAG)                                                                        \
  /* planner kernel on the caller's stream (no overlap with the solve before it) */                                                                     \
  K(bool, no_plan_stream, false, "NRQ_NO_PLAN_STREAM", "no_plan_stream", KNOB_FLAG)                                                                     \
  K(bool, tx_dword, false, 0, "tx_dword", KNOB_FLAG) /* (A/B runs) the emit kernels' 4-byte path also where the 16-byte one applies */                  \
  K(bool, plan_no_wg128, false, "NRQ_PLAN_NO_WG128", "plan_no_wg128", KNOB_FLAG) /* the smallest blocks' planner workgroups stay at 256 threads */      \
  /* (tests) blocks whose peeling state fits the LDS are given to the planner instance for the others -- pl_init_a must notice                          \
   * (PL_PEEL_FORM_OK) and the blocks go to the host planner */                                                                                         \
  K(bool, plan_wrong_instance, false, 0, "plan_wrong_instance", KNOB_FLAG)                                                                              \
  /* inactive-column capacity of the device planner (0 = P + 768, at most 1280); tests lower it to send blocks through the                              \
   * capacity fallback (host re-plan) */                                                                                                                \
  K(uint32_t, plan_ucap, 0, 0, "plan_ucap", KNOB_NUM)                                                                                                   \
  /* (tests) strip bytes of the split solve's back-substitution: 0 = by the W words per row (solve_shape), 16 = 16-byte strips                          \
   * whatever they are.  (Nothing forces 32: beyond 20 words its tables do not fit beside a second workgroup.) */                                      \
  K(uint32_t, backsub_sb, 0, 0, "backsub_sb", KNOB_NUM)                                                                                                 \
  /* (tests) every plan the context builds on the HOST (decode, encode, the capacity fallback) starts with this many columns                            \
   * more inactive (planner_host.h nrq_host_plan_build_forced): same results, a chosen number of inactive columns u -- and with                         \
   * it the back-substitution form the solve runs (solve_body.h: by wpr = ceil(u / 32)).  0: the plans are what they are */                             \
  K(uint32_t, plan_force_inact, 0, 0, "plan_force_inact", KNOB_NUM)                                                                                     \
  /* (tests) device-planned decodes get no out view (plan.h off_wout; bit 10 of nrq_planjob::mode): their jobs run on the                               \
   * needed-pivot view, as they do when the image finds no room in the arena (planner_body.h pl_final_b) */                                             \
  K(bool, plan_no_out_view, false, 0, "plan_no_out_view", KNOB_FLAG)

static inline long long knob_norm(KnobKind kind, long long v) {
  switch (kind) {
    case KNOB_WIDEG: return (v == 2 || v == 4 || v == 8) ? v : 0;
    case KNOB_LDSMAX: return (v > 0 && v <= (long long)NRQ_LDS_MAX) ? v : (long long)NRQ_LDS_MAX;
    case KNOB_NUM: return v;
    default: return v != 0;
  }
}
static inline bool knob_named(const char *opt, const char *name) { return opt && !strcmp(opt, name); }
template <class X> static inline void knob_from_env(X &field, const char *env, KnobKind kind) {
  if (!env) return;
  const char *e = getenv(env);
  if (kind == KNOB_FLAG) field = (X)(e != nullptr);
  else if (kind == KNOB_NFLAG) field = (X)(e == nullptr);
  else if (e && *e) field = (X)knob_norm(kind, (long long)(X)atoll(e));
}

struct Tuning {
#define NRQ_KNOB_FIELD(type, field, def, env, opt, kind) type field = def;
  NRQ_KNOBS(NRQ_KNOB_FIELD)
#undef NRQ_KNOB_FIELD
  void read() {
#define NRQ_KNOB_READ(type, field, def, env, opt, kind) knob_from_env(field, env, kind);
    NRQ_KNOBS(NRQ_KNOB_READ)
#undef NRQ_KNOB_READ
  }
  /* an option by name; false: no knob has that option name */
  bool set(const char *name, long long value) {
#define NRQ_KNOB_SET(type, field, def, env, opt, kind) \
  if (knob_named(opt, name)) { field = (type)knob_norm(kind, value); return true; }
    NRQ_KNOBS(NRQ_KNOB_SET)
#undef NRQ_KNOB_SET
    return false;
  }
};

/* ============================================================================================
 * The compiled instances
 * ========================================================================================== */

/* nrq_solve_kernel<WB, NT, WV, G, AL>, every instance the library holds, in the order their attributes are set (on the first
 * launch at a width: that width's rows).  A launch looks its key up here; a key that is not listed is an error.
 * The four shapes of 16 / 8 / 4 / 2-byte strips with both mover forms, the full-size workgroup of the 12-byte strip (compiled for
 * it only), the wide strips.  NOTHING selects the four WB = 2 rows with AL = true -- solve_shape() allows the aligned movers from
 * 4 bytes on -- they are kept because the ledger of variants (tests/variant_ledger.py) counts them. */
#define NRQ_SOLVE_WIDTH(X, WB)                                                                                                        \
  X(WB, NRQ_WG, 1, 1, false) X(WB, NRQ_WG, 1, 1, true) X(WB, 256, NRQ_SMALL_WV, 1, false) X(WB, 256, NRQ_SMALL_WV, 1, true)           \
  X(WB, 256, 5, 1, false) X(WB, 256, 5, 1, true) X(WB, 64, NRQ_TINY_WV, 1, false) X(WB, 64, NRQ_TINY_WV, 1, true)
#define NRQ_SOLVE_INSTANCES(X)                                                                                                        \
  NRQ_SOLVE_WIDTH(X, 16) X(16, 256, 4, 2, false) X(16, 256, 4, 4, false) X(16, 256, 4, 8, false)                                      \
  X(12, NRQ_WG, 1, 1, false) X(12, NRQ_WG, 1, 1, true)                                                                                \
  NRQ_SOLVE_WIDTH(X, 8) NRQ_SOLVE_WIDTH(X, 4) NRQ_SOLVE_WIDTH(X, 2)

struct SolveKey {
  int WB, NT, WV, G;
  bool AL;
  bool operator==(const SolveKey &o) const { return WB == o.WB && NT == o.NT && WV == o.WV && G == o.G && AL == o.AL; }
};
#define NRQ_SOLVE_KEY(WB, NT, WV, G, AL) {WB, NT, WV, G, AL},
static const SolveKey nrq_solve_keys[] = {NRQ_SOLVE_INSTANCES(NRQ_SOLVE_KEY)};
#undef NRQ_SOLVE_KEY
static const int nrq_solve_nkeys = (int)(sizeof(nrq_solve_keys) / sizeof(nrq_solve_keys[0]));
/* an instance that cannot work (solve_roles.h) fails the host build too, not only the kernels' */
#define NRQ_SOLVE_CHECK(WB, NT, WV, G, AL) static_assert(solve_roles_valid(WB, NT, WV, G, AL), "nrq_solve_kernel<" #WB ", " #NT ", " #WV ", " #G ", " #AL ">");
NRQ_SOLVE_INSTANCES(NRQ_SOLVE_CHECK)
#undef NRQ_SOLVE_CHECK
/* row of a key in nrq_solve_keys[] (and in the launch table made from the same list); -1: not compiled */
static inline int solve_key_index(const SolveKey &k) {
  for (int i = 0; i < nrq_solve_nkeys; i++)
    if (nrq_solve_keys[i] == k) return i;
  return -1;
}

/* nrq_plan_kernel<NT, compact>, in the order their attributes are set */
#define NRQ_PLAN_INSTANCES(X) X(PL_NT, 0) X(PL_NT, 1) X(PL_NT_MIN, 0) X(PL_NT_TINY, 0)
struct PlanKey {
  uint32_t NT, compact;
};
#define NRQ_PLAN_KEY(NT, PK) {NT, PK},
static const PlanKey nrq_plan_keys[] = {NRQ_PLAN_INSTANCES(NRQ_PLAN_KEY)};
#undef NRQ_PLAN_KEY
static const int nrq_plan_nkeys = (int)(sizeof(nrq_plan_keys) / sizeof(nrq_plan_keys[0]));
static inline int plan_key_index(uint32_t nt, uint32_t compact) {
  for (int i = 0; i < nrq_plan_nkeys; i++)
    if (nrq_plan_keys[i].NT == nt && nrq_plan_keys[i].compact == compact) return i;
  return -1;
}

enum ShapeErr {
  SHAPE_OK = 0,
  SHAPE_BLOCK_TOO_LARGE, /* solve_lists: a block's image fits the LDS at no width */
  SHAPE_GRID_TOO_LARGE,  /* solve_shape: more work slots than a 31-bit count */
  SHAPE_BACKSUB_TABLES,  /* solve_shape: the back-substitution tables of a split launch do not fit the LDS */
  SHAPE_PLAN_SEGMENTED   /* plan_shape: a segmented run needs the instance for big blocks */
};

/* ============================================================================================
 * The solve launch(es) of a batch
 * ========================================================================================== */

/* widest width at which the image of h fits the LDS (0: none) and its size there */
static inline uint32_t widest_fit(const Tuning &t, const nrq_plan_hdr *h, uint32_t *need) {
  /* (12 bytes: between the 16-byte image's limit, K ~ 8500, and ~12000; below, a block that does not fit 16 bytes is the odd one
   * of its batch -- a decode plan with many inactive columns -- and goes on the second list at 12 as well) */
  static const uint32_t widths[5] = {16, 12, 8, 4, 2};
  for (int s = 0; s < 5; s++) {
    if (widths[s] > t.max_wb) continue;
    if (widths[s] == 12u && t.no_wb12) continue;
    const uint32_t n = nrq_lds_plan(h, widths[s]).total;
    if (n <= t.lds_max) { *need = n; return widths[s]; }
  }
  *need = 0;
  return 0;
}

/* A launch runs at one strip width, and the widest width a block can have is set by ITS plan (a decode plan's LDS image grows
 * with its inactive columns): at K=8192 one block in a few thousand -- one launch in 40 at 10 % loss, 4 in 40 at 30 % -- does not
 * fit the 16-byte image.  Round 5 sent the whole launch to the width every block fits (8 bytes: ~1.7 x the time for 256 blocks
 * because of one); now the batch is split into at most TWO LISTS -- the blocks that fit the widest width any block has (a), and
 * the others (b), launched at the widest width THEY all fit. */
struct SolveLists {
  ShapeErr err = SHAPE_OK;
  uint32_t nsolv = 0;              /* solvable headers (0: nothing to launch) */
  bool two = false;                /* two lists; else one launch of everybody at wa / need_a */
  uint32_t wa = 0, need_a = 0;     /* strip width and LDS bytes of the (first) list */
  uint32_t wb = 0, need_b = 0;     /* ... of the second, narrower list */
  std::vector<uint8_t> on_b;       /* two lists: per header, 1 = on the second list (unsolvable headers: 0) */
};
/* can_split: the caller knows the block of every header (else all blocks share one plan, or nothing can be moved) */
static inline SolveLists solve_lists(const Tuning &t, const nrq_plan_hdr *const *hdrs, size_t n, bool can_split) {
  SolveLists l;
  uint32_t wb_ = 16, na = 0;
  std::vector<uint32_t> wd(n, 0), nd(n, 0);
  for (size_t i = 0; i < n; i++) {
    if (hdrs[i]->status) continue;
    l.nsolv++;
    wd[i] = widest_fit(t, hdrs[i], &nd[i]);
    if (!wd[i]) { l.err = SHAPE_BLOCK_TOO_LARGE; return l; }
    if (wd[i] > l.wa) l.wa = wd[i];
  }
  if (!l.nsolv) return l;
  for (size_t i = 0; i < n; i++) {
    if (hdrs[i]->status) continue;
    if (wd[i] == l.wa) { na++; if (nd[i] > l.need_a) l.need_a = nd[i]; }
    else if (wd[i] < wb_) wb_ = wd[i];
  }
  const uint32_t nb = l.nsolv - na;
  /* one list: everybody fits the widest width -- or lists are off / impossible (no block indices) / not worth it (the wide list
   * would be the minority: then everybody runs at the narrow width, as before) */
  if (nb == 0 || !can_split || t.no_lists || na < nb) {
    if (nb != 0) l.wa = wb_;
    l.need_a = 0;
    for (size_t i = 0; i < n; i++)
      if (!hdrs[i]->status) { const uint32_t x = nrq_lds_plan(hdrs[i], l.wa).total; if (x > l.need_a) l.need_a = x; }
    return l;
  }
  l.two = true;
  l.wb = wb_;
  l.on_b.assign(n, 0);
  for (size_t i = 0; i < n; i++) {
    if (hdrs[i]->status || wd[i] == l.wa) continue;
    l.on_b[i] = 1;
    const uint32_t x = nrq_lds_plan(hdrs[i], wb_).total;
    if (x > l.need_b) l.need_b = x;
  }
  return l;
}

/* What one solve launch is given ... */
struct SolveIn {
  uint32_t wb = 0, nblk = 0, T = 0; /* strip width of the list, blocks in the launch (the unsolvable ones included), symbol bytes */
  uint32_t lds_bytes = 0;           /* the largest strip image of the list at that width */
  uint32_t max_slots = 0, max_out = 0, max_u = 0, max_wpr = 0; /* over the list's solvable plans: rows M, rows to write, inactive columns, W words */
  bool io_aligned = false;          /* every symbol row of the call is 16-byte aligned */
  const nrq_plan_hdr *const *hdrs = nullptr; /* the list's plan headers: ONE when all blocks share a plan (encode), else one per block */
  size_t nhdrs = 0;
};
/* ... and everything that is decided about it */
struct SolveShape {
  ShapeErr err = SHAPE_OK;
  SolveKey key = {0, 0, 0, 1, false}; /* the instance to launch */
  uint32_t lds_bytes = 0;           /* dynamic LDS of a workgroup (re-derived for wide strips) */
  uint32_t wg_threads = 0, wg_waves = 0; /* the workgroup the sizing is for, as the call stats report it: key.NT / key.WV -- except that
                                     * a wide-strip launch under big_wg (or of a lone block) is sized for the full-size workgroup
                                     * and still runs the 256-thread instance, the only one wide strips have */
  bool split = false;               /* the solve kernel stops after the dense stage: back-substitution and collect kernels follow */
  bool by_block = false;
  uint32_t nstrips = 0, spl = 0;    /* strips of a block; strips per line group */
  uint32_t occ = 0;                 /* workgroups per CU */
  uint32_t grid = 0, lsub = 0, nslots = 0; /* persistent workgroups; log2 of the strips per work slot; work slots */
  uint32_t stage_stride = 0, ostage_stride = 0; /* bytes of one strip's input / output staging buffer */
  /* split launches */
  size_t ybuf_stride = 0;           /* bytes of a block's work buffer: (M + u) full-width rows */
  uint32_t res_elems = 0;           /* rows nrq_collect_kernel writes per block at most */
  uint32_t backsub_strip = 0, backsub_nsb = 0, backsub_tbl = 0, nchunks = 0; /* nrq_backsub_kernel<strip>: grid x, table bytes (LDS), grid y */
  size_t stage_bytes() const { return (size_t)grid * 2u * spl * ((size_t)stage_stride + ostage_stride); }
};

static inline SolveShape solve_shape(const Tuning &t, int ncu, uint32_t ahead_hint, const SolveIn &in) {
  SolveShape s;
  const uint32_t WB = in.wb, nblk = in.nblk, T = in.T, max_slots = in.max_slots;
  uint32_t lds_bytes = in.lds_bytes, max_out = in.max_out;
  /* WIDE strips (G lanes per element, 16 * G bytes per strip; solve_body.h) -- an experiment for small blocks, whose levels
   * hold a dozen ops and whose HDPC / dense phases a dozen rows, so that most lanes of a wave idle through them on a
   * 16-byte strip.  Measured (K=100 / 500 / 1000, G = 8 / 4 / 2, two or three 256-thread workgroups per CU): 270-313 /
   * 600-619 / 727-731 Gbit/s against 326 / 613 / 881 with 16-byte strips: the LDS holds the same number of symbol bytes
   * either way, a strip's chain of phases is no shorter for being wider, and G x fewer virtual threads make its
   * per-thread loops longer.  Not selected automatically; the knob wide_g forces it (tests keep it correct). */
  uint32_t G = 1;
  if (WB == 16 && t.wide_g > 1u && T >= 16u * t.wide_g) {
    uint32_t need = 0;
    for (size_t i = 0; i < in.nhdrs; i++)
      if (!in.hdrs[i]->status) { const uint32_t x = nrq_lds_plan(in.hdrs[i], 16u * t.wide_g).total; if (x > need) need = x; }
    if (lds_alloc(need) * 2u <= NRQ_LDS_MAX) { G = t.wide_g; lds_bytes = need; }
  }
  const uint32_t WBE = WB * G;
  /* narrow strips: the solve kernel stops after the dense stage, nrq_backsub_kernel / nrq_collect_kernel finish on
   * full-width rows of a per-block work buffer (see there) */
  const bool split = WB <= 4 && !t.no_split;
  s.res_elems = max_out;
  if (split) max_out = max_slots + in.max_u;
  const uint32_t nstrips = (T + WBE - 1) / WBE, spl = nrq_group_strips(WBE);
  const bool by_block = nrq_map_by_block(nblk) && !t.map_spread;
  /* workgroup shape: the full-size workgroup when a strip image needs more than half of the CU's LDS, 256-thread ones
   * when two or more fit */
  /* (a launch whose strips each get a CU of their own -- a lone block of the reference's harness -- takes the full-size workgroup from
   * K ~ 1200 on: encode column of benchmark.c K=1500 208 -> 225 Gbit/s, K=3000 294 -> 315, K=4000 313 -> 333; below, the same) */
  const bool lone = (uint64_t)nblk * ((T + WB - 1) / WB) <= (uint64_t)ncu && max_slots >= 1200u && !t.tiny_any;
  const bool small = WB != 12 && lds_alloc(lds_bytes) * t.small_div <= NRQ_LDS_MAX && !t.big_wg && !lone; /* (12-byte strips: big blocks) */
  /* single-wave workgroups when 12 or more images fit a CU (see the kernel; K=256: +26 % over five 256-thread workgroups) */
  const uint32_t tdiv = in.nhdrs > 1u ? t.tiny_div_dec : t.tiny_div;
  /* ... and when the launch has the strips to fill them: a lone block's 80 strips each get a 256-thread workgroup and a CU of their own
   * (the reference's benchmark.c, one block per call, K=500: encode column 81 -> 106 Gbit/s without the single-wave form; from ~1000
   * strips on -- 16 blocks of K=500 -- the single-wave form is the faster one again: 0.07 against 0.09 ms) */
  const bool tiny = G == 1 && small && (uint64_t)lds_alloc(lds_bytes) * tdiv <= NRQ_LDS_MAX && !t.no_tiny &&
                    ((uint64_t)nblk * nstrips > 2u * (uint64_t)ncu || t.tiny_any);
  const uint32_t nt = tiny ? 64u : small ? 256u : (uint32_t)NRQ_WG;
  uint32_t occ = NRQ_LDS_MAX / lds_alloc(lds_bytes ? lds_bytes : 1u);
  if (occ > 2048u / nt) occ = 2048u / nt;
  /* registers: the 256-thread variant (one wave per SIMD) is compiled for NRQ_SMALL_WAVES waves per SIMD.  More
   * workgroups than are resident at once would run as a second, thinner round of a statically partitioned job. */
  const bool five = G == 1 && small && !tiny && occ >= 5u && !t.small_waves4;
  if (tiny) { if (occ > NRQ_TINY_OCC) occ = NRQ_TINY_OCC; } /* one wave per workgroup, compiled for 5 waves per SIMD; 20 per CU by the LDS sum, but
                                              * measured: with 20 x 256 workgroups not all are resident and the rest runs as a second
                                              * round (10.4 ms against 8.7 ms with 18 x 256 at K=100, T=1024, 8192 blocks) */
  else if (small && occ > (five ? 5u : (uint32_t)NRQ_SMALL_WV)) occ = five ? 5u : (uint32_t)NRQ_SMALL_WV;
  if (occ < 1u) occ = 1u;
  /* persistent workgroups fill the device; a multiple of 8 keeps a workgroup's slots on its XCD */
  uint64_t grid = (uint64_t)(ncu / 8) * 8 * occ;
  /* A batch of few big blocks: leave a compute unit per block (one per XCD at least) to the planner workgroups of the
   * decode that follows or runs beside this launch on the context's planner stream (decode_device) -- a planner
   * workgroup needs a whole CU's LDS, and the persistent workgroups of this launch would otherwise hold every CU until
   * they are all done.  ~3 % of the solve's throughput for 8 blocks; the planner (one workgroup per block, latency
   * bound: 12 ms at K=27000, 36 ms at K'=56403) then hides behind the encode solve. */
  if (!small && occ == 1u) {
    /* (with planner runs issued ahead -- nrq_decode_plan_ahead -- up to `ahead_hint` batches' planner workgroups are resident at
     * once, and the encode plan of a big block is built by one more workgroup on a stream of its own: without a compute unit
     * for each of them one waits until this launch's persistent workgroups are through, and its 20-30 ms start from there) */
    const uint32_t runs = ahead_hint > 1u ? ahead_hint : 1u;
    uint32_t reserve = t.reserve_cus >= 0 ? (uint32_t)t.reserve_cus : (nblk <= 16u ? (nblk * runs + 1u + 7u) / 8u * 8u : 0u);
    if (reserve + 64u <= grid) grid -= reserve / 8u * 8u;
  }
  if (t.solve_grid) grid = t.solve_grid / 8 * 8;
  if (grid < 8) grid = 8;
  /* work slots (nrq_map_group): `sub` strips of a block each -- the strips of a whole line unless that would leave
   * workgroups idle -- incl. the empty slots of a partial block octet */
  uint32_t lsub = 0;
  while ((1u << lsub) < spl) lsub++;
  auto slots_for = [&](uint32_t ls) -> uint64_t {
    const uint32_t sub = 1u << ls, spb = (nstrips + sub - 1) / sub;
    return by_block ? (uint64_t)((nblk + 7u) / 8u) * 8u * spb : (uint64_t)nblk * spb;
  };
  while (lsub > 0 && slots_for(lsub) < grid) lsub--;
  {
    /* Work is dealt statically (workgroup g takes slots g, g + grid, ...): with few big blocks the rounds do not come
     * out even -- K'=56403, 8 blocks: 320 whole-line slots on 256 workgroups is two rounds for a quarter of them, 32
     * strips against 20 on average.  Smaller slots even that out; what they cost is gather efficiency (pieces shorter
     * than a 128-byte line), which matters for wide strips only: a 2- or 4-byte strip is solved at the same cost per
     * strip as a 16-byte one, so its data movement is an eighth or a quarter of the time share. */
    auto max_strips = [&](uint32_t ls) -> uint64_t {
      const uint64_t ns = slots_for(ls), g = grid < ns ? grid : ns;
      return ((ns + g - 1) / g) << ls;
    };
    const uint32_t min_ls = WB >= 8 ? (lsub < 2u ? lsub : 2u) : 0u;
    uint32_t best = lsub;
    for (uint32_t ls = lsub; ls-- > min_ls;)
      if (max_strips(ls) * 100u < max_strips(best) * 93u) best = ls;
    if (!t.no_balance) lsub = best;
  }
  const uint64_t nslots = slots_for(lsub);
  if (nslots > 0x7FFFFFFFull) { s.err = SHAPE_GRID_TOO_LARGE; return s; }
  if (grid > nslots) grid = by_block ? (nslots + 7) / 8 * 8 : nslots;
  /* the instance.  (The movers' aligned-only form; 12-byte strips: whole dwords, solve_body.h g_get_al12) */
  const bool al = in.io_aligned && G == 1 && WB >= 4 && T % (uint32_t)(WB == 12 ? 4 : WB) == 0u;
  s.wg_threads = nt;
  s.wg_waves = tiny ? (uint32_t)NRQ_TINY_WV : five ? 5u : small ? (uint32_t)NRQ_SMALL_WV : 1u;
  if (G > 1) s.key = {16, 256, 4, (int)G, false};
  else s.key = {(int)WB, (int)nt, (int)s.wg_waves, 1, al}; /* (12-byte strips are never `small`: the full-size workgroup) */
  s.lds_bytes = lds_bytes;
  s.split = split; s.by_block = by_block; s.nstrips = nstrips; s.spl = spl; s.occ = occ;
  s.grid = (uint32_t)grid; s.lsub = lsub; s.nslots = (uint32_t)nslots;
  /* per workgroup: two sets of `spl` input staging buffers (the line group being solved, the one being gathered)
   * and two sets of `spl` output staging buffers (the group being solved, the one being scattered) */
  s.stage_stride = (max_slots * WBE + 255u) & ~255u;
  s.ostage_stride = (max_out * WBE + 255u) & ~255u;
  if (split) {
    s.ybuf_stride = ((size_t)(max_slots + in.max_u) * T + 255u) & ~(size_t)255u;
    /* 32-byte strips while the tables (4 KiB per W word) leave room for two workgroups per CU, 16-byte strips beyond */
    const uint32_t sb = in.max_wpr <= 20u && t.backsub_sb != 16u ? 32u : 16u, nsb = (T + sb - 1u) / sb;
    s.backsub_strip = sb; s.backsub_nsb = nsb; s.backsub_tbl = in.max_wpr * 8u * 16u * sb;
    if (s.backsub_tbl > NRQ_LDS_MAX) { s.err = SHAPE_BACKSUB_TABLES; return s; } /* (launch_solve refuses the call, before any launch) */
    uint32_t nchunks = (2048u + nsb * nblk - 1u) / (nsb * nblk);
    if (nchunks < 1u) nchunks = 1u;
    if (nchunks > 16u) nchunks = 16u;
    s.nchunks = nchunks;
  }
  return s;
}

/* ============================================================================================
 * The planner run (the decode planner and the device build of encode plans)
 * ========================================================================================== */

/* Big blocks, whose peeling state does not fit the LDS next to the dense-stage reserve (pl_ctx_setup's rule), run the
 * planner in two parts with helper kernels between and after them (planner_seq.h).  The jobs carry the choice in
 * bit 8 of nrq_planjob::mode (pl_final_c then leaves the W transposition to nrq_wt_kernel). */
static inline bool plan_is_segmented(const Tuning &t, uint32_t L, uint32_t Mcap) {
  const uint32_t sh_bytes = pl_shared_bytes(PL_QCAP, PL_LOWCAP, PL_NT), dyn = NRQ_LDS_MAX - sh_bytes;
  if (t.plan_split_force) return true; /* (tests: the segmented path at sizes the oracle checks quickly) */
  return pl_state_in_lds(L, Mcap, dyn) == 0u && !t.no_plan_split;
}

struct PlanShape {
  ShapeErr err = SHAPE_OK;
  /* the instance nrq_plan_kernel<wg_threads, compact> (nrq_call_stats::plan_wg_threads, plan_compact_state, plan_segmented) */
  uint32_t wg_threads = 0, compact = 0, segmented = 0;
  uint32_t mode = 0;                /* nrq_planjob::mode, bit 8: segmented run, bit 9: entry pass by nrq_wentry_kernel, bit 10: no out view (tests) */
  uint32_t nparts = 0, parts[3] = {0, 0, 0}; /* the kernel's `seg` argument, launch by launch: everything | 3, (entry pass), 4, (W pass, HDPC fold), 2 */
  uint32_t qcap = 0, lowcap = 0, sh_bytes = 0, dyn_bytes = 0; /* capacities and bytes of the workgroup state; dynamic LDS in front of it */
  /* helper kernels of a segmented run, per block: workgroups and LDS bytes */
  uint32_t wentry_wgs = 0;          /* nrq_wentry_kernel (behind part 3), LDS sh_bytes */
  uint32_t wpass_wgs = 0, wpass_lds = 0; /* nrq_wpass_kernel (behind parts 1 and 4) */
  uint32_t mh_wgs = 0, mh_dyn = 0;  /* nrq_mh_kernel (behind it), LDS mh_dyn + sh_bytes */
};

static inline PlanShape plan_shape(const Tuning &t, int ncu, const rq_params &p, uint32_t nblk, uint32_t Mcap, uint32_t ucap) {
  PlanShape s;
  /* The workgroup state (pl_shared and the arrays behind it: frontier queues, claim lists, per-thread scratch, Gauss-Jordan
   * flags) is sized by the launch: 25 KB for big blocks; a small block's frontier and dense stage need a fraction, and
   * with 8 KB of it four 256-thread planner workgroups share a CU instead of two (the planner is latency bound: twice
   * the workgroups, half the time).  Overflowing a capacity is reported as such and re-planned on the host. */
  uint32_t qcap = PL_QCAP, lowcap = PL_LOWCAP;
  uint32_t sh_bytes = pl_shared_bytes(qcap, lowcap, PL_NT);
  /* dynamic LDS: everything a CU has for a big block; for small blocks what the planner can use (peeling state plus the
   * dense-stage reserve, or a 16-byte strip image of the W rows), so that several workgroups share a CU */
  uint32_t dyn_bytes = NRQ_LDS_MAX - sh_bytes;
  bool small_wg = false; /* 256-thread workgroups: a small block has no use for 1024 threads, a CU has for 4 blocks */
  bool tiny_wg = false;  /* 128-thread workgroups (with small_wg) */
  {
    const uint32_t peel = 2u * pl_r16(Mcap * 4u) + pl_r16(p.L * 4u) + pl_dense_reserve(p.L);
    const uint32_t wimg = (Mcap + 320u + NRQ_SCRATCH) * 16u;
    const uint32_t fit = pl_r16((peel > wimg ? peel : wimg) + 2048u);
    /* (queues / claim lists / Gauss-Jordan flags: a frontier, a round's claims and the leftover rows are at most the block's rows) */
    const uint32_t q_s = Mcap <= 248u ? 256u : p.L <= 1500u ? 512u : 1024u, low_s = Mcap <= 248u ? 256u : p.L <= 1500u ? 384u : 768u;
    const uint32_t sh_s = t.plan_small_state ? pl_shared_bytes(q_s, low_s, PL_NT_MIN) : sh_bytes;
    /* ... when there are more blocks than compute units.  A batch of at most one block per CU gains nothing from sharing: every block
     * gets the 1024-thread workgroup and the whole LDS (round 6, planner per batch, 256-thread / 1024-thread workgroups: K=500 x 256
     * blocks 0.55 / 0.39 ms, K=1000 x 256 0.53 / 0.44, K=2500 x 256 0.95 / 0.69, K=2500 x 64 1.15 / 0.79; one block of K=2500 through
     * the reference's benchmark.c: decode column 24.1 -> 30.8 Gbit/s).  The knob plan_pack packs regardless (tests of the small forms). */
    const bool pack = nblk > (uint32_t)ncu || t.plan_pack;
    if (lds_alloc(fit + sh_s) <= NRQ_LDS_MAX / 2u && !t.plan_lds_max) {
      dyn_bytes = fit; /* (also for the 1024-thread workgroup of a small batch: it then leaves LDS and wave slots to a solve running beside it) */
      small_wg = !t.plan_big_wg && pack;
      if (small_wg && t.plan_small_state) { qcap = q_s; lowcap = low_s; sh_bytes = sh_s; }
      /* The smallest blocks: 128 threads.  A planner phase is one wave's chain of instructions and trips,
       * the other waves of the workgroup mostly wait; the registers of the kernel (~100) let a CU hold 20 waves -- five
       * 256-thread workgroups, or as many 128-thread ones as the LDS takes (six or more from here on): more blocks in flight
       * for the same waves. */
      const uint32_t sh_t = pl_shared_bytes(q_s, low_s, PL_NT_TINY);
      if (small_wg && t.plan_small_state && !t.plan_no_wg128 && lds_alloc(fit + sh_t) * 6u <= NRQ_LDS_MAX) { tiny_wg = true; sh_bytes = sh_t; }
    }
  }
  const bool seg = plan_is_segmented(t, p.L, Mcap);
  if (seg && t.plan_split_force) {
    /* a segmented run keeps nothing in LDS between its parts: its peeling state must live in the workspace, which
     * pl_ctx_setup chooses when the dynamic region is too small for it -- so make it too small (dense stage only) */
    const uint32_t need = 2u * pl_r16(Mcap * 4u) + pl_r16(p.L * 4u);
    uint32_t only_dense = (pl_dense_reserve(p.L) + need - 16u) & ~15u; /* 16 bytes short of holding the peeling state */
    if (only_dense < dyn_bytes) dyn_bytes = only_dense;
    if (pl_state_in_lds(p.L, Mcap, dyn_bytes) != 0u) dyn_bytes = (need - 16u) & ~15u; /* (... also for the form that shares the rowstate image) */
    small_wg = false; tiny_wg = false;
    qcap = PL_QCAP; lowcap = PL_LOWCAP; sh_bytes = pl_shared_bytes(qcap, lowcap, PL_NT);
  }
  const bool wentry = seg && !t.no_wentry;
  const bool hbm_state = pl_state_in_lds(p.L, Mcap, dyn_bytes) == 0u; /* (pl_ctx_setup's rule, on the dynamic bytes as they are NOW) */
  s.nparts = !seg ? 1u : wentry ? 3u : 2u;
  if (seg) { s.parts[0] = wentry ? 3u : 1u; s.parts[1] = wentry ? 4u : 2u; s.parts[2] = 2u; }
  s.segmented = seg ? 1u : 0u;
  s.mode = (seg ? (t.no_wentry ? 0x100u : 0x300u) : 0u) | (t.plan_no_out_view ? PL_MODE_NO_OUTW : 0u);
  if (seg && (tiny_wg || small_wg || !hbm_state)) s.err = SHAPE_PLAN_SEGMENTED;
  s.wg_threads = tiny_wg ? (uint32_t)PL_NT_TINY : small_wg ? (uint32_t)PL_NT_MIN : (uint32_t)PL_NT;
  /* (the state stays in HBM; plan_wrong_instance names this instance for blocks whose state does not) */
  s.compact = !tiny_wg && !small_wg && (hbm_state || t.plan_wrong_instance) ? 1u : 0u;
  s.qcap = qcap; s.lowcap = lowcap; s.sh_bytes = sh_bytes; s.dyn_bytes = dyn_bytes;
  s.wentry_wgs = 64u / (nblk ? nblk : 1u); /* workgroups per block: what a batch of few big blocks finds free beside the solves */
  if (s.wentry_wgs < 2u) s.wentry_wgs = 2u;
  if (s.wentry_wgs > 8u) s.wentry_wgs = 8u;
  s.wpass_wgs = ((ucap + 31u) / 32u) * 2u;
  s.wpass_lds = (Mcap + NRQ_SCRATCH) * 2u + 64u;
  s.mh_wgs = 256u / (nblk ? nblk : 1u); /* the HDPC fold: as many workgroups per block as leave the whole batch ~256 */
  if (s.mh_wgs < 1u) s.mh_wgs = 1u;
  if (s.mh_wgs > 64u) s.mh_wgs = 64u;
  s.mh_dyn = 72u * 1024u; /* nrq_mh_kernel: MhT (16 B x u <= 20 KB) + the tiles (4 KB + 256 x wpr words <= 40 KB) */
  return s;
}

#endif /* NRQ_LAUNCH_SHAPE_H */
