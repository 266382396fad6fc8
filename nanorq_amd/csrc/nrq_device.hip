/*
 * nrq_device.hip -- gfx950 kernels and the C ABI of include/nanorq_hip.h.
 *
 * Kernels
 *   nrq_solve_kernel<WB,NT,WV>  the whole data stage of the precode solve: persistent workgroups, one WB-byte column
 *                            strip of one source block at a time, LDS-resident (phases in solve_body.h)
 *   nrq_plan_kernel          the symbolic stage of a decode block (phases in planner_body.h, order in planner_seq.h)
 *   nrq_gen_kernel           LT symbol generation from intermediate symbols in HBM
 *                            (reference decode_row, nanorq.c:184-204)
 * Host side: context, per-K' caches, plan staging, batching, launch geometry.
 * MI355X only: wave64, 160 KiB LDS per workgroup, XCD-aware placement of the work.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../include/nanorq_hip.h"
#include "plan.h"
#include "planner_host.h"
#include "rq_math.h"
#include "out_lists.h"
#include "solve_body.h"
#include "split_body.h"
#include "planner_body.h"
#include "ingest_body.h"
#include "ingest_set_body.h"
#include "lists_set_body.h"
#include "rxset_plan.h"
#include "held_body.h"
#include "want_body.h"
#include "want_set_body.h"
#include "emit_body.h"
#include "emit_set_body.h"
#include "emit_set_range_body.h"
#include "syms_body.h"
#include "syms_set_body.h"
#include "runs_body.h"
#include "runs_set_body.h"
#include "obj_body.h"
static_assert(RQ_LT_COLS_MAX_REAL <= NRQ_LT_LIST_MAX, "solve_body.h sizes the slack behind out_slots[] for the longest LT list");
static_assert(RQ_LT_COLS_MAX_REAL <= TX_COLS, "emit_body.h sizes a packet's column list for the longest LT list");

#include "launch_shape.h" /* the knobs, the solve kernel's roles (solve_roles.h), the instance lists, what a launch looks like: host code the tests compile on their own */

#define NRQ_GEN_WG 256

/* ============================================================================================
 * Kernels
 * ========================================================================================== */

/* (nrq_map_group / nrq_next_group, which deal the work slots to the workgroups, are in solve_body.h: the launch emulation of
 * tests/emu runs the same two functions) */

/* The data stage: persistent workgroups, one line group at a time, its strips one after the other (solve_body.h:
 * load -> forward passes -> HDPC -> dense stage -> back-substitution -> store).  While wave 0 runs the forward
 * passes of a strip, a few of the other waves gather a portion of the NEXT line group into the input staging
 * buffers and scatter a portion of the PREVIOUS group's results from the output staging buffers to their rows. */
/* NT threads per workgroup: NRQ_WG when one strip image owns the CU's LDS (big blocks), 256 when several fit (small
 * blocks: more workgroups per CU beat more waves per workgroup, each has its own single-wave forward pass).
 * `lsub`: log2 of the strips per work slot -- a whole line (128/WB strips) unless that leaves CUs without work. */
/* WV: waves per SIMD the kernel is compiled for, i.e. its register budget (512 / WV).  The 768-thread variant has
 * the CU to itself (3 waves per SIMD, 168 registers).  The 256-thread variant puts one wave on every SIMD, so WV is
 * also the number of workgroups a CU holds: 4 (128 registers) or, when the LDS images are small enough for 5
 * workgroups, 5 (96 registers, a few more spills).  Left to itself the compiler took 207 registers: 2 workgroups. */
/* G > 1: WIDE strips -- an element is G adjacent 16-byte columns, one lane each (solve_body.h): thread t is lane t % G of
 * virtual thread t / G, and every phase runs on the NT / G virtual threads.  For small blocks. */
/* AL: every symbol row of the launch is aligned to the strip width and T is a multiple of it (the host checks): the movers are
 * then compiled WITHOUT their byte-wise forms -- with both forms at every call site the kernels were half as large again
 * (persistent workgroups in different phases share the instruction cache), and a byte-wise path inside a mover loop makes the
 * compiler wait for all loads in flight where the paths join. */
#ifndef NRQ_PROF_DONE
#define NRQ_PROF_DONE 9 /* NRQ_PROF samples this strip (counted from 0) of every 16th workgroup.  It must lie behind the workgroup's FIRST work
                         * slot to see a scatter at all (the first slot has no results of a slot before it to move): strip 9 is in the second
                         * slot when slots are 8 strips (16- and 12-byte strips), in the first when they are 16 or more (8 bytes and narrower) */
#endif
template <int WB, int NT, int WV, int G = 1, bool AL = false>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(WV)))
void nrq_solve_kernel(const nrq_job *__restrict__ jobs, uint32_t nblk,
                                                       uint32_t T, uint32_t nstrips, uint32_t by_block, uint32_t nslots,
                                                       uint32_t lsub, const uint8_t *__restrict__ kc,
                                                       uint8_t *__restrict__ stage_all, uint32_t stage_stride,
                                                       uint32_t ostage_stride, unsigned long long *__restrict__ prof,
                                                       uint8_t *__restrict__ ybuf, size_t ybuf_stride) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const uint32_t tid = threadIdx.x;
  static_assert(solve_roles_valid(WB, NT, WV, G, AL), "wide strips are 16-byte lanes, 12-byte strips need the 768-thread workgroup, several waves need two movers");
  /* who runs the forward passes, who moves data and in which form, the phases' forms: solve_roles.h.  (R is read in constant
   * expressions only: read at run time it would be an object in the kernel's frame.) */
  constexpr SolveRoles R = solve_roles(WB, NT, WV, G, AL);
  constexpr uint32_t WBE(R.WBE), VNT(R.VNT), SPL(nrq_group_strips(WBE)), NFW(R.NFW), NGW(R.NGW), NSW(R.NSW), RU(R.RU), HNT(R.HNT), SLATE(R.SLATE), GLATE(R.GLATE);
  constexpr bool MPIPE(R.MPIPE), ALX(R.ALX), LATE(R.LATE);
  const uint32_t vt = tid / G, subl = tid % G; /* virtual thread, lane inside it */
  /* NT == 64: ONE wave solves the strip on its own (no mover waves: it gathers and scatters its portions itself after
   * the forward passes; barriers are free).  For images of a few KB -- K up to ~400 -- where a strip is a chain of
   * short phases with little parallel work: 19-20 such workgroups share a CU instead of five 256-thread ones, i.e.
   * four times as many strips are in flight to hide the phases' latencies. */
  const uint32_t sub = 1u << lsub;               /* strips per slot */
  const uint32_t gpb = (nstrips + sub - 1u) / sub; /* slots per block */
  /* per workgroup: two sets of SPL input staging buffers (the group being solved, the group being gathered) and two
   * sets of SPL output staging buffers (the group being solved, the group being scattered) */
  const size_t wg_bytes = 2u * SPL * ((size_t)stage_stride + ostage_stride);
  (void)SPL;
  NRQ_GAS uint8_t *stage0 = gptr_w<uint8_t>((uint64_t)(uintptr_t)(stage_all + (size_t)blockIdx.x * wg_bytes));
  NRQ_GAS uint8_t *ostage0 = stage0 + 2u * SPL * (size_t)stage_stride;
  uint32_t q = nrq_next_group(blockIdx.x, gridDim.x, nslots, jobs, nblk, gpb, by_block != 0u);
  if (q >= nslots) return;
  uint32_t buf = 0, done = 0, qp = nslots; /* qp: the group whose results wait in the other output set */
  {
    GroupSrc<WB> g0;
    uint32_t b0;
    nrq_group_src<WB>(q, jobs, nblk, gpb, by_block, sub, T, nstrips, lsub, g0, &b0);
    pf_gather_impl<WB, G, MPIPE, ALX>(g0, stage0, stage_stride, 0u, g0.M << lsub, (tid) / G, (NT) / G, subl); /* the first group: nothing to overlap it with */
    __syncthreads();
  }
  while (q < nslots) {
    const uint32_t qn = nrq_next_group(q + gridDim.x, gridDim.x, nslots, jobs, nblk, gpb, by_block != 0u);
    GroupSrc<WB> gn;
    GroupDst<WB> gp;
    uint32_t blk, blkn = 0, units_n = 0, units_p = 0;
    if (qn < nslots) { nrq_group_src<WB>(qn, jobs, nblk, gpb, by_block, sub, T, nstrips, lsub, gn, &blkn); units_n = gn.M << lsub; }
    if (qp < nslots) units_p = nrq_group_dst<WB>(qp, jobs, nblk, gpb, by_block, sub, T, nstrips, lsub, ybuf, ybuf_stride, gp) << lsub;
    {
      GroupSrc<WB> gc;
      nrq_group_src<WB>(q, jobs, nblk, gpb, by_block, sub, T, nstrips, lsub, gc, &blk);
    }
    NRQ_GAS uint8_t *stage_cur = stage0 + (size_t)buf * SPL * stage_stride, *stage_nxt = stage0 + (size_t)(buf ^ 1u) * SPL * stage_stride;
    NRQ_GAS uint8_t *ostage_cur = ostage0 + (size_t)buf * SPL * ostage_stride, *ostage_prv = ostage0 + (size_t)(buf ^ 1u) * SPL * ostage_stride;
    const uint32_t strip0 = ((by_block ? (q >> 3) : q) % gpb) * sub;
    for (uint32_t sidx = 0; sidx < sub; sidx++) {
      /* this strip index's portions of the next group's gather and of the previous group's scatter; [um, u1) and [sm, s1) of them
       * are left to the waves that the HDPC phase does not use (when there are any) */
      const uint32_t u0 = NRQ_PORTION_AT(units_n, sidx, lsub), u1 = NRQ_PORTION_AT(units_n, sidx + 1u, lsub);
      const uint32_t s0 = NRQ_PORTION_AT(units_p, sidx, lsub), s1 = NRQ_PORTION_AT(units_p, sidx + 1u, lsub);
      const uint32_t sm = NRQ_PORTION_LATE_AT(s0, s1, SLATE, LATE);
      const uint32_t um = NRQ_PORTION_LATE_AT(u0, u1, GLATE, LATE);
      const uint32_t strip = strip0 + sidx;
      if (strip >= nstrips) { /* no such strip: everybody moves this portion */
        if (u1 > u0) pf_gather_impl<WB, G, MPIPE, ALX>(gn, stage_nxt, stage_stride, u0, u1, (tid) / G, (NT) / G, subl);
        if (s1 > s0) pf_scatter_impl<WB, G, MPIPE, ALX>(gp, ostage_prv, ostage_stride, s0, s1, (tid) / G, (NT) / G, subl);
        continue;
      }
      StripCtx<WB, G> c;
      c.job = jobs + blk;
      c.plan = reinterpret_cast<const uint8_t *>(c.job->plan);
      c.h = reinterpret_cast<const nrq_plan_hdr *>(c.plan);
      c.kc = kc;
      c.lds = smem + subl * WB;
      c.lay = nrq_lds_plan(c.h, WBE);
      c.T = T;
      c.strip = strip;
      const uint32_t at = strip * WBE + subl * WB, rem = at < T ? T - at : 0u;
      c.valid = rem < (uint32_t)WB ? rem : (uint32_t)WB;
      const uint32_t lpr_ = c.h->lpr; /* (fetched here, with the header fields the first phases need: not a trip of its own later) */
      /* NRQ_PROF=1 debugging aid: shader-clock stamps at phase boundaries, the 10th strip of every 16th workgroup */
      unsigned long long *stamp = nullptr;
      const bool sampled = prof && (blockIdx.x & 15u) == 0 && done == (uint32_t)NRQ_PROF_DONE;
      if (sampled && tid == 0) stamp = prof + (size_t)(blockIdx.x >> 4) * 16;
#define NRQ_STAMP(i) do { if (stamp) stamp[i] = (unsigned long long)clock64(); } while (0)
      /* -DNRQ_STOP_AFTER=p (tools/phase_counters.sh): a strip ends behind phase p -- 0 load, 1 forward, 2 HDPC, 3 GF(2) combinations,
       * 4 dense, 5 tables, 6 back-substitution (7 = the whole strip) -- so that the hardware counters of the variants p and p - 1
       * differ by what phase p costs (phases are separated by workgroup barriers).  Results are garbage; nothing reads them. */
#ifdef NRQ_STOP_AFTER
#define NRQ_STOP(p) if ((NRQ_STOP_AFTER) == (p)) { __syncthreads(); continue; }
#else
#define NRQ_STOP(p)
#endif
      c.dbg = sampled ? prof + (size_t)(blockIdx.x >> 4) * 16 + 9 : nullptr;
      c.dbg_t0 = tid == 0;
      done++;
      NRQ_STAMP(0);
      pf_commit<WB, G, R.commit_pb>(c, stage_cur + (size_t)sidx * stage_stride + subl * WB, 0u, vt, VNT);
      ph_clear<WB, G>(c, vt, VNT);
      __syncthreads();
      NRQ_STAMP(1);
      NRQ_STOP(0)

      /* forward passes (plan.h): wave 0 walks the op stream alone (fwd_rows).  A few waves move data meanwhile -- few,
       * because the forward passes leave them plenty of time and a deep queue of their requests in the CU's memory
       * pipeline would delay the op words wave 0 is waiting for */
      const uint32_t wv = tid >> 6;
      if constexpr (NT == 64) {
        if constexpr (G > 1) fwd_rows_wide<G>(c.template arr<uint32_t>(c.h->off_ops), c.h->nrows, tid);
        else fwd_rows<WB, RU>(c.template arr<uint32_t>(c.h->off_ops), c.h->nrows, tid);
        if (u1 > u0) pf_gather_impl<WB, G, MPIPE, ALX>(gn, stage_nxt, stage_stride, u0, u1, (tid) / G, (64u) / G, subl);
        if (sm > s0) pf_scatter_impl<WB, G, MPIPE, ALX>(gp, ostage_prv, ostage_stride, s0, sm, (tid) / G, (64u) / G, subl);
      } else if (wv < NFW) {
        __builtin_amdgcn_s_setprio(3); /* the critical waves: ahead of the others at instruction issue */
        const NRQ_GAS uint32_t *ops_ = c.template arr<uint32_t>(c.h->off_ops);
        if constexpr (G > 1) {
          fwd_rows_wide<G>(ops_, c.h->nrows, tid);
        } else if constexpr (NFW == 3u) { /* 12-byte strips: a dword of the strip width each */
          if (wv == 0u) fwd_rows_third<0, RU>(ops_, c.h->nrows, tid);
          else if (wv == 1u) fwd_rows_third<4, RU>(ops_, c.h->nrows, tid & 63u);
          else fwd_rows_third<8, RU>(ops_, c.h->nrows, tid & 63u);
        } else if constexpr (NFW == 2u && WB == 12) { /* 12-byte strips on two waves: dwords 0 and 1, dword 2 */
          if (wv == 0u) fwd_rows_two_thirds<RU>(ops_, c.h->nrows, tid);
          else fwd_rows_third<8, RU>(ops_, c.h->nrows, tid & 63u);
        } else if constexpr (NFW == 2u) { /* one half of the strip width each */
          /* (the big workgroup has the registers for the deep ring: 168 per thread) */
          if (wv == 0u) fwd_rows_half<WB, 0, RU>(ops_, c.h->nrows, tid);
          else fwd_rows_half<WB, WB / 2, RU>(ops_, c.h->nrows, tid & 63u);
        } else {
          fwd_rows<WB, RU>(ops_, c.h->nrows, tid);
        }
        __builtin_amdgcn_s_setprio(0);
        NRQ_MARK(c, 1);
      } else if (NRQ_WAVE_MOVES(NFW, wv)) { /* the waves that do not share a SIMD with the forward waves; index among them: */
        const uint32_t mv = NRQ_MOVER_INDEX(NFW, wv);
        if (mv < NGW) {
#if !defined(NRQ_EXPERIMENT_NO_MOVERS) && !defined(NRQ_EXPERIMENT_NO_GATHER) /* (measurement only: what the forward window costs with no mover traffic beside it; results are garbage) */
          if (um > u0) pf_gather_impl<WB, G, MPIPE, ALX>(gn, stage_nxt, stage_stride, u0, um, (mv * 64u + (tid & 63u)) / G, (NGW * 64u) / G, subl);
#endif
          NRQ_MARK_MAX(c, 2);
        } else if (mv < NGW + NSW) {
#if !defined(NRQ_EXPERIMENT_NO_MOVERS) && !defined(NRQ_EXPERIMENT_NO_SCATTER)
          if (sm > s0) pf_scatter_impl<WB, G, MPIPE, ALX>(gp, ostage_prv, ostage_stride, s0, sm, ((mv - NGW) * 64u + (tid & 63u)) / G, (NSW * 64u) / G, subl);
#endif
          NRQ_MARK_MAX(c, 3);
        }
      }
      __syncthreads();
      NRQ_STAMP(2);
      NRQ_STOP(1)

      if (tid < HNT) { ph_hdpc<WB, G, R.hdpc_regs>(c, tid / G, HNT / G); }
      else { /* the waves HDPC leaves idle */
        if (u1 > um) pf_gather_impl<WB, G, MPIPE, ALX>(gn, stage_nxt, stage_stride, um, u1, (tid - HNT) / G, (NT - HNT) / G, subl);
        if (s1 > sm) pf_scatter_impl<WB, G, MPIPE, ALX>(gp, ostage_prv, ostage_stride, sm, s1, (tid - HNT) / G, (NT - HNT) / G, subl);
      }
      __syncthreads();
      ph_hdpc_reduce<WB, G>(c, vt, VNT);
      __syncthreads();
      NRQ_STAMP(3);
      NRQ_STOP(2)
      /* the GF(2) combinations E_p of the dense stage: tables over the leftover rows in region X (zero again after the
       * reduce above), as many words of the bit rows at a time as it holds */
      for (uint32_t w0 = 0; w0 < lpr_; w0 += low_table_words<WB, G>(c)) {
        uint32_t cb_[NRQ_COMBINE_WU];
        ph_low_tables<WB, G>(c, w0, vt, VNT);
        ph_combine_fetch<WB, G>(c, w0, vt, VNT, cb_);
        __syncthreads();
        ph_combine<WB, G>(c, w0, vt, VNT, cb_);
        __syncthreads();
      }
      if (lpr_) { /* (0: the combinations were ops of the stream -- small blocks) */
        ph_clear_x<WB, G>(c, vt, VNT);
        __syncthreads();
      }
      NRQ_STAMP(4);
      NRQ_STOP(3)
      ph_dense_fold<WB, G, R.fold_batch>(c, vt, VNT);
      __syncthreads();
      NRQ_MARK(c, 4);
      if (dense_fold_shared(VNT) || G > 1) { /* (then the fold leaves its products in the accumulator copies) */
        ph_hdpc_reduce<WB, G>(c, vt, VNT);
        __syncthreads();
      }
      NRQ_MARK(c, 5);
      ph_dense_free<WB, G, R.batch>(c, vt, VNT);
      __syncthreads();
      NRQ_MARK(c, 6);
      ph_dense_cu<WB, G, R.batch>(c, vt, VNT);
      __syncthreads();
      NRQ_STAMP(5);
      NRQ_STOP(4)
      if (ybuf) { /* split solve (narrow strips): back-substitution and results are nrq_backsub_kernel / nrq_collect_kernel */
        NRQ_STAMP(6);
        NRQ_STAMP(7);
        ph_store_raw<WB, G>(c, ostage_cur + (size_t)sidx * ostage_stride + subl * WB, vt, VNT);
      } else {
        ph_tables<WB, G>(c, vt, VNT);
        __syncthreads();
        NRQ_STAMP(6);
        NRQ_STOP(5)
        ph_backsub<WB, G, R.fast>(c, vt, VNT);
        ph_park<WB, G>(c, vt, VNT);
        __syncthreads();
        NRQ_STAMP(7);
        NRQ_STOP(6)
        ph_store<WB, G, R.fast>(c, ostage_cur + (size_t)sidx * ostage_stride + subl * WB, vt, VNT);
      }
      __syncthreads();
      NRQ_STAMP(8);
#undef NRQ_STAMP
#undef NRQ_STOP
    }
    __syncthreads(); /* the gathered group is complete (and, for what a strip-less portion moved, visible) */
    qp = q;
    q = qn;
    buf ^= 1u;
  }
  /* the results of the last group */
  if (qp < nslots) {
    GroupDst<WB> gp;
    const uint32_t units_p = nrq_group_dst<WB>(qp, jobs, nblk, gpb, by_block, sub, T, nstrips, lsub, ybuf, ybuf_stride, gp) << lsub;
    pf_scatter_impl<WB, G, MPIPE, ALX>(gp, ostage0 + (size_t)(buf ^ 1u) * SPL * ostage_stride, ostage_stride, 0u, units_p, (tid) / G, (NT) / G, subl);
  }
}

enum {
#ifdef NRQ_PROF_INIT /* diagnostic build: the init phases one by one, in the slots big blocks leave empty (Wrun, Wmove, mh) */
  pl_tag_pl_init_a = 0,
  pl_tag_pl_init_b = 2,
  pl_tag_pl_scan_a = 4,
  pl_tag_pl_scan_b = 4,
  pl_tag_pl_scan_c = 4,
  pl_tag_pl_pcsc_fill = 11,
#else
  pl_tag_pl_init_a = 0,
  pl_tag_pl_init_b = 0,
  pl_tag_pl_scan_a = 0,
  pl_tag_pl_scan_b = 0,
  pl_tag_pl_scan_c = 0,
  pl_tag_pl_pcsc_fill = 0,
#endif
  pl_tag_pl_round_claim = 1,
  pl_tag_pl_round_drop = 3,
  pl_tag_pl_round_chain_end = 3,
  pl_tag_pl_inact_find = 5,
  pl_tag_pl_inact_find_b = 5,
  pl_tag_pl_inact_find_c = 5,
  pl_tag_pl_inact_apply_a = 6,
  pl_tag_pl_inact_apply_b = 6,
  pl_tag_pl_inact_next = 6,
  pl_tag_pl_event_scan = 5,
  pl_tag_pl_event_pick = 6,
  pl_tag_pl_event_drop = 6,
  pl_tag_pl_lev_0 = 7,
  pl_tag_pl_pivot_sort = 7,
  pl_tag_pl_lev_a = 7,
  pl_tag_pl_check_a = 7,
  pl_tag_pl_check_b = 7,
  pl_tag_pl_check_c = 7,
  pl_tag_pl_lev_b = 7,
  pl_tag_pl_w_init = 8,
  pl_tag_pl_w_init_b = 8,
  pl_tag_pl_cls_fetch = 8,
  pl_tag_pl_w_group = 8,
  pl_tag_pl_w_stage = 8,
  pl_tag_pl_wfast_spill = 4,
  pl_tag_pl_wfast_load = 4,
  pl_tag_pl_wfast_store = 4,
  pl_tag_pl_wfast_restore = 4,
  pl_tag_pl_low_a = 9,
  pl_tag_pl_low_b = 9,
  pl_tag_pl_low_c = 9,
  pl_tag_pl_ops_layout_a = 10,
  pl_tag_pl_ops_layout = 10,
  pl_tag_pl_ops_clear = 10,
  pl_tag_pl_ops_emit = 10,
  pl_tag_pl_ops_check_a = 10,
  pl_tag_pl_ops_check_b = 10,
  pl_tag_pl_ops_check_c = 10,
  pl_tag_pl_sh_restore = 0,
  pl_tag_pl_sh_save = 15,
  pl_tag_pl_mh_ext_clear = 15,
  pl_tag_pl_mh_fetch = 11,
  pl_tag_pl_mh_init = 11,
  pl_tag_pl_mh_load = 11,
  pl_tag_pl_mh_acc = 11,
  pl_tag_pl_gj_a = 12,
  pl_tag_pl_gjp_init = 12,
  pl_tag_pl_gjp_bid = 12,
  pl_tag_pl_gjp_step = 12,
  pl_tag_pl_gjp_wave = 12,
  pl_tag_pl_mhrev_load = 11,
  pl_tag_pl_mhrev_load_b = 11,
  pl_tag_pl_mhrev_store = 11,
  pl_tag_pl_mhrev_scatter = 11,
  pl_tag_pl_gjp_comb = 12,
  pl_tag_pl_gjp_stage = 12,
  pl_tag_pl_gjp_apply = 12,
  pl_tag_pl_gj_b = 12,
  pl_tag_pl_bin_a = 13,
  pl_tag_pl_bin_b = 13,
  pl_tag_pl_bin_c = 13,
  pl_tag_pl_dense_a = 14,
  pl_tag_pl_dense_b = 14,
  pl_tag_pl_dense_step_a = 14,
  pl_tag_pl_dense_step_b = 14,
  pl_tag_pl_dense_c = 14,
  pl_tag_pl_extra_a = 14,
  pl_tag_pl_extra_b = 14,
  pl_tag_pl_extra_c = 14,
  pl_tag_pl_extra_d = 14,
  pl_tag_pl_final_a = 15,
  pl_tag_pl_final_b = 15,
  pl_tag_pl_final_c = 15,
  pl_tag_pl_final_c2 = 15,
  pl_tag_pl_final_c3 = 15,
  pl_tag_pl_final_d = 15,
  pl_tag_pl_final_e = 15,
  pl_tag_pl_need_a = 15,
  pl_tag_pl_need_b = 15,
  pl_tag_pl_out_w = 15,
  pl_tag_pl_mark_failed = 15,
};

/* The symbolic stage of one decode block per workgroup (phases in planner_body.h, order in
 * planner_seq.h): reception pattern -> device plan + the block's solve job. */
/* PK = 1: the instance for blocks whose peeling state does not fit the LDS -- it carries the compact form of that state
 * (planner_body.h "compact peeling state"); the others are compiled without it */
/* (the instances for small blocks are built for five waves per SIMD, 96 registers: at the ~100 the compiler takes by itself a
 * SIMD holds four, and what bounds their planner is the number of blocks in flight per CU) */
template <int NT, int PK = 0>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(NT <= 256 ? 5 : 1)))
void nrq_plan_kernel(rq_params p, const uint8_t *__restrict__ kc,
                                                         const nrq_planjob *__restrict__ pjobs,
                                                         nrq_job *__restrict__ jobs_out, uint32_t nblk, uint32_t Mcap,
                                                         uint32_t npcap, uint32_t ucap, uint32_t lds_dyn_bytes,
                                                         unsigned long long *__restrict__ prof, uint32_t seg, uint32_t qcap,
                                                         uint32_t lowcap) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const uint32_t b = blockIdx.x, tid = threadIdx.x;
#define PL_SEG_ (PK == 0 ? 0u : seg) /* (blocks whose peeling state fits the LDS run in one part: launch_plan_kernel) */
  if (b >= nblk) return;
  /* the dynamic region comes first (LDS address 0: the W strip image is addressed like the solve kernel's), the
   * fixed workgroup state after it */
  uint8_t *dyn = smem;
  pl_shared *sh = reinterpret_cast<pl_shared *>(smem + lds_dyn_bytes);
  PlanCtx c;
  pl_ctx_setup(c, p, kc, pjobs[b], sh, dyn, lds_dyn_bytes, Mcap, npcap, ucap, jobs_out + b, qcap, lowcap, (uint32_t)NT);
  if (!PK) c.pk_cnt = c.pk_un = c.pk_pa = c.pk_vb = nullptr;
  if (PL_SEG_ == 3u) c.cls_glob = reinterpret_cast<uint32_t *>(c.work + c.wl.cls_g); /* (pl_lev_b zeroes the counters nrq_wentry_kernel counts into) */
  /* NRQ_PROF=1: thread 0 of block 0 accumulates shader clocks per phase family (index = PL_TAG) */
  unsigned long long t_prev = prof ? (unsigned long long)clock64() : 0ull;
#ifdef PL_STAMP
#define PL_ACC(tag) ((void)0) /* (the stamps alone: the per-phase clocks' stores to memory would be what the stamped loads wait for) */
#else
#define PL_ACC(tag) do { if (__builtin_expect(prof && b == 0 && tid == 0, 0)) { unsigned long long t_ = (unsigned long long)clock64(); \
                                                          prof[tag] += t_ - t_prev; prof[16 + tag] += 1; t_prev = t_; } } while (0)
#endif
#define PL_PHASE(fn) do { fn<PK>(c, tid, (uint32_t)NT); __syncthreads(); PL_ACC(pl_tag_##fn); } while (0)
#define PL_PHASE1(fn, a) do { fn<PK>(c, (a), tid, (uint32_t)NT); __syncthreads(); PL_ACC(pl_tag_##fn); } while (0)
#ifndef PL_CLAIM_FULL_BARRIER
#define PL_CLAIM_FULL_BARRIER 0
#endif
/* (the claim phase: with the peeling decisions in LDS its global stores -- pivot lists, the HBM copies of row / column
 * state -- are read after peeling only, or by nobody before the next full barrier: the barrier waits for the LDS alone, not
 * for the stores' way to memory and back, a trip per round) */
#ifndef PL_CLAIM_SKIP_IDLE
#define PL_CLAIM_SKIP_IDLE 1
#endif
#define PL_PHASE1_CLAIM(fn, a) do { if (!PL_CLAIM_SKIP_IDLE || (tid & ~63u) < nq_) fn<PK>(c, (a), tid, (uint32_t)NT); \
    if (!PL_CLAIM_FULL_BARRIER && (pl_peel_in_lds(c) || c.pk_cnt)) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); else __syncthreads(); \
    PL_ACC(pl_tag_##fn); } while (0)
#define PL_WFAST_RUN(wb) do { \
    if (tid < NRQ_ROW) { \
      const NRQ_GAS uint32_t *ops_ = gptr<uint32_t>(c.arena + c.sh->off_ops); \
      if ((wb) == 16u) fwd_rows<16>(ops_, pl_wfast_rows(c), tid); \
      else if ((wb) == 8u) fwd_rows<8>(ops_, pl_wfast_rows(c), tid); \
      else fwd_rows<4>(ops_, pl_wfast_rows(c), tid); \
    } \
    __syncthreads(); PL_ACC(2); } while (0)
#define PL_MHREV_RUN(wb) do { \
    if (tid < NRQ_ROW) { \
      const NRQ_GAS uint32_t *ops_ = gptr<uint32_t>(c.arena + c.sh->off_ops); \
      if ((wb) == 16u) rev_rows<16>(ops_, pl_wfast_rows(c), tid); \
      else if ((wb) == 8u) rev_rows<8>(ops_, pl_wfast_rows(c), tid); \
      else rev_rows<4>(ops_, pl_wfast_rows(c), tid); \
    } \
    __syncthreads(); PL_ACC(11); } while (0)
#define PL_SEG PL_SEG_ /* (blocks whose peeling state fits the LDS run in one part: launch_plan_kernel) */
#define PL_STEER_SYNC __syncthreads()
#define PL_NT_ ((uint32_t)NT)
#define PL_Z ((uint32_t)PK)
#ifdef PL_STAMP
  c.st_on = prof && b == 0 && tid == 0; c.st_prev = 0; c.st_blk = prof && b == 0;
  if (tid < 32) sh->st_acc[tid] = 0;
  __syncthreads();
#endif
  if (PL_SEG_ == 2u || PL_SEG_ == 4u) PL_PHASE(pl_sh_restore);
#include "planner_seq.h"
#ifdef PL_STAMP
  if (c.st_on) { for (int i_ = 0; i_ < 32; i_++) prof[32 + i_] = sh->st_acc[i_]; }
#endif
  if (PL_SEG_ == 1u || PL_SEG_ == 4u) PL_PHASE(pl_mh_ext_clear);
  if (PL_SEG_ == 1u || PL_SEG_ == 3u || PL_SEG_ == 4u) PL_PHASE(pl_sh_save);
#undef PL_SEG
#undef PL_SEG_
#undef PL_STEER_SYNC
#undef PL_NT_
#undef PL_PHASE
#undef PL_PHASE1
#undef PL_PHASE1_CLAIM
#undef PL_WFAST_RUN
#undef PL_MHREV_RUN
#undef PL_Z
#undef PL_ACC
}

/* Between parts 3 and 4 of a segmented planner run: the entry pass over the constraint matrix (pl_w_init: every entry either
 * toggles a bit of its row's W row or becomes a row op, counted in its level group and lane class and recorded) by `nparts`
 * workgroups per block.  One workgroup is bound by its CU's rate of scattered accesses there -- three per entry, 571 k entries at
 * K'=56403: 4.7 M clocks, a fifth of the plan.  Counters and the record counter are the workspace's for the duration. */
__global__ __launch_bounds__(1024) void nrq_wentry_kernel(rq_params p, const uint8_t *__restrict__ kc, const nrq_planjob *__restrict__ pjobs,
                                                          uint32_t Mcap, uint32_t npcap, uint32_t ucap, uint32_t lds_dyn_bytes) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const uint32_t part = blockIdx.x, nparts = gridDim.x, b = blockIdx.y, tid = threadIdx.x;
  pl_shared *sh = reinterpret_cast<pl_shared *>(smem);
  PlanCtx c;
  /* (lds_dyn_bytes: what the planner workgroup has -- pl_cls_place / pl_col_level decide by it; nothing of it is touched here) */
  pl_ctx_setup(c, p, kc, pjobs[b], sh, nullptr, 0u, Mcap, npcap, ucap, nullptr, PL_QCAP, PL_LOWCAP, PL_NT);
  c.aux_lds = reinterpret_cast<uint8_t *>(smem); c.aux_bytes = lds_dyn_bytes; c.dense_lds = c.aux_lds; c.dense_bytes = lds_dyn_bytes; /* (as the planner sees them: only their sizes matter) */
  pl_sh_restore<0>(c, tid, 1024u);
  __syncthreads();
  if (sh->status != 0 || sh->nV != 0) return;
  c.cls_glob = reinterpret_cast<uint32_t *>(c.work + c.wl.cls_g);
  c.nrec_ptr = &c.wentry[0];
  c.own_ptr = &c.wentry[3];
  pl_w_init_part<0>(c, part, nparts, tid, 1024u);
  __syncthreads();
  pl_wentry_report<0>(c, tid, 1024u);
}

/* Between the two parts of a segmented planner run (planner_seq.h): the HDPC fold over the pivots,
 * MhT[x] = G_U[:,x] ^ SUM_k W[k][x] * G[:, pivcol k], by `nparts` workgroups per block -- each folds every nparts-th tile
 * of 256 pivots into a private MhT in LDS (the planner's own phases pl_mh_load / pl_mh_acc) and XORs it into the copy in
 * the block's workspace.  One workgroup did this alone in 12 M clocks at K'=56403 (18 % of the plan). */
__global__ __launch_bounds__(1024) void nrq_mh_kernel(rq_params p, const uint8_t *__restrict__ kc, const nrq_planjob *__restrict__ pjobs,
                                                      uint32_t Mcap, uint32_t npcap, uint32_t ucap, uint32_t lds_dyn_bytes) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const uint32_t part = blockIdx.x, nparts = gridDim.x, b = blockIdx.y, tid = threadIdx.x;
  pl_shared *sh = reinterpret_cast<pl_shared *>(smem + lds_dyn_bytes);
  PlanCtx c;
  pl_ctx_setup(c, p, kc, pjobs[b], sh, smem, lds_dyn_bytes, Mcap, npcap, ucap, nullptr, PL_QCAP, PL_LOWCAP, PL_NT); /* (as the big planner workgroup) */
  pl_sh_restore<0>(c, tid, 1024u);
  __syncthreads();
  if (sh->status != 0 || sh->nV != 0) return;
  if (part == 0) pl_mh_init<0>(c, tid, 1024u); else pl_mh_part_zero<0>(c, tid, 1024u);
  __syncthreads();
  const uint32_t ntiles = (sh->npiv + PL_MH_TILE - 1u) / PL_MH_TILE;
  for (uint32_t tl = part; tl < ntiles; tl += nparts) {
    pl_mh_load<0>(c, tl, tid, 1024u);
    __syncthreads();
    pl_mh_acc<0>(c, tl, tid, 1024u);
    __syncthreads();
  }
  pl_mh_part_flush<0>(c, tid, 1024u);
}

/* Between the two parts of a segmented planner run: the W pass -- W = X^-1 * A_U and the leftover rows' reduced
 * coefficients are the op stream applied to the bit rows (planner_body.h "W pass, fast path").  Bit columns are
 * independent, so every workgroup takes a 2-byte strip of all W rows into LDS (slot image like the solve kernel's),
 * one wave runs the row pipeline over the stream (fwd_rows<2>), the strip goes back: wpr * 2 workgroups per block
 * instead of a level-by-level pass on the HBM rows by one (12 M clocks at K'=56403). */
__global__ __launch_bounds__(256) void nrq_wpass_kernel(rq_params p, const uint8_t *__restrict__ kc, const nrq_planjob *__restrict__ pjobs,
                                                        uint32_t Mcap, uint32_t npcap, uint32_t ucap) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[]; /* the strip image, from LDS address 0 */
  const uint32_t strip = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const nrq_planjob &j = pjobs[b];
  const nrq_kconst_hdr *kh = reinterpret_cast<const nrq_kconst_hdr *>(kc);
  const pl_work_layout wl = pl_work_plan(p.L, Mcap, npcap, ucap, kh->nnz + npcap * PL_PATCH_STRIDE);
  uint8_t *work = PL_HBM(uint8_t, j.work);
  const pl_shared *sv = reinterpret_cast<const pl_shared *>(work + wl.sh_save); /* part 1's state */
  if (sv->status != 0 || sv->nV != 0 || strip >= sv->wpr * 2u) return;
  const uint32_t M = sv->M, wpr = sv->wpr, nrows = sv->spare_base;
  uint16_t *rows16 = reinterpret_cast<uint16_t *>(work + wl.wrows); /* W row r, halfword h at [r * wpr * 2 + h] */
  uint16_t *img = reinterpret_cast<uint16_t *>(smem);
  for (uint32_t e = tid; e < M + NRQ_SCRATCH; e += 256u)
    img[e] = e >= NRQ_SCRATCH ? rows16[(size_t)(e - NRQ_SCRATCH) * wpr * 2u + strip] : (uint16_t)0;
  __syncthreads();
  if (tid < NRQ_ROW) fwd_rows<2>(gptr<uint32_t>(PL_HBM(uint8_t, j.arena) + sv->off_ops), nrows, tid);
  __syncthreads();
  for (uint32_t r = tid; r < M; r += 256u) rows16[(size_t)r * wpr * 2u + strip] = img[r + NRQ_SCRATCH];
}

/* After a segmented planner run: W transposed by word into the plan (pl_wt_fill), by many workgroups. */
__global__ __launch_bounds__(256) void nrq_wt_kernel(const nrq_planjob *__restrict__ pjobs, uint32_t L, uint32_t Mcap, uint32_t npcap,
                                                     uint32_t ucap, uint32_t nnzcap) {
  const nrq_planjob &j = pjobs[blockIdx.y];
  const pl_work_layout wl = pl_work_plan(L, Mcap, npcap, ucap, nnzcap);
  pl_wt_fill(PL_HBM(uint8_t, j.arena), reinterpret_cast<const uint32_t *>(PL_HBM(uint8_t, j.work) + wl.wrows),
             blockIdx.x * 256u + threadIdx.x, gridDim.x * 256u);
}

/* ---- split solve of big blocks (strips of 2 or 4 bytes) ----
 * An LDS-resident strip pays every per-row cost per WB bytes; at WB = 2 the back-substitution C(pivot k) = Y_k ^ W_k * C_u
 * alone is 55 % of a strip (K'=56403: 160 table lookups of TWO bytes per pivot).  It needs no slot image, only Y_k and
 * the u values C_u -- so for narrow strips the solve kernel stops after the dense stage and hands Y and C_u over as
 * full-width rows of a per-block work buffer, and this kernel finishes on 32-byte strips: 16-entry XOR tables over
 * groups of 4 inactive columns in LDS (80 KB at u <= 640), one pivot per thread, 32 bytes per lookup.
 * Rows [0, M) of the work buffer: slot image (Y at the pivots' slots), rows [M, M + u): C_u.  On return the buffer
 * holds the FINAL slot image: the pivot rows hold their intermediate symbols, the rows uslot[x] the inactive columns'. */
template <int SB>
__global__ __launch_bounds__(256) void nrq_backsub_kernel(const nrq_job *__restrict__ jobs, uint32_t T, uint8_t *__restrict__ ybuf,
                                                          size_t ybuf_stride, uint32_t nchunks) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const uint32_t tid = threadIdx.x, chunk = blockIdx.y, blk = blockIdx.z;
  SplitCtx<SB> c;
  if (!sp_ctx<SB>(c, reinterpret_cast<const uint8_t *>(jobs[blk].plan), gptr_w<uint8_t>((uint64_t)(uintptr_t)(ybuf + (size_t)blk * ybuf_stride)), T,
                  sp_strip_of<SB>(blockIdx.x, gridDim.x)))
    return;
  sp_tables<SB>(c, smem, tid);
  __syncthreads();
  sp_backsub<SB>(c, smem, chunk, nchunks, tid);
}

/* Results of the split solve, from the final slot image in the work buffer: workgroup (e, blk) writes one row (split_body.h) */
__global__ __launch_bounds__(256) void nrq_collect_kernel(const nrq_job *__restrict__ jobs, uint32_t T, const uint8_t *__restrict__ ybuf,
                                                          size_t ybuf_stride) {
  const uint32_t e = blockIdx.x, blk = blockIdx.y, tid = threadIdx.x;
  const nrq_job *j = jobs + blk;
  const uint8_t *plan = reinterpret_cast<const uint8_t *>(j->plan);
  const nrq_plan_hdr *h = reinterpret_cast<const nrq_plan_hdr *>(plan);
  if (h->status) return;
  if (e >= sc_elems(j, h)) return;
  __shared__ uint32_t rows[RQ_MAX_LT_COLS + 1];
  __shared__ uint32_t nrows;
  NRQ_GAS uint8_t *dst = sc_fetch(j, plan, e, T, tid, rows, &nrows);
  __syncthreads();
  sc_sum(gptr<uint8_t>((uint64_t)(uintptr_t)(ybuf + (size_t)blk * ybuf_stride)), dst, T, rows, nrows, tid);
}

/* Symbol ingestion on the device (nrq_scatter_symbols): symbol k of a contiguous packet buffer goes to the row its
 * tag names -- dst[k] is the row's device address (0 = drop).  One workgroup per symbol. */
/* Control data (job records, lists of lost / received ESIs: KBs) from page-locked host memory into a device buffer by a
 * KERNEL that reads the host memory directly: a hipMemcpyAsync of it is served by the host-to-device copy engine in the order
 * of submission, i.e. behind every bulk upload queued before it on ANY stream -- the planner of nanorq_repair_all then
 * started when the last packet of a deferred ingestion had landed (24 ms for 128 blocks of K=8192) instead of at once. */
__global__ __launch_bounds__(256) void nrq_ctl_copy_kernel(uint4 *__restrict__ dst, const uint4 *__restrict__ src, uint32_t n16) {
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n16; i += gridDim.x * 256u) dst[i] = src[i];
}

__global__ __launch_bounds__(128) void nrq_scatter_kernel(const uint8_t *__restrict__ blob, uint32_t T, const uint64_t *__restrict__ dst,
                                                          uint32_t n) {
  const uint32_t k = blockIdx.x;
  if (k >= n) return;
  uint8_t *d = reinterpret_cast<uint8_t *>(dst[k]);
  if (!d) return;
  const uint8_t *s = blob + (size_t)k * T;
  if ((T & 15u) == 0 && ((reinterpret_cast<uintptr_t>(s) | reinterpret_cast<uintptr_t>(d)) & 15u) == 0) {
    for (uint32_t off = threadIdx.x * 16u; off < T; off += 128u * 16u)
      *reinterpret_cast<uint4 *>(d + off) = *reinterpret_cast<const uint4 *>(s + off);
  } else {
    for (uint32_t off = threadIdx.x; off < T; off += 128u) d[off] = s[off];
  }
}

/* Rows by address pair: row k (T bytes) from src[k] to dst[k]; either may be page-locked HOST memory (the receiver's repaired
 * symbols leave for their places in the caller's output buffer: no staging buffer, no copy per row).  pairs = src0, dst0, src1, ... */
__global__ __launch_bounds__(128) void nrq_move_rows_kernel(const uint64_t *__restrict__ pairs, uint32_t T, uint32_t n) {
  const uint32_t k = blockIdx.x;
  if (k >= n) return;
  const uint8_t *s = reinterpret_cast<const uint8_t *>(pairs[2u * k]);
  uint8_t *d = reinterpret_cast<uint8_t *>(pairs[2u * k + 1u]);
  if (!s || !d) return;
  if ((T & 15u) == 0 && ((reinterpret_cast<uintptr_t>(s) | reinterpret_cast<uintptr_t>(d)) & 15u) == 0) {
    for (uint32_t off = threadIdx.x * 16u; off < T; off += 128u * 16u)
      *reinterpret_cast<uint4 *>(d + off) = *reinterpret_cast<const uint4 *>(s + off);
  } else {
    for (uint32_t off = threadIdx.x; off < T; off += 128u) d[off] = s[off];
  }
}

/* One workgroup per (symbol, block): out = XOR of the LT neighbours of `isi` among the L
 * intermediate symbols in HBM (coalesced 16-byte lanes along the symbol). */
__global__ __launch_bounds__(NRQ_GEN_WG) void nrq_gen_kernel(rq_params p, uint32_t T, const uint8_t *__restrict__ inter,
                                                         size_t inter_stride, const uint32_t *__restrict__ isis,
                                                         uint8_t *__restrict__ out, size_t out_stride) {
  __shared__ uint32_t cols[RQ_MAX_LT_COLS];
  __shared__ uint32_t ncols;
  const uint32_t q = blockIdx.x, b = blockIdx.y;
  if (threadIdx.x == 0) {
    uint32_t tmp[RQ_MAX_LT_COLS];
    uint32_t n = rq_lt_columns(&p, isis[q], tmp);
    for (uint32_t k = 0; k < n; k++) cols[k] = tmp[k];
    ncols = n;
  }
  __syncthreads();
  const uint8_t *C = inter + (size_t)b * inter_stride;
  uint8_t *dst = out + (size_t)b * out_stride + (size_t)q * T;
  const uint32_t n = ncols;
  const bool vec = ((T & 15u) == 0) && ((reinterpret_cast<uintptr_t>(C) & 15u) == 0) &&
                   ((reinterpret_cast<uintptr_t>(dst) & 15u) == 0);
  if (vec) {
    for (uint32_t off = threadIdx.x * 16u; off < T; off += NRQ_GEN_WG * 16u) {
      uint4 acc = make_uint4(0, 0, 0, 0);
      for (uint32_t k = 0; k < n; k++) {
        uint4 v = *reinterpret_cast<const uint4 *>(C + (size_t)cols[k] * T + off);
        acc.x ^= v.x; acc.y ^= v.y; acc.z ^= v.z; acc.w ^= v.w;
      }
      *reinterpret_cast<uint4 *>(dst + off) = acc;
    }
  } else {
    for (uint32_t off = threadIdx.x; off < T; off += NRQ_GEN_WG) {
      uint8_t acc = 0;
      for (uint32_t k = 0; k < n; k++) acc ^= C[(size_t)cols[k] * T + off];
      dst[off] = acc;
    }
  }
}

/* ============================================================================================
 * Host side
 * ========================================================================================== */
namespace {

double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

/* What the host side holds of the runtime is owned by the member that names it: move-only, released by its destructor.
 * ACQUISITION stays with the code that needs the thing (ensure_dev / ensure_pin, the checked create calls), and so does
 * every ORDERING question -- a destructor synchronises nothing (nrq_ctx_destroy does, before the members go). */
template <auto Release> struct Buf {
  uint8_t *p = nullptr;
  size_t cap = 0;
  Buf() = default;
  Buf(Buf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  Buf &operator=(Buf &&o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
  ~Buf() { if (p) (void)Release(p); }
};
using DevBuf = Buf<hipFree>;
using PinBuf = Buf<hipHostFree>;
using HostBuf = Buf<nrq_host_free>; /* what planner_host.cpp hands out (cap is not used) */

template <class H, auto Release> struct Handle {
  H h = nullptr;
  Handle() = default;
  Handle(Handle &&o) noexcept : h(o.h) { o.h = nullptr; }
  Handle &operator=(Handle &&o) noexcept { std::swap(h, o.h); return *this; }
  ~Handle() { if (h) (void)Release(h); }
  operator H() const { return h; }
};
using Event = Handle<hipEvent_t, hipEventDestroy>;
using Stream = Handle<hipStream_t, hipStreamDestroy>;
using TimingPool = std::vector<std::pair<Event, Event>>;

struct KConst {
  HostBuf host;
  DevBuf dev;
  uint32_t bytes = 0;
};

struct EncPlan {
  bool valid = false;     /* false after nrq_plan_cache_clear: rebuilt on next use, buffers are kept */
  PinBuf pin;             /* host planner: pinned image for the asynchronous upload; device planner: what comes back */
  uint8_t *dev = nullptr; /* the plan in use: plan arena and rowsrc (one of devbuf[]) */
  uint32_t plan_bytes = 0;
  uint32_t rowsrc_off = 0;
  nrq_plan_hdr hdr;
  std::vector<uint16_t> colslot; /* host copy, to translate LT neighbour lists into slots */
  double build_ms = 0;
  /* Two device buffers: a plan that is rebuilt ON THE DEVICE (big K', encplan_device_launch) goes to the buffer that is
   * not in use, on a stream of its own, while solves may still read the other one.  The host planner keeps to buffer 0
   * (its upload is ordered on the caller's stream). */
  DevBuf devbuf[2];
  Event used[2]; /* last solve launch that reads devbuf[i] */
  bool used_set[2] = {false, false};
  int cur = 0;
  bool pending = false;   /* a device build is in flight into devbuf[pend]; encplan_finish() completes it */
  int pend = 0;
  Event ready;
  uint32_t rb_bytes = 0;  /* device build: bytes of the arena's front (header .. colslot) read back */
  double t_launch = 0;
  bool dev_built = false; /* the plan in use came from the planner kernel (nrq_call_stats::encplan_device) */
};

inline size_t r16(size_t x) { return (x + 15) & ~(size_t)15; }

/* The symbol rows of a call, T bytes each, one run per block: base + b * stride, or an address per block (the _v entry points). */
struct Rows {
  const void *base = nullptr;
  size_t stride = 0;
  const uint64_t *vec = nullptr;
  explicit operator bool() const { return base || vec; }
  bool operator==(const Rows &o) const { return base == o.base && stride == o.stride && vec == o.vec; }
  uint64_t of(uint32_t b) const { return vec ? vec[b] : (uint64_t)(uintptr_t)((const uint8_t *)base + (size_t)b * stride); }
  /* every row starts 16-byte aligned */
  bool aligned(uint32_t nblk, uint32_t T) const {
    uintptr_t bits = vec ? 0 : (reinterpret_cast<uintptr_t>(base) | (uintptr_t)stride);
    for (uint32_t b = 0; vec && b < nblk; b++) bits |= (uintptr_t)vec[b];
    return ((bits | (uintptr_t)T) & 15u) == 0;
  }
};

/* What a decode call IS: the entry points build one and everything below them takes it.  Pointers, not copies -- the lists
 * are the caller's for the length of the call (PlanRun, which outlives its call, points them into vectors of its own). */
struct DecodeCall {
  uint32_t K = 0, Kp = 0, T = 0, nblk = 0;
  Rows src, rep, inter; /* source rows (recovered symbols go back into them), repair rows, intermediate symbols (optional) */
  const uint32_t *h_lost = nullptr, *h_nlost = nullptr; /* per block: lost_cap ESIs, ascending, and how many of them count */
  const uint32_t *h_rep_esi = nullptr, *h_nrep = nullptr; /* per block: rep_cap repair ESIs, how many to use ... */
  const uint32_t *h_avail = nullptr;                     /* ... and how many may be used if those leave the system rank deficient (optional) */
  uint32_t lost_cap = 0, rep_cap = 0;
  int *h_status = nullptr;    /* out, per block: 1 = decoded */
  uint32_t *h_used = nullptr; /* out, per block: repair symbols used (optional) */
  uint32_t chunk_blocks = 0;  /* nrq_decode_blocks_vc: blocks per solve launch (0: one launch for all) ... */
  void *const *chunk_done = nullptr, *const *chunk_up = nullptr; /* ... with an event to record behind / to wait for ahead of each */
  bool io_aligned = false; /* every symbol row of the call is 16-byte aligned: the solve's movers take their aligned-only form */
  uint64_t src_of(uint32_t b) const { return src.of(b); }
  uint64_t rep_of(uint32_t b) const { return rep.of(b); }
  uint64_t inter_of(uint32_t b) const { return inter ? inter.of(b) : 0; }
};

} // namespace

#define NRQ_PLAN_AHEAD_MAX 2u
struct PlanRun;
static void plan_ahead_drop(struct nrq_ctx *ctx);
struct nrq_ctx {
  int device = 0;
  long long fail_after = 0;      /* fault injection: checked runtime calls until the injected failure (0 = off) */
  bool fault_inject_armed = false; /* NANORQ_HIP_FAULT_INJECT=1 was in the environment when the context was created */
  long long faults_injected = 0;
  Tuning tune;
  int ncu = 256; /* compute units of the device */
  hipStream_t stream = nullptr;
  std::string err;
  std::map<uint32_t, KConst> kconst;    /* by K' */
  std::map<uint64_t, EncPlan> encplans; /* by (K', K) */
  DevBuf scratch[2];                    /* per-call device arrays (double-buffered across calls) */
  PinBuf staging[2];
  Event staged[2];
  int flip = 0;
  int threads = 0;
  nrq_call_stats stats;
  Event t0, t1;
  Event encplan_uploaded;
  uint32_t attr_widths = 0; /* bit WB: the attributes of the solve instances of that strip width are set */
  /* optional per-launch timing of the solve kernel (HIP events on the launch stream) */
  bool ktime_on = false;
  bool ktime_outer = false; /* the solve launches in flight are bracketed by their caller's pair of events */
  Event ktime_base; /* recorded by nrq_ktime_enable: origin of the launch intervals */
  TimingPool ktime_pool;
  size_t ktime_used = 0;
  TimingPool ptime_pool; /* same for the planner launches (all kernels of a planner run) */
  size_t ptime_used = 0;
  /* device planner */
  int planner = 1; /* 1 = device planner for decode (default), 0 = host planner */
  /* Planner runs may be issued AHEAD of their decode call (nrq_decode_plan_ahead), up to NRQ_PLAN_AHEAD_MAX of them: plan
   * arenas / job records come in three sets in turn (one being read by the solve in flight, two being written), the planner
   * workspace and the planner stream in two (two runs side by side: a planner workgroup is latency bound on ONE compute unit,
   * so two batches' planners on twice the compute units take the time of one), the input / header staging in four. */
  DevBuf plan_work[2], plan_arena[3], plan_jobs[3];
  uint32_t prun = 0; /* planner runs launched so far (chooses stream and workspace) */
  uint32_t ahead_hint = 0; /* most planner runs that were waiting at once since the last discard: sizes the CU reserve of big-block launches */
  DevBuf stage; /* solve kernel: staging buffers of the persistent workgroups */
  DevBuf ybuf;  /* split solve of narrow strips: per block, (M + u) full-width rows (slot image + inactive columns) */
  DevBuf jobs_b; /* pick_and_launch: the job records of a batch's second (narrower) block list, side by side */
  /* nrq_dev_alloc / nrq_dev_free: a caching pool (the object API allocates per call; hipMalloc / hipFree are
   * device-wide synchronisation points).  Freed blocks are reused for requests of up to 1.25x less; reuse is safe
   * because all work on a block is ordered on the context's streams and the object layer waits for its copy
   * streams before it frees. */
  std::multimap<size_t, void *> pool_free;
  std::map<void *, size_t> pool_size;
  size_t pool_cached = 0;
  Stream aux[3]; /* streams of the object layer: [0] host -> device copies, [1] device -> host copies,
                  * [2] kernels that sort uploaded packets into rows beside both */
  DevBuf scat_dev[2];
  PinBuf scat_pin[2];
  Event scat_ev[2];
  int scat_flip = 0;
  bool plan_attr = false;
  /* The planner kernel runs on a stream of its own: it depends on the reception pattern only, not on the symbols, so
   * it may run beside whatever the caller's stream is still doing (typically the encode solve launched just before).
   * `planned`: planner + header download done (the host waits for it, the solve launch on the caller's stream is
   * ordered behind it); `arena_free`: the solve that reads the plan arenas / job records has finished -- the next
   * planner launch overwrites them and waits for it. */
  Stream plan_stream;
  Stream plan_stream_b; /* the second planner stream (runs issued ahead alternate) */
  Event planned[3], arena_free[3];
  bool arena_busy[3] = {false, false, false};
  int aflip = 0;
  std::deque<struct PlanRun *> ahead; /* planner runs issued by nrq_decode_plan_ahead and not yet consumed, oldest first */
  Stream plan_stream2; /* encode plans built on the device (encplan_device_launch): beside both of the above */
  DevBuf encplan_work;                /* planner workspace of that build */
  DevBuf pscratch[4]; /* planner inputs: buffers of their own (the per-call arrays above belong to the caller's stream) */
  PinBuf pstaging[4];
  Event pstaged[4];
  int pflip = 0;
};

namespace {

#ifdef NRQ_NO_FAULT_INJECT
static inline bool nrq_inject(nrq_ctx *) { return false; } /* (a build without the hook: -DNRQ_NO_FAULT_INJECT) */
#else
static inline bool nrq_inject(nrq_ctx *ctx) {
  if (!ctx || ctx->fail_after <= 0) return false; /* (fail_after can only be set on a context created with NANORQ_HIP_FAULT_INJECT=1) */
  if (--ctx->fail_after > 0) return false;
  ctx->faults_injected++;
  return true;
}
#endif

int fail(nrq_ctx *ctx, int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (ctx) ctx->err = buf;
  return code;
}

/* Fault injection (nrq_ctx_set_option "fail_after" n): the n-th checked runtime call of the context from now on -- an
 * allocation, a copy, an event or stream operation, the error check behind a launch -- is not made and reports an error
 * instead, once.  The tests drive the error paths of the object layer with it (rollback of a packet batch, a failed chunk of
 * nanorq_repair_all, ...); nothing else sets it.  It is a TEST facility: the option exists only on a context created while
 * the environment holds NANORQ_HIP_FAULT_INJECT=1 (tests/conftest.py, tools/sanitize.sh set it) -- in any other process
 * "fail_after" is an unknown option, so no caller of the public nanorq_hip_option can make a runtime call fail -- and
 * -DNRQ_NO_FAULT_INJECT builds the library without the hook altogether. */
static inline bool nrq_inject(nrq_ctx *ctx);
#define HIPCHK(ctx, call)                                                                                   \
  do {                                                                                                      \
    hipError_t e_ = nrq_inject(ctx) ? hipErrorUnknown : (call);                                             \
    if (e_ != hipSuccess) return fail(ctx, -10, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_),      \
                                      __FILE__, __LINE__);                                                  \
  } while (0)

/* grow a buffer to `bytes` at least: the old one is freed, `want` bytes are allocated (0: the per-call arrays' margin, a
 * quarter and a page; the encode plans, one size per K', ask for an eighth) */
int ensure_dev(nrq_ctx *ctx, DevBuf &b, size_t bytes, size_t want = 0) {
  if (b.cap >= bytes) return 0;
  if (b.p) HIPCHK(ctx, hipFree(b.p));
  b.p = nullptr; b.cap = 0;
  if (!want) want = bytes + bytes / 4 + 4096;
  HIPCHK(ctx, hipMalloc((void **)&b.p, want));
  b.cap = want;
  return 0;
}
int ensure_pin(nrq_ctx *ctx, PinBuf &b, size_t bytes, size_t want = 0) {
  if (b.cap >= bytes) return 0;
  if (b.p) HIPCHK(ctx, hipHostFree(b.p));
  b.p = nullptr; b.cap = 0;
  if (!want) want = bytes + bytes / 4 + 4096;
  HIPCHK(ctx, hipHostMalloc((void **)&b.p, want, hipHostMallocDefault));
  b.cap = want;
  return 0;
}

/* The next pair of timing events of a pool (created on first use): the first is recorded on `st`, the second is handed back
 * for the caller to record behind its launches.  A caller that cannot do so gives the pair back (used--): the readers
 * (nrq_ktime_read, ...) take the elapsed time of every pair in use, and an event that was never recorded has none. */
int timing_pair(nrq_ctx *ctx, TimingPool &pool, size_t &used, hipStream_t st, hipEvent_t *ev_end) {
  if (used == pool.size()) {
    Event a, b;
    HIPCHK(ctx, hipEventCreate(&a.h));
    HIPCHK(ctx, hipEventCreate(&b.h));
    pool.emplace_back(std::move(a), std::move(b));
  }
  HIPCHK(ctx, hipEventRecord(pool[used].first, st));
  *ev_end = pool[used].second;
  used++;
  return 0;
}

/* parameters for a block of K symbols coded with the table row K' = Kp (0: the row RFC 6330 assigns to
 * K).  nanorq codes every block of an object with block 0's row (lib/nanorq.c:289, :372), so a short
 * last block can carry a K' larger than its own. */
int block_params(nrq_ctx *ctx, uint32_t K, uint32_t Kp, rq_params *p) {
  if (!rq_params_init(Kp ? Kp : K, p)) return fail(ctx, -1, "K=%u K'=%u out of range", K, Kp);
  if (K == 0 || K > p->Kp || (Kp && p->Kp != Kp)) return fail(ctx, -1, "K=%u does not fit table row K'=%u", K, Kp);
  p->K = K;
  return 0;
}

/* nrq_plan_kernel<NT, compact>: row i is the instance of nrq_plan_keys[i] (launch_shape.h) */
using plan_fn = void (*)(rq_params, const uint8_t *, const nrq_planjob *, nrq_job *, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t,
                         unsigned long long *, uint32_t, uint32_t, uint32_t);
#define NRQ_PLAN_ROW(NT, PK) &nrq_plan_kernel<(int)NT, PK>,
static const plan_fn plan_table[] = {NRQ_PLAN_INSTANCES(NRQ_PLAN_ROW)};
#undef NRQ_PLAN_ROW

/* the planner kernels may own the whole LDS of a CU (also the first touch of the code object: the runtime loads it here) */
static int plan_attr_once(nrq_ctx *ctx) {
  if (ctx->plan_attr) return 0;
  for (const plan_fn fn : plan_table)
    HIPCHK(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)NRQ_LDS_MAX));
  HIPCHK(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&nrq_mh_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)NRQ_LDS_MAX));
  HIPCHK(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&nrq_wpass_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)NRQ_LDS_MAX));
  ctx->plan_attr = true;
  return 0;
}

int get_kconst(nrq_ctx *ctx, uint32_t K, KConst **out) {
  rq_params p;
  if (!rq_params_init(K, &p)) return fail(ctx, -1, "K=%u out of range", K);
  auto it = ctx->kconst.find(p.Kp);
  if (it == ctx->kconst.end()) {
    KConst kc;
    if (nrq_host_kconst_build(K, &kc.host.p, &kc.bytes) != 0) return fail(ctx, -2, "kconst build failed");
    HIPCHK(ctx, hipMalloc((void **)&kc.dev.p, kc.bytes));
    kc.dev.cap = kc.bytes;
    HIPCHK(ctx, hipMemcpy(kc.dev.p, kc.host.p, kc.bytes, hipMemcpyHostToDevice));
    it = ctx->kconst.emplace(p.Kp, std::move(kc)).first;
  }
  *out = &it->second;
  return 0;
}

/* One planner run as plan_shape() decided it (the decode planner and the device build of encode plans): the instance once per
 * part, the helper kernels of a segmented run between and behind the parts (planner_seq.h). */
int launch_plan_kernel(nrq_ctx *ctx, hipStream_t ps, const PlanShape &s, const rq_params &p, const uint8_t *d_kc, const nrq_planjob *d_pj,
                       nrq_job *d_jobs, uint32_t nblk, uint32_t Mcap, uint32_t npcap, uint32_t ucap, unsigned long long *pprof,
                       uint32_t nnzcap) {
  { int rc_ = plan_attr_once(ctx); if (rc_) return rc_; }
  if (s.err) return fail(ctx, -2, "planner: a segmented run needs the instance for big blocks");
  const int inst = plan_key_index(s.wg_threads, s.compact);
  if (inst < 0) return fail(ctx, -2, "planner: no instance nrq_plan_kernel<%u, %u>", s.wg_threads, s.compact);
  for (uint32_t pi = 0; pi < s.nparts; pi++) {
    const uint32_t part = s.parts[pi];
    hipLaunchKernelGGL(plan_table[inst], dim3(nblk), dim3(s.wg_threads), s.dyn_bytes + s.sh_bytes, ps, p, d_kc, d_pj, d_jobs, nblk, Mcap,
                       npcap, ucap, s.dyn_bytes, pprof, part, s.qcap, s.lowcap);
    HIPCHK(ctx, hipGetLastError());
    if (part == 3u) {
      hipLaunchKernelGGL(nrq_wentry_kernel, dim3(s.wentry_wgs, nblk), dim3(1024), s.sh_bytes, ps, p, d_kc, d_pj, Mcap, npcap, ucap, s.dyn_bytes);
      HIPCHK(ctx, hipGetLastError());
    }
    if (part == 1u || part == 4u) {
      hipLaunchKernelGGL(nrq_wpass_kernel, dim3(s.wpass_wgs, nblk), dim3(256), s.wpass_lds, ps, p, d_kc, d_pj, Mcap, npcap, ucap);
      HIPCHK(ctx, hipGetLastError());
      hipLaunchKernelGGL(nrq_mh_kernel, dim3(s.mh_wgs, nblk), dim3(1024), s.mh_dyn + s.sh_bytes, ps, p, d_kc, d_pj, Mcap, npcap, ucap, s.mh_dyn);
      HIPCHK(ctx, hipGetLastError());
    }
  }
  if (s.segmented) {
    hipLaunchKernelGGL(nrq_wt_kernel, dim3(64, nblk), dim3(256), 0, ps, d_pj, p.L, Mcap, npcap, ucap, nnzcap);
    HIPCHK(ctx, hipGetLastError());
  }
  return 0;
}

/* host planner: build, stage in pinned memory, upload on the caller's stream (buffer 0) */
int encplan_host_build(nrq_ctx *ctx, const rq_params &p, uint32_t K, KConst *kc, EncPlan &ep) {
  double t0 = now_ms();
  std::vector<uint32_t> isis(p.Kp);
  for (uint32_t j = 0; j < p.Kp; j++) isis[j] = j;
  HostBuf arena;
  uint32_t bytes = 0;
  if (nrq_host_plan_build_forced(p.Kp, p.Kp, isis.data(), kc->host.p, &arena.p, &bytes, ctx->tune.plan_force_inact) != 0)
    return fail(ctx, -2, "encode plan build failed for K=%u", K);
  memcpy(&ep.hdr, arena.p, sizeof(ep.hdr));
  if (ep.hdr.status) return fail(ctx, -3, "encode matrix singular for K=%u (cannot happen)", K);
  ep.plan_bytes = bytes;
  ep.colslot.assign(reinterpret_cast<const uint16_t *>(arena.p + ep.hdr.off_colslot),
                    reinterpret_cast<const uint16_t *>(arena.p + ep.hdr.off_colslot) + p.L);
  ep.rowsrc_off = (uint32_t)r16(bytes);
  const size_t total = ep.rowsrc_off + (size_t)p.L * 4;
  /* device and pinned buffers survive a cache clear (same K => same size class); the upload is
   * asynchronous on the context's stream, so rebuilding a plan never waits for the GPU */
  int rc = ensure_dev(ctx, ep.devbuf[0], total, total + total / 8);
  if (rc) return rc;
  if (ep.pin.cap < total) {
    if ((rc = ensure_pin(ctx, ep.pin, total, total + total / 8))) return rc;
  } else {
    /* the previous upload from this pinned image must have been consumed */
    HIPCHK(ctx, hipEventSynchronize(ctx->encplan_uploaded));
  }
  memcpy(ep.pin.p, arena.p, bytes);
  uint32_t *rowsrc = reinterpret_cast<uint32_t *>(ep.pin.p + ep.rowsrc_off);
  for (uint32_t r = 0; r < p.L; r++) rowsrc[r] = NRQ_ROW_ZERO;
  for (uint32_t j = 0; j < K; j++) rowsrc[p.S + p.H + j] = j;
  HIPCHK(ctx, hipMemcpyAsync(ep.devbuf[0].p, ep.pin.p, total, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipEventRecord(ctx->encplan_uploaded, ctx->stream));
  ep.cur = 0;
  ep.dev = ep.devbuf[0].p;
  ep.valid = true;
  ep.pending = false;
  ep.dev_built = false;
  ep.build_ms = now_ms() - t0;
  return 0;
}

/* Device planner for an encode plan: the constraint matrix of an encode is that of a decode in which nothing was
 * replaced -- the planner kernel runs it as a job without missing symbols (nrq_planjob::mode).  Asynchronous, on
 * plan_stream2, into the buffer that is not in use; encplan_finish() waits for it and reads the header, the job
 * record and colslot[] back.  (reference: nanorq_precalculate, lib/nanorq.c:393-401) */
int encplan_device_launch(nrq_ctx *ctx, const rq_params &p, uint32_t K, KConst *kc, EncPlan &ep) {
  const nrq_kconst_hdr *kh = reinterpret_cast<const nrq_kconst_hdr *>(kc->host.p);
  uint32_t ucap = p.P + 768u;
  if (ucap > 1280u) ucap = 1280u;
  if (ucap < p.P + 32u) return 1; /* not for the device planner */
  const uint32_t Mcap = p.L + PL_EXTRA_ROWS + 8u, npcap = PL_EXTRA_ROWS + 8u;
  const pl_work_layout wl = pl_work_plan(p.L, Mcap, npcap, ucap, kh->nnz + npcap * PL_PATCH_STRIDE);
  const uint32_t arena_cap = pl_arena_bound(p.L, Mcap, ucap, kh->nnz + npcap * PL_PATCH_STRIDE, 8u);
  /* front of the arena that comes back: header, pivslot, pivcol, colslot (pl_ctx_setup's layout) */
  const uint32_t rb = (uint32_t)(r16(r16(r16(r16(sizeof(nrq_plan_hdr)) + p.L * 2u) + p.L * 2u) + p.L * 2u));
  const size_t off_pj = arena_cap, off_job = off_pj + r16(sizeof(nrq_planjob)), dev_total = off_job + r16(sizeof(nrq_job));
  const size_t pin_pj = 0, pin_rb = r16(sizeof(nrq_planjob)), pin_job = pin_rb + rb, pin_total = pin_job + r16(sizeof(nrq_job));
  const int buf = (ep.devbuf[ep.cur].p && (ep.valid || ep.used_set[ep.cur])) ? ep.cur ^ 1 : ep.cur;
  int rc;
  if ((rc = ensure_dev(ctx, ep.devbuf[buf], dev_total, dev_total + dev_total / 8))) return rc;
  if ((rc = ensure_dev(ctx, ctx->encplan_work, wl.total))) return rc;
  /* (the pinned image may still be the source of a host-built plan's asynchronous upload: encplan_host_build after a failed
   * device build -- wait for it before the job record is written over its first bytes) */
  HIPCHK(ctx, hipEventSynchronize(ctx->encplan_uploaded));
  if ((rc = ensure_pin(ctx, ep.pin, pin_total, pin_total + pin_total / 8))) return rc;
  if (!ep.ready) HIPCHK(ctx, hipEventCreateWithFlags(&ep.ready.h, hipEventDisableTiming));
  for (int i = 0; i < 2; i++)
    if (!ep.used[i]) HIPCHK(ctx, hipEventCreateWithFlags(&ep.used[i].h, hipEventDisableTiming));
  hipStream_t ps = ctx->plan_stream2;
  if (ep.used_set[buf]) HIPCHK(ctx, hipStreamWaitEvent(ps, ep.used[buf], 0));
  nrq_planjob *pj = reinterpret_cast<nrq_planjob *>(ep.pin.p + pin_pj);
  memset(pj, 0, sizeof(*pj));
  pj->work = (uint64_t)(uintptr_t)ctx->encplan_work.p;
  pj->arena = (uint64_t)(uintptr_t)ep.devbuf[buf].p;
  pj->arena_cap = arena_cap;
  const PlanShape shape = plan_shape(ctx->tune, ctx->ncu, p, 1u, Mcap, ucap);
  pj->mode = 1u | shape.mode;
  HIPCHK(ctx, hipMemcpyAsync(ep.devbuf[buf].p + off_pj, pj, sizeof(*pj), hipMemcpyHostToDevice, ps));
  rq_params pk = p;
  pk.K = K;
  if ((rc = launch_plan_kernel(ctx, ps, shape, pk, kc->dev.p, reinterpret_cast<const nrq_planjob *>(ep.devbuf[buf].p + off_pj),
                               reinterpret_cast<nrq_job *>(ep.devbuf[buf].p + off_job), 1u, Mcap, npcap, ucap, nullptr,
                               kh->nnz + npcap * PL_PATCH_STRIDE)))
    return rc;
  HIPCHK(ctx, hipMemcpyAsync(ep.pin.p + pin_rb, ep.devbuf[buf].p, rb, hipMemcpyDeviceToHost, ps));
  HIPCHK(ctx, hipMemcpyAsync(ep.pin.p + pin_job, ep.devbuf[buf].p + off_job, sizeof(nrq_job), hipMemcpyDeviceToHost, ps));
  HIPCHK(ctx, hipEventRecord(ep.ready, ps));
  ep.pending = true;
  ep.pend = buf;
  ep.rb_bytes = rb;
  ep.t_launch = now_ms();
  return 0;
}

int encplan_finish(nrq_ctx *ctx, const rq_params &p, uint32_t K, KConst *kc, EncPlan &ep) {
  if (!ep.pending) return 0;
  HIPCHK(ctx, hipEventSynchronize(ep.ready));
  ep.pending = false;
  const uint8_t *rbp = ep.pin.p + r16(sizeof(nrq_planjob));
  nrq_plan_hdr hd;
  memcpy(&hd, rbp, sizeof(hd));
  nrq_job jb;
  memcpy(&jb, rbp + ep.rb_bytes, sizeof(jb));
  if (hd.magic != NRQ_PLAN_MAGIC || hd.status != 0 || hd.off_colslot + p.L * 2u > ep.rb_bytes || jb.plan != (uint64_t)(uintptr_t)ep.devbuf[ep.pend].p) {
    /* a planner capacity was exceeded (or worse): the host planner takes over */
    if (ctx->tune.prof) fprintf(stderr, "[NRQ_PROF] encode plan K'=%u: device build failed (status %u, planner_body.h:%u), host planner\n",
                                p.Kp, hd.reserved[0], hd.fail_site);
    return encplan_host_build(ctx, p, K, kc, ep);
  }
  ep.hdr = hd;
  ep.colslot.assign(reinterpret_cast<const uint16_t *>(rbp + hd.off_colslot), reinterpret_cast<const uint16_t *>(rbp + hd.off_colslot) + p.L);
  ep.plan_bytes = hd.total_bytes;
  ep.rowsrc_off = (uint32_t)(jb.rowsrc - jb.plan);
  ep.cur = ep.pend;
  ep.dev = ep.devbuf[ep.cur].p;
  ep.valid = true;
  ep.dev_built = true;
  ep.build_ms = now_ms() - ep.t_launch;
  return 0;
}

/* The encode plan of (K', K): cached; built by the host planner (synchronously, uploaded on the caller's stream) or,
 * for big K', by the device planner -- asynchronously: with finish == false (nrq_precalculate) the call returns once
 * the build is enqueued, and the encode that needs the plan completes it. */
int get_encplan(nrq_ctx *ctx, uint32_t K, uint32_t Kp, EncPlan **out, bool finish = true) {
  rq_params p;
  int rc = block_params(ctx, K, Kp, &p);
  if (rc) return rc;
  const uint64_t key = ((uint64_t)p.Kp << 32) | K;
  auto it = ctx->encplans.find(key);
  if (it != ctx->encplans.end() && it->second.valid) { *out = &it->second; return 0; }
  KConst *kc;
  rc = get_kconst(ctx, p.Kp, &kc);
  if (rc) return rc;
  if (it == ctx->encplans.end()) it = ctx->encplans.emplace(key, EncPlan()).first;
  EncPlan &ep = it->second;
  *out = &ep;
  if (!ep.pending) {
    rc = 1;
    if (ctx->planner && p.L >= ctx->tune.encplan_dev_min_l) rc = encplan_device_launch(ctx, p, K, kc, ep);
    if (rc < 0) return rc;
    if (rc > 0) return encplan_host_build(ctx, p, K, kc, ep);
  }
  return finish ? encplan_finish(ctx, p, K, kc, ep) : 0;
}

/* nrq_solve_kernel<WB, NT, WV, G, AL>: row i is the instance of nrq_solve_keys[i] (launch_shape.h) */
using solve_fn = void (*)(const nrq_job *, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, const uint8_t *, uint8_t *, uint32_t,
                          uint32_t, unsigned long long *, uint8_t *, size_t);
#define NRQ_SOLVE_ROW(WB, NT, WV, G, AL) &nrq_solve_kernel<WB, NT, WV, G, AL>,
static const solve_fn solve_table[] = {NRQ_SOLVE_INSTANCES(NRQ_SOLVE_ROW)};
#undef NRQ_SOLVE_ROW

/* One solve launch: the blocks of d_jobs at strip width wb, as solve_shape() decides it -- buffers, attributes, the instance the
 * shape names, the two kernels that finish a split solve, the profile, the call's stats. */
static int launch_solve(nrq_ctx *ctx, const std::vector<const nrq_plan_hdr *> &hdrs, const nrq_job *d_jobs, uint32_t nblk,
                        uint32_t T, const uint8_t *d_kc, uint32_t max_out, uint32_t wb, uint32_t need, bool io_aligned) {
  SolveIn in;
  in.wb = wb; in.nblk = nblk; in.T = T; in.lds_bytes = need; in.max_out = max_out; in.io_aligned = io_aligned;
  in.hdrs = hdrs.data(); in.nhdrs = hdrs.size();
  for (const nrq_plan_hdr *h : hdrs) {
    if (h->status) continue;
    if (h->M > in.max_slots) in.max_slots = h->M;
    if (h->u > in.max_u) in.max_u = h->u;
    if (h->wpr > in.max_wpr) in.max_wpr = h->wpr;
  }
  const SolveShape s = solve_shape(ctx->tune, ctx->ncu, ctx->ahead_hint, in);
  if (s.err == SHAPE_GRID_TOO_LARGE) return fail(ctx, -4, "grid too large");
  /* (refused before anything is launched: it was reported behind the solve kernel's launch, whose work buffers nobody then read) */
  if (s.err == SHAPE_BACKSUB_TABLES) return fail(ctx, -5, "back-substitution tables do not fit the LDS (wpr=%u)", in.max_wpr);
  if (s.key.NT == 64 && ctx->tune.diag) fprintf(stderr, "[NRQ_DIAG] single-wave workgroups: %u bytes of LDS each, %u per CU\n", s.lds_bytes, s.occ);
  const int inst = solve_key_index(s.key);
  if (inst < 0)
    return fail(ctx, -2, "no solve kernel instance <%d, %d, %d, %d, %s>", s.key.WB, s.key.NT, s.key.WV, s.key.G, s.key.AL ? "true" : "false");
  {
    int rc_ = ensure_dev(ctx, ctx->stage, s.stage_bytes());
    if (rc_) return rc_;
  }
  uint8_t *ybuf = nullptr;
  if (s.split) {
    int rc_ = ensure_dev(ctx, ctx->ybuf, (size_t)nblk * s.ybuf_stride);
    if (rc_) return rc_;
    ybuf = ctx->ybuf.p;
  }
  if (!(ctx->attr_widths >> wb & 1u)) { /* first launch at this width: its instances (and the back-substitution kernels) may own the LDS */
    HIPCHK(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&nrq_backsub_kernel<32>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)NRQ_LDS_MAX));
    HIPCHK(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&nrq_backsub_kernel<16>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)NRQ_LDS_MAX));
    for (int i = 0; i < nrq_solve_nkeys; i++)
      if (nrq_solve_keys[i].WB == (int)wb)
        HIPCHK(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(solve_table[i]), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)NRQ_LDS_MAX));
    ctx->attr_widths |= 1u << wb;
  }
  hipEvent_t ev1 = nullptr;
  if (ctx->ktime_on && !ctx->ktime_outer) { /* (ktime_outer: pick_and_launch brackets the launches of both block lists itself) */
    int rc_ = timing_pair(ctx, ctx->ktime_pool, ctx->ktime_used, ctx->stream, &ev1);
    if (rc_) return rc_;
  }
  const uint32_t nprof = (s.grid + 15u) / 16u;
  DevBuf prof; /* NRQ_PROF=1: the workgroups' shader-clock marks, for the length of this launch */
  if (ctx->tune.prof) {
    HIPCHK(ctx, hipMalloc((void **)&prof.p, (size_t)nprof * 16 * 8));
    HIPCHK(ctx, hipMemsetAsync(prof.p, 0, (size_t)nprof * 16 * 8, ctx->stream));
  }
  unsigned long long *const d_prof = reinterpret_cast<unsigned long long *>(prof.p);
  hipLaunchKernelGGL(solve_table[inst], dim3(s.grid), dim3((uint32_t)s.key.NT), s.lds_bytes, ctx->stream, d_jobs, nblk, T, s.nstrips,
                     s.by_block ? 1u : 0u, s.nslots, s.lsub, d_kc, (uint8_t *)ctx->stage.p, s.stage_stride, s.ostage_stride, d_prof, ybuf,
                     s.ybuf_stride);
  if (s.key.G == 1) ctx->stats.movers_aligned = s.key.AL ? 1u : 0u; /* (a wide-strip launch leaves it as the call's reset gave it) */
  HIPCHK(ctx, hipGetLastError());
  if (s.split) {
    const dim3 bgrid(s.backsub_nsb, s.nchunks, nblk);
    if (s.backsub_strip == 32u)
      hipLaunchKernelGGL(nrq_backsub_kernel<32>, bgrid, dim3(256), s.backsub_tbl, ctx->stream, d_jobs, T, ybuf, s.ybuf_stride, s.nchunks);
    else
      hipLaunchKernelGGL(nrq_backsub_kernel<16>, bgrid, dim3(256), s.backsub_tbl, ctx->stream, d_jobs, T, ybuf, s.ybuf_stride, s.nchunks);
    HIPCHK(ctx, hipGetLastError());
    if (s.res_elems) {
      hipLaunchKernelGGL(nrq_collect_kernel, dim3(s.res_elems, nblk), dim3(256), 0, ctx->stream, d_jobs, T, (const uint8_t *)ybuf, s.ybuf_stride);
      HIPCHK(ctx, hipGetLastError());
    }
  }
  if (ev1) HIPCHK(ctx, hipEventRecord(ev1, ctx->stream));
  if (d_prof) {
    std::vector<unsigned long long> hp((size_t)nprof * 16);
    HIPCHK(ctx, hipMemcpyAsync(hp.data(), d_prof, hp.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    static const char *names[8] = {"load", "fwd", "hdpc", "bin", "dense", "tables", "backsub", "store"};
    double sum[8] = {0}, tot = 0;
    uint32_t cnt = 0;
    for (uint32_t w = 0; w < nprof; w++) {
      const unsigned long long *q = &hp[(size_t)w * 16];
      if (!q[8]) continue;
      for (int k = 0; k < 8; k++) sum[k] += (double)(q[k + 1] - q[k]);
      tot += (double)(q[8] - q[0]);
      cnt++;
    }
    fprintf(stderr, "[NRQ_PROF] WB=%u grid=%llu sampled=%u total=%.0f clk:", wb, (unsigned long long)s.grid, cnt,
            cnt ? tot / cnt : 0.0);
    for (int k = 0; k < 8; k++) fprintf(stderr, " %s=%.0f", names[k], cnt ? sum[k] / cnt : 0.0);
    /* slots 9..15: free-form marks a phase may leave through StripCtx::dbg (differences to the phase start) */
    double ext[7] = {0};
    for (uint32_t w = 0; w < nprof; w++) {
      const unsigned long long *q = &hp[(size_t)w * 16];
      if (!q[8]) continue;
      for (int k = 0; k < 7; k++) if (q[9 + k]) ext[k] += (double)(q[9 + k] - q[ctx->tune.prof_base]);
    }
    fprintf(stderr, " | marks since fwd end:");
    for (int k = 0; k < 7; k++) fprintf(stderr, " %.0f", cnt ? ext[k] / cnt : 0.0);
    fprintf(stderr, "\n");
  }
  ctx->stats.strip_bytes = wb * (uint32_t)s.key.G;
  ctx->stats.lds_bytes = s.lds_bytes;
  ctx->stats.grid = s.grid;
  ctx->stats.wg_threads = s.wg_threads;
  ctx->stats.strips_per_slot = 1u << s.lsub;
  ctx->stats.wg_waves_per_simd = s.wg_waves;
  ctx->stats.backsub_strip = s.backsub_strip;
  return 0;
}

/* The solve launch(es) of a batch: one, or -- when solve_lists() puts the blocks on two lists -- one per list, each list's job
 * records copied side by side first (a handful of small device-to-device copies, only when a batch splits).
 * blk_of_hdr: index in d_jobs of every header (nullptr: all blocks share one plan, nothing to split). */
int pick_and_launch(nrq_ctx *ctx, const std::vector<const nrq_plan_hdr *> &hdrs, const nrq_job *d_jobs, uint32_t nblk,
                    uint32_t T, const uint8_t *d_kc, uint32_t max_out, bool io_aligned, const std::vector<uint32_t> *blk_of_hdr = nullptr) {
  const SolveLists l = solve_lists(ctx->tune, hdrs.data(), hdrs.size(), blk_of_hdr != nullptr);
  if (l.err) return fail(ctx, -5, "block too large for the LDS-resident solver");
  if (!l.nsolv) return 0; /* nothing solvable in this batch */
  ctx->stats.strip_bytes_b = 0; ctx->stats.blocks_b = 0;
  if (!l.two) return launch_solve(ctx, hdrs, d_jobs, nblk, T, d_kc, max_out, l.wa, l.need_a, io_aligned);
  std::vector<const nrq_plan_hdr *> ha, hb;
  std::vector<uint32_t> ib;
  for (size_t i = 0; i < hdrs.size(); i++) {
    if (hdrs[i]->status) continue;
    if (l.on_b[i]) { hb.push_back(hdrs[i]); ib.push_back((*blk_of_hdr)[i]); }
    else ha.push_back(hdrs[i]);
  }
  /* both lists' job records side by side in scratch arrays: the second list's few records one by one (runs of neighbours in one
   * copy), the first list's as the stretches between them -- |B| + 1 copies of 80-byte records at most.  (A kernel-side rule --
   * "leave out the block whose image exceeds this launch's LDS" -- was tried first: the extra argument and header reads cost
   * the 256-thread variants, which live on 128 registers, 2.6 % at K=1000.) */
  int rc = ensure_dev(ctx, ctx->jobs_b, (ib.size() + (size_t)nblk) * sizeof(nrq_job));
  if (rc) return rc;
  nrq_job *jb = reinterpret_cast<nrq_job *>(ctx->jobs_b.p), *ja = jb + ib.size();
  for (size_t k = 0; k < ib.size(); k++) {
    size_t run = 1;
    while (k + run < ib.size() && ib[k + run] == ib[k] + run) run++;
    HIPCHK(ctx, hipMemcpyAsync(jb + k, d_jobs + ib[k], run * sizeof(nrq_job), hipMemcpyDeviceToDevice, ctx->stream));
    k += run - 1;
  }
  uint32_t na_blocks = 0; /* (every block of the batch that is not on the second list: the unsolvable ones stay, the kernel skips them) */
  for (size_t k = 0, from = 0; k <= ib.size(); k++) {
    const uint32_t to = k < ib.size() ? ib[k] : nblk;
    if (to > from) {
      HIPCHK(ctx, hipMemcpyAsync(ja + na_blocks, d_jobs + from, (to - from) * sizeof(nrq_job), hipMemcpyDeviceToDevice, ctx->stream));
      na_blocks += to - (uint32_t)from;
    }
    from = (size_t)to + 1u;
  }
  /* one pair of timing events around both launches (bench.py reads one interval per call) */
  hipEvent_t ev1 = nullptr;
  if (ctx->ktime_on) {
    if ((rc = timing_pair(ctx, ctx->ktime_pool, ctx->ktime_used, ctx->stream, &ev1))) return rc;
    ctx->ktime_outer = true;
  }
  rc = launch_solve(ctx, hb, jb, (uint32_t)ib.size(), T, d_kc, max_out, l.wb, l.need_b, io_aligned);
  const uint32_t sb_b = ctx->stats.strip_bytes;
  if (!rc) rc = launch_solve(ctx, ha, ja, na_blocks, T, d_kc, max_out, l.wa, l.need_a, io_aligned); /* (last: the call's stats describe the wide list) */
  ctx->ktime_outer = false;
  if (rc) {
    if (ev1) ctx->ktime_used--; /* (the pair's second event will not be recorded) */
    return rc;
  }
  if (ev1) HIPCHK(ctx, hipEventRecord(ev1, ctx->stream));
  ctx->stats.strip_bytes_b = sb_b;
  ctx->stats.blocks_b = (uint32_t)ib.size();
  return 0;
}

} // namespace

/* ============================================================================================
 * C ABI
 * ========================================================================================== */
extern "C" {

int nrq_params(uint32_t K, uint32_t out[10]) {
  rq_params p;
  if (!rq_params_init(K, &p)) return -1;
  out[0] = p.Kp; out[1] = p.J; out[2] = p.S; out[3] = p.H; out[4] = p.W;
  out[5] = p.L; out[6] = p.P; out[7] = p.P1; out[8] = p.U; out[9] = p.B;
  return 0;
}

int nrq_ctx_create(int device, void *stream, nrq_ctx **out) {
  if (!out) return -1;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return -20; /* no HIP device: fail loudly, no fallback */
  if (device < 0 || device >= ndev) return -21;
  if (hipSetDevice(device) != hipSuccess) return -22;
  nrq_ctx *ctx = new nrq_ctx();
  ctx->device = device;
  ctx->stream = (hipStream_t)stream;
  {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && n > 0) ctx->ncu = n;
  }
  ctx->tune.read();
  if (getenv("NRQ_HOST_PLANNER")) ctx->planner = 0;
  {
    const char *fi = getenv("NANORQ_HIP_FAULT_INJECT");
    ctx->fault_inject_armed = fi && *fi == '1';
  }
  memset(&ctx->stats, 0, sizeof(ctx->stats));
  bool ok = true;
  for (Stream *st : {&ctx->plan_stream, &ctx->plan_stream_b, &ctx->plan_stream2, &ctx->aux[0], &ctx->aux[1], &ctx->aux[2]})
    ok = ok && hipStreamCreateWithFlags(&st->h, hipStreamNonBlocking) == hipSuccess;
  for (Event *ev : {&ctx->scat_ev[0], &ctx->scat_ev[1], &ctx->planned[0], &ctx->planned[1], &ctx->planned[2], &ctx->arena_free[0],
                    &ctx->arena_free[1], &ctx->arena_free[2], &ctx->pstaged[0], &ctx->pstaged[1], &ctx->pstaged[2], &ctx->pstaged[3],
                    &ctx->encplan_uploaded, &ctx->staged[0], &ctx->staged[1]})
    ok = ok && hipEventCreateWithFlags(&ev->h, hipEventDisableTiming) == hipSuccess;
  ok = ok && hipEventCreate(&ctx->t0.h) == hipSuccess && hipEventCreate(&ctx->t1.h) == hipSuccess;
  if (!ok) {
    delete ctx; /* (what was created goes with it) */
    return -23;
  }
  *out = ctx;
  return 0;
}

void nrq_plan_cache_clear(nrq_ctx *ctx) {
  if (!ctx) return;
  for (auto &kv : ctx->encplans) kv.second.valid = false; /* buffers are reused by the rebuild */
}

static void encplans_release(nrq_ctx *ctx) {
  (void)hipStreamSynchronize(ctx->stream);
  if (ctx->plan_stream2) (void)hipStreamSynchronize(ctx->plan_stream2);
  ctx->encplans.clear();
}

void nrq_ctx_destroy(nrq_ctx *ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  /* ORDERING first, spelled out: the work on every stream is over and the planner runs issued ahead are through before
   * anything is released ... */
  (void)hipStreamSynchronize(ctx->stream);
  encplans_release(ctx);
  plan_ahead_drop(ctx);
  for (const Stream *st : {&ctx->plan_stream, &ctx->plan_stream_b, &ctx->plan_stream2, &ctx->aux[0], &ctx->aux[1], &ctx->aux[2]})
    if (*st) (void)hipStreamSynchronize(*st);
  /* ... then RELEASE: the pool's blocks (cached, or never given back by the caller) here, everything else by the members' destructors */
  for (auto &kv : ctx->pool_size) (void)hipFree(kv.first);
  delete ctx;
}

int nrq_ctx_set_stream(nrq_ctx *ctx, void *stream) {
  if (!ctx) return -1;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  ctx->stream = (hipStream_t)stream;
  return 0;
}

const char *nrq_ctx_error(nrq_ctx *ctx) { return ctx ? ctx->err.c_str() : "no context"; }

int nrq_ctx_sync(nrq_ctx *ctx) {
  if (!ctx) return -1;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return 0;
}

void nrq_ctx_last_stats(nrq_ctx *ctx, nrq_call_stats *out) {
  if (ctx && out) *out = ctx->stats;
}

int nrq_ctx_set_planner(nrq_ctx *ctx, int device_planner) {
  if (!ctx) return -1;
  ctx->planner = device_planner ? 1 : 0;
  return 0;
}

int nrq_ctx_set_option(nrq_ctx *ctx, const char *name, long long value) {
  if (!ctx || !name) return -1;
  const std::string n(name);
  if (ctx->tune.set(name, value)) return 0; /* (the knobs: NRQ_KNOBS, launch_shape.h) */
  if (n == "fail_after" && ctx->fault_inject_armed) ctx->fail_after = value > 0 ? value : 0;
  else if (n == "faults_injected") return (int)ctx->faults_injected; /* (read: injected failures so far) */
  else return fail(ctx, -1, "unknown option %s", name);
  return 0;
}

int nrq_ctx_set_threads(nrq_ctx *ctx, int n) {
  if (!ctx || n < 0) return -1;
  ctx->threads = n;
  return 0;
}

int nrq_precalculate(nrq_ctx *ctx, uint32_t K, uint32_t Kp) {
  if (!ctx) return -1;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  EncPlan *ep;
  return get_encplan(ctx, K, Kp, &ep, /*finish=*/false); /* a device build is only enqueued; the encode that needs it waits */
}

int nrq_warm(nrq_ctx *ctx, uint32_t K, uint32_t Kp, int encode_plan) {
  if (!ctx) return -1;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc = plan_attr_once(ctx);
  if (rc) return rc;
  rq_params p;
  if ((rc = block_params(ctx, K, Kp, &p))) return rc;
  KConst *kc;
  if ((rc = get_kconst(ctx, p.Kp, &kc))) return rc;
  if (encode_plan) {
    EncPlan *ep;
    rc = get_encplan(ctx, K, Kp, &ep, /*finish=*/encode_plan > 1); /* (2: also wait for a device build of the plan) */
  }
  return rc;
}

/* nrq_encode_blocks / nrq_encode_blocks_v: the intermediate symbols (optional) go to base + stride or to an address per block */
static int encode_blocks(nrq_ctx *ctx, uint32_t K, uint32_t Kp, uint32_t T, uint32_t nblk, const Rows &src, const Rows &inter, uint32_t nrep,
                         const uint32_t *h_esis, const Rows &rep) {
  if (!src || T == 0 || nblk == 0 || (nrep && (!h_esis || !rep))) return fail(ctx, -1, "bad arguments");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const double t_begin = now_ms();
  rq_params p;
  int rc = block_params(ctx, K, Kp, &p);
  if (rc) return rc;
  for (uint32_t q = 0; q < nrep; q++)
    if (h_esis[q] < K || h_esis[q] >= (1u << 24)) return fail(ctx, -1, "repair ESI %u out of range", h_esis[q]);
  const bool io_aligned = src.aligned(nblk, T) && (!nrep || rep.aligned(nblk, T)) && (!inter || inter.aligned(nblk, T));
  KConst *kc;
  rc = get_kconst(ctx, p.Kp, &kc);
  if (rc) return rc;
  const auto cached_it = ctx->encplans.find(((uint64_t)p.Kp << 32) | K);
  const bool cached = cached_it != ctx->encplans.end() && cached_it->second.valid;
  EncPlan *ep;
  rc = get_encplan(ctx, K, p.Kp, &ep);
  if (rc) return rc;
  memset(&ctx->stats, 0, sizeof(ctx->stats));
  ctx->stats.plan_ms = cached ? 0.0 : ep->build_ms;
  ctx->stats.plan_bytes = ep->plan_bytes;
  ctx->stats.xor_ops = (uint64_t)ep->hdr.n_xor_ops * nblk;
  ctx->stats.npiv = ep->hdr.npiv; ctx->stats.u = ep->hdr.u; ctx->stats.nlev = ep->hdr.nlev;
  ctx->stats.nfree = ep->hdr.nfree;
  ctx->stats.encplan_device = ep->dev_built ? 1u : 0u;

  /* per-call arrays: [jobs][isi->(cptr, cols, row)] */
  std::vector<uint32_t> isis(nrep), cptr, order;
  std::vector<uint16_t> cols;
  for (uint32_t q = 0; q < nrep; q++) isis[q] = h_esis[q] + (p.Kp - K);
  build_out_lists(p, ep->colslot.data(), nrep, isis.data(), cptr, cols, order);
  const size_t off_jobs = 0;
  const size_t off_cptr = r16(off_jobs + (size_t)nblk * sizeof(nrq_job));
  const size_t off_row = r16(off_cptr + (size_t)(nrep + 1) * 4);
  const size_t off_cols = r16(off_row + (size_t)(nrep ? nrep : 1) * 4);
  const size_t total = r16(off_cols + cols.size() * 2 + NRQ_STORE_SLACK); /* (ph_store reads a whole trip from a list's start) */
  const int f = ctx->flip;
  ctx->flip ^= 1;
  HIPCHK(ctx, hipEventSynchronize(ctx->staged[f]));
  if ((rc = ensure_pin(ctx, ctx->staging[f], total))) return rc;
  if ((rc = ensure_dev(ctx, ctx->scratch[f], total))) return rc;
  uint8_t *hs = ctx->staging[f].p, *ds = ctx->scratch[f].p;
  memcpy(hs + off_cptr, cptr.data(), (size_t)(nrep + 1) * 4);
  if (nrep) memcpy(hs + off_row, order.data(), (size_t)nrep * 4); /* (the list stored i-th is repair symbol order[i]'s: row order[i] of rep) */
  if (!cols.empty()) memcpy(hs + off_cols, cols.data(), cols.size() * 2);
  nrq_job *jobs = reinterpret_cast<nrq_job *>(hs + off_jobs);
  for (uint32_t b = 0; b < nblk; b++) {
    nrq_job &j = jobs[b];
    memset(&j, 0, sizeof(j));
    j.plan = (uint64_t)(uintptr_t)ep->dev;
    j.rowsrc = (uint64_t)(uintptr_t)(ep->dev + ep->rowsrc_off);
    j.src = src.of(b);
    j.rep = 0;
    j.inter = inter ? inter.of(b) : 0;
    j.out = nrep ? rep.of(b) : 0;
    j.out_cptr = (uint64_t)(uintptr_t)(ds + off_cptr);
    j.out_slots = (uint64_t)(uintptr_t)(ds + off_cols);
    j.out_row = (uint64_t)(uintptr_t)(ds + off_row);
    j.nout = nrep;
  }
  HIPCHK(ctx, hipMemcpyAsync(ds, hs, total, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipEventRecord(ctx->staged[f], ctx->stream));
  std::vector<const nrq_plan_hdr *> hdrs(1, &ep->hdr);
  rc = pick_and_launch(ctx, hdrs, reinterpret_cast<const nrq_job *>(ds + off_jobs), nblk, T, kc->dev.p, (inter ? p.L : 0u) + nrep, io_aligned);
  if (ep->used[ep->cur]) { /* (device-built plans: the next build may not overwrite this buffer before the launch is done) */
    HIPCHK(ctx, hipEventRecord(ep->used[ep->cur], ctx->stream));
    ep->used_set[ep->cur] = true;
  }
  ctx->stats.host_ms = now_ms() - t_begin;
  return rc;
}

int nrq_encode_blocks(nrq_ctx *ctx, uint32_t K, uint32_t Kp, uint32_t T, uint32_t nblk, const void *d_src, size_t src_stride,
                      void *d_inter, size_t inter_stride, uint32_t nrep, const uint32_t *h_esis, void *d_rep,
                      size_t rep_stride) {
  if (!ctx) return -1;
  return encode_blocks(ctx, K, Kp, T, nblk, Rows{d_src, src_stride}, Rows{d_inter, inter_stride}, nrep, h_esis, Rows{d_rep, rep_stride});
}

int nrq_encode_blocks_v(nrq_ctx *ctx, uint32_t K, uint32_t Kp, uint32_t T, uint32_t nblk, const void *d_src, size_t src_stride,
                        const uint64_t *d_inter_v) {
  if (!ctx || !d_inter_v) return -1;
  return encode_blocks(ctx, K, Kp, T, nblk, Rows{d_src, src_stride}, Rows{nullptr, 0, d_inter_v}, 0, nullptr, Rows{});
}

/* decode with the symbolic stage on the host; select: the blocks to do (nullptr: all of them), the others' status is left alone */
static int decode_host(nrq_ctx *ctx, const DecodeCall &c, const uint8_t *select) {
  const uint32_t K = c.K, T = c.T, nblk = c.nblk;
  const double t_begin = now_ms();
  rq_params p;
  int rc = block_params(ctx, K, c.Kp, &p);
  if (rc) return rc;
  KConst *kc;
  rc = get_kconst(ctx, p.Kp, &kc);
  if (rc) return rc;
  if (!select) memset(&ctx->stats, 0, sizeof(ctx->stats));

  struct Prep {
    HostBuf plan; /* the host-built plan arena */
    uint32_t plan_bytes = 0;
    std::vector<uint32_t> rowsrc, cptr, orow;
    std::vector<uint16_t> cols;
    std::vector<uint32_t> wout; /* the out view's image of these lists (plan.h off_wout): appended to the arena */
    int state = 0; /* 0 = nothing to do, 1 = solve, -1 = cannot */
    uint32_t used = 0;
    size_t off_plan = 0, off_wout = 0, off_rowsrc = 0, off_cptr = 0, off_row = 0, off_cols = 0;
  };
  std::vector<Prep> prep(nblk);
  const uint32_t pad = p.Kp - K;

  auto prepare = [&](uint32_t b) {
    Prep &pr = prep[b];
    const uint32_t nl = c.h_nlost[b], nr = c.h_nrep[b];
    if (select && !select[b]) { pr.state = 2; return; } /* not ours: leave its status alone */
    if (nl == 0) { pr.state = 0; return; }             /* nothing missing (nanorq.c:605-606) */
    if (nr < nl || nl > c.lost_cap || nr > c.rep_cap) { pr.state = -1; return; } /* nanorq.c:607-608 */
    const uint32_t *lost = c.h_lost + (size_t)b * c.lost_cap;
    const uint32_t *resi = c.h_rep_esi + (size_t)b * c.rep_cap;
    uint32_t avail = c.h_avail ? c.h_avail[b] : nr;
    if (avail < nr) avail = nr;
    if (avail > c.rep_cap) avail = c.rep_cap;
    /* use nr symbols; while the system is rank deficient and the caller holds more, take one more and re-plan */
    for (uint32_t use = nr;; use++) {
      const uint32_t overhead = use - nl;
      const uint32_t M = p.L + overhead;
      if (M > 65535u) { pr.state = -1; return; }
      std::vector<uint32_t> isis(p.Kp + overhead);
      for (uint32_t j = 0; j < p.Kp; j++) isis[j] = j;
      pr.rowsrc.assign(M, NRQ_ROW_ZERO);
      for (uint32_t j = 0; j < K; j++) pr.rowsrc[p.S + p.H + j] = j;
      for (uint32_t g = 0; g < nl; g++) {
        if (lost[g] >= K || (g && lost[g] <= lost[g - 1]) || resi[g] < K || resi[g] >= (1u << 24)) { pr.state = -1; return; }
        isis[lost[g]] = resi[g] + pad;
        pr.rowsrc[p.S + p.H + lost[g]] = NRQ_ROW_REP | g;
      }
      for (uint32_t e = 0; e < overhead; e++) {
        if (resi[nl + e] < K || resi[nl + e] >= (1u << 24)) { pr.state = -1; return; }
        isis[p.Kp + e] = resi[nl + e] + pad;
        pr.rowsrc[p.L + e] = NRQ_ROW_REP | (nl + e);
      }
      pr.plan = HostBuf();
      if (nrq_host_plan_build_forced(p.Kp, p.Kp + overhead, isis.data(), kc->host.p, &pr.plan.p, &pr.plan_bytes, ctx->tune.plan_force_inact) != 0) {
        pr.state = -1;
        return;
      }
      if (reinterpret_cast<const nrq_plan_hdr *>(pr.plan.p)->status == 0) { pr.used = use; break; }
      if (use + 1 > avail) { pr.state = -1; return; } /* rank(A) < L with everything the caller holds */
    }
    build_out_lists(p, reinterpret_cast<const uint16_t *>(pr.plan.p + reinterpret_cast<const nrq_plan_hdr *>(pr.plan.p)->off_colslot),
                    nl, lost, pr.cptr, pr.cols, pr.orow); /* ISI of a source symbol is its ESI */
    if (!c.inter) build_out_w(pr.plan.p, pr.cptr, pr.cols, pr.wout); /* (before orow[] names rows; needs cptr / cols only) */
    for (uint32_t &g : pr.orow) g = lost[g]; /* (the list stored i-th is that of missing symbol orow[i]: its row) */
    pr.state = 1;
  };

  const double t_plan0 = now_ms();
  {
    uint32_t nth = ctx->threads > 0 ? (uint32_t)ctx->threads : std::thread::hardware_concurrency();
    if (nth == 0) nth = 1;
    if (nth > nblk) nth = nblk;
    if ((uint64_t)K * nblk < 920u) nth = 1; /* (a few small blocks: ~0.4 us x K each -- less than starting and joining threads, ~200 us) */
    std::atomic<uint32_t> next(0);
    auto worker = [&]() {
      for (;;) {
        uint32_t b = next.fetch_add(1);
        if (b >= nblk) break;
        prepare(b);
      }
    };
    if (nth <= 1) worker();
    else {
      std::vector<std::thread> pool;
      for (uint32_t t = 0; t < nth; t++) pool.emplace_back(worker);
      for (auto &t : pool) t.join();
    }
  }
  ctx->stats.plan_ms += now_ms() - t_plan0;

  /* pack everything the kernel reads into one staging image */
  size_t off = r16((size_t)nblk * sizeof(nrq_job));
  /* a shared dummy header (status=1) for blocks that need no launch work */
  const size_t off_dummy = off;
  off = r16(off + sizeof(nrq_plan_hdr));
  uint32_t nsolve = 0;
  for (uint32_t b = 0; b < nblk; b++) {
    Prep &pr = prep[b];
    if (pr.state != 2) { c.h_status[b] = pr.state >= 0 ? 1 : 0; if (c.h_used) c.h_used[b] = pr.state == 1 ? pr.used : 0; }
    if (pr.state != 1) continue;
    nsolve++;
    pr.off_plan = off;   off = r16(off + pr.plan_bytes);
    pr.off_wout = off;   off = r16(off + pr.wout.size() * 4); /* (behind the arena: the job's out_w counts from the plan) */
    pr.off_rowsrc = off; off = r16(off + pr.rowsrc.size() * 4);
    pr.off_cptr = off;   off = r16(off + pr.cptr.size() * 4);
    pr.off_row = off;    off = r16(off + pr.orow.size() * 4);
    pr.off_cols = off;   off = r16(off + pr.cols.size() * 2 + NRQ_STORE_SLACK);
  }
  const size_t total = off;
  int result = 0;
  if (nsolve) {
    const int f = ctx->flip;
    ctx->flip ^= 1;
    HIPCHK(ctx, hipEventSynchronize(ctx->staged[f]));
    if ((rc = ensure_pin(ctx, ctx->staging[f], total))) return rc;
    if ((rc = ensure_dev(ctx, ctx->scratch[f], total))) return rc;
    uint8_t *hs = ctx->staging[f].p, *ds = ctx->scratch[f].p;
    nrq_plan_hdr dummy;
    memset(&dummy, 0, sizeof(dummy));
    dummy.magic = NRQ_PLAN_MAGIC;
    dummy.status = 1;
    memcpy(hs + off_dummy, &dummy, sizeof(dummy));
    nrq_job *jobs = reinterpret_cast<nrq_job *>(hs);
    std::vector<const nrq_plan_hdr *> hdrs;
    std::vector<uint32_t> hblk;
    for (uint32_t b = 0; b < nblk; b++) {
      Prep &pr = prep[b];
      nrq_job &j = jobs[b];
      memset(&j, 0, sizeof(j));
      if (pr.state != 1) { j.plan = (uint64_t)(uintptr_t)(ds + off_dummy); continue; }
      hblk.push_back(b);
      memcpy(hs + pr.off_plan, pr.plan.p, pr.plan_bytes);
      memcpy(hs + pr.off_rowsrc, pr.rowsrc.data(), pr.rowsrc.size() * 4);
      memcpy(hs + pr.off_cptr, pr.cptr.data(), pr.cptr.size() * 4);
      memcpy(hs + pr.off_row, pr.orow.data(), pr.orow.size() * 4);
      if (!pr.cols.empty()) memcpy(hs + pr.off_cols, pr.cols.data(), pr.cols.size() * 2);
      nrq_plan_hdr *h = reinterpret_cast<nrq_plan_hdr *>(hs + pr.off_plan);
      if (!pr.wout.empty()) { /* the lists' W' image: no back-substitution for this job (solve_body.h nrq_job_out_view) */
        memcpy(hs + pr.off_wout, pr.wout.data(), pr.wout.size() * 4);
        h->off_wout = j.out_w = (uint32_t)(pr.off_wout - pr.off_plan);
        h->out_n = (uint32_t)pr.orow.size(); h->out_pad = (h->out_n + 63u) & ~63u;
        h->total_bytes = h->off_wout + (uint32_t)pr.wout.size() * 4u;
        ctx->stats.out_view++;
        ctx->stats.plan_bytes += pr.wout.size() * 4;
      }
      hdrs.push_back(h);
      if (ctx->stats.npiv == 0) {
        ctx->stats.npiv = h->npiv; ctx->stats.u = h->u; ctx->stats.nlev = h->nlev; ctx->stats.nfree = h->nfree;
      }
      ctx->stats.xor_ops += h->n_xor_ops;
      ctx->stats.plan_bytes += pr.plan_bytes;
      j.plan = (uint64_t)(uintptr_t)(ds + pr.off_plan);
      j.rowsrc = (uint64_t)(uintptr_t)(ds + pr.off_rowsrc);
      j.src = c.src_of(b);
      j.rep = c.rep_of(b);
      j.inter = c.inter_of(b);
      j.out = j.src; /* recovered symbols go back into the block's own rows */
      j.out_cptr = (uint64_t)(uintptr_t)(ds + pr.off_cptr);
      j.out_slots = (uint64_t)(uintptr_t)(ds + pr.off_cols);
      j.out_row = (uint64_t)(uintptr_t)(ds + pr.off_row);
      j.nout = (uint32_t)pr.orow.size();
    }
    hipError_t e = hipMemcpyAsync(ds, hs, total, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipEventRecord(ctx->staged[f], ctx->stream);
    if (e != hipSuccess) result = fail(ctx, -10, "staging copy failed: %s", hipGetErrorString(e));
    else {
      uint32_t max_out = 0;
      for (uint32_t b = 0; b < nblk; b++)
        if (prep[b].state == 1 && prep[b].orow.size() > max_out) max_out = (uint32_t)prep[b].orow.size();
      result = pick_and_launch(ctx, hdrs, reinterpret_cast<const nrq_job *>(ds), nblk, T, kc->dev.p, (c.inter ? p.L : 0u) + max_out, c.io_aligned, &hblk);
    }
  }
  ctx->stats.host_ms += now_ms() - t_begin;
  return result;
}


/* One planner run of a batch of decode blocks: what its launch leaves for the half that waits for it and launches the solve.
 * Kept in the context between nrq_decode_plan_ahead and the decode call it was issued for (`call`: that call's record). */
struct PlanRun {
  rq_params p;
  KConst *kc = nullptr;
  uint32_t ucap = 0, Mcap = 0, npcap = 0, arena_cap = 0, max_nl = 0;
  size_t off_hdrs = 0;
  int f = 0, ab = 0; /* staging set, arena set */
  hipStream_t ps = nullptr;
  double t_begin = 0;
  /* the call this run was issued for: its lists point into the copies beside it */
  DecodeCall call;
  std::vector<uint32_t> lost, nlost, resi, nrep, avail;
  PlanShape shape; /* the planner form this run launched */
};

static void plan_ahead_drop(nrq_ctx *ctx) {
  for (PlanRun *r : ctx->ahead) {
    (void)hipEventSynchronize(ctx->planned[r->ab]); /* (its arena set is free again once it has run) */
    delete r;
  }
  ctx->ahead.clear();
  ctx->ahead_hint = 0;
}

/* first half: inputs down, planner kernels and the headers' way back enqueued on the planner stream */
static int plan_launch(nrq_ctx *ctx, PlanRun &r, const DecodeCall &c) {
  const uint32_t K = c.K, nblk = c.nblk;
  r.t_begin = now_ms();
  rq_params &p = r.p;
  int rc = block_params(ctx, K, c.Kp, &p);
  if (rc) return rc;
  KConst *kc;
  rc = get_kconst(ctx, p.Kp, &kc);
  if (rc) return rc;
  r.kc = kc;
  const nrq_kconst_hdr *kh = reinterpret_cast<const nrq_kconst_hdr *>(kc->host.p);
  uint32_t max_oh = 0, max_nrep = 0, max_nl = 0;
  for (uint32_t b = 0; b < nblk; b++) {
    const uint32_t nl = c.h_nlost[b];
    uint32_t nr = c.h_nrep[b];
    if (nl == 0 || nr < nl || nl > c.lost_cap || nr > c.rep_cap) continue;
    if (c.h_avail && c.h_avail[b] > nr) nr = c.h_avail[b] < c.rep_cap ? c.h_avail[b] : c.rep_cap; /* sizing: everything it may use */
    if (nr - nl > max_oh) max_oh = nr - nl;
    if (nr > max_nrep) max_nrep = nr;
    if (nl > max_nl) max_nl = nl;
  }
  r.max_nl = max_nl;
  uint32_t ucap = p.P + 768u;
  if (ucap > 1280u) ucap = 1280u; /* 40 words per W row at most */
  if (ctx->tune.plan_ucap && ctx->tune.plan_ucap < ucap) ucap = ctx->tune.plan_ucap;
  if (ucap < p.P + 32u) return fail(ctx, -5, "K'=%u has too many permanently inactive columns for the device planner", p.Kp);
  const uint32_t Mcap = p.L + max_oh + PL_EXTRA_ROWS + 8u, npcap = max_nrep + PL_EXTRA_ROWS + 8u;
  const pl_work_layout wl = pl_work_plan(p.L, Mcap, npcap, ucap, kh->nnz + npcap * PL_PATCH_STRIDE);
  const uint32_t arena_cap = pl_arena_bound(p.L, Mcap, ucap, kh->nnz + npcap * PL_PATCH_STRIDE, max_nl + 8u);
  r.ucap = ucap; r.Mcap = Mcap; r.npcap = npcap; r.arena_cap = arena_cap;
  r.shape = plan_shape(ctx->tune, ctx->ncu, p, nblk, Mcap, ucap);
  const int ab = ctx->aflip;
  ctx->aflip = (ctx->aflip + 1) % 3;
  r.ab = ab;
  const uint32_t run_no = ctx->prun++;
  DevBuf &work = ctx->plan_work[run_no & 1u];
  /* (growing a buffer frees the old one: nothing may still be running in it) */
  if (work.cap < (size_t)nblk * wl.total || ctx->plan_arena[ab].cap < (size_t)nblk * arena_cap ||
      ctx->plan_jobs[ab].cap < (size_t)nblk * sizeof(nrq_job)) {
    HIPCHK(ctx, hipStreamSynchronize(ctx->plan_stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->plan_stream_b));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  }
  if ((rc = ensure_dev(ctx, work, (size_t)nblk * wl.total))) return rc;
  if ((rc = ensure_dev(ctx, ctx->plan_arena[ab], (size_t)nblk * arena_cap))) return rc;
  if ((rc = ensure_dev(ctx, ctx->plan_jobs[ab], (size_t)nblk * sizeof(nrq_job)))) return rc;

  /* inputs of the planner: [planjobs][lost lists][repair ESI lists]; headers come back after them */
  const size_t off_pj = 0;
  const size_t off_lost = r16(off_pj + (size_t)nblk * sizeof(nrq_planjob));
  const size_t off_resi = r16(off_lost + (size_t)nblk * c.lost_cap * 4);
  const size_t in_bytes = r16(off_resi + (size_t)nblk * c.rep_cap * 4);
  const size_t off_hdrs = in_bytes;
  const size_t total = r16(off_hdrs + (size_t)nblk * sizeof(nrq_plan_hdr));
  r.off_hdrs = off_hdrs;
  /* everything up to the headers' way back runs on the planner stream (see nrq_ctx::plan_stream) */
  /* (only while the planner workgroups leave at least half of the CUs alone: with one per CU the two kernels just take
   * turns, and planner workgroups that get in first delay the persistent workgroups of the solve -- measured at 256
   * blocks of K=8192: encode solve 7.6 -> 10.4 ms, step +0.4 ms; at 64 blocks of K=20000 the overlap is worth 10 %) */
  hipStream_t ps = (ctx->tune.no_plan_stream || nblk * 2u > (uint32_t)ctx->ncu) ? ctx->stream
                   : (run_no & 1u)                                                 ? ctx->plan_stream_b
                                                                                   : ctx->plan_stream;
  r.ps = ps;
  const int f = ctx->pflip;
  ctx->pflip = (ctx->pflip + 1) & 3;
  r.f = f;
  HIPCHK(ctx, hipEventSynchronize(ctx->pstaged[f]));
  if ((rc = ensure_pin(ctx, ctx->pstaging[f], total))) return rc;
  if ((rc = ensure_dev(ctx, ctx->pscratch[f], total))) return rc; /* (inputs, and the headers side by side behind them) */
  uint8_t *hs = ctx->pstaging[f].p, *ds = ctx->pscratch[f].p;
  if (ctx->arena_busy[ab] && ps != ctx->stream) HIPCHK(ctx, hipStreamWaitEvent(ps, ctx->arena_free[ab], 0));
  memcpy(hs + off_lost, c.h_lost, (size_t)nblk * c.lost_cap * 4);
  memcpy(hs + off_resi, c.h_rep_esi, (size_t)nblk * c.rep_cap * 4);
  nrq_planjob *pj = reinterpret_cast<nrq_planjob *>(hs + off_pj);
  for (uint32_t b = 0; b < nblk; b++) {
    nrq_planjob &j = pj[b];
    memset(&j, 0, sizeof(j));
    const bool sane = c.h_nlost[b] <= c.lost_cap && c.h_nrep[b] <= c.rep_cap;
    j.lost = (uint64_t)(uintptr_t)(ds + off_lost + (size_t)b * c.lost_cap * 4);
    j.rep_esi = (uint64_t)(uintptr_t)(ds + off_resi + (size_t)b * c.rep_cap * 4);
    j.work = (uint64_t)(uintptr_t)(work.p + (size_t)b * wl.total);
    j.arena = (uint64_t)(uintptr_t)(ctx->plan_arena[ab].p + (size_t)b * arena_cap);
    j.hdr_out = (uint64_t)(uintptr_t)(ds + off_hdrs + (size_t)b * sizeof(nrq_plan_hdr));
    j.src = c.src_of(b);
    j.rep = c.rep_of(b);
    j.inter = c.inter_of(b);
    j.nlost = sane ? c.h_nlost[b] : 0;
    j.nrep = sane ? c.h_nrep[b] : 0;
    j.nrep_avail = j.nrep;
    if (sane && c.h_avail && c.h_avail[b] > j.nrep) j.nrep_avail = c.h_avail[b] < c.rep_cap ? c.h_avail[b] : c.rep_cap;
    j.arena_cap = arena_cap;
    j.mode = r.shape.mode;
  }
  { /* (in_bytes is a multiple of 16; both buffers are 16-byte aligned allocations) */
    const uint32_t n16 = (uint32_t)(in_bytes / 16u);
    uint32_t g = (n16 + 255u) / 256u;
    if (g > 64u) g = 64u;
    hipLaunchKernelGGL(nrq_ctl_copy_kernel, dim3(g ? g : 1u), dim3(256), 0, ps, reinterpret_cast<uint4 *>(ds), reinterpret_cast<const uint4 *>(hs), n16);
    HIPCHK(ctx, hipGetLastError());
  }
  DevBuf prof; /* NRQ_PROF=1: the planner's shader-clock marks, for the length of this run's launch */
  if (ctx->tune.prof) {
    HIPCHK(ctx, hipMalloc((void **)&prof.p, 64 * 8));
    HIPCHK(ctx, hipMemsetAsync(prof.p, 0, 64 * 8, ps));
  }
  unsigned long long *const pprof = reinterpret_cast<unsigned long long *>(prof.p);
  hipEvent_t pe1 = nullptr;
  if (ctx->ktime_on && (rc = timing_pair(ctx, ctx->ptime_pool, ctx->ptime_used, ps, &pe1))) return rc;
  if ((rc = launch_plan_kernel(ctx, ps, r.shape, p, kc->dev.p, reinterpret_cast<const nrq_planjob *>(ds + off_pj),
                               reinterpret_cast<nrq_job *>(ctx->plan_jobs[ab].p), nblk, Mcap, npcap, ucap, pprof,
                               kh->nnz + npcap * PL_PATCH_STRIDE)))
    return rc;
  if (pe1) HIPCHK(ctx, hipEventRecord(pe1, ps));
  if (pprof) {
    unsigned long long hp[64];
    HIPCHK(ctx, hipMemcpyAsync(hp, pprof, sizeof(hp), hipMemcpyDeviceToHost, ps));
    HIPCHK(ctx, hipStreamSynchronize(ps));
    static const char *nm[16] = {"init", "claim", "Wrun", "drop", "Wmove", "ifind", "iapply", "lev", "W", "low", "ops", "mh",
                                 "gj", "bin", "dense", "final"};
    unsigned long long tot = 0;
    for (int k = 0; k < 16; k++) tot += hp[k];
    fprintf(stderr, "[NRQ_PROF] planner nblk=%u total=%llu clk:", nblk, tot);
    for (int k = 0; k < 16; k++) fprintf(stderr, " %s=%llu(%llu)", nm[k], hp[k], hp[16 + k]);
    fprintf(stderr, "\n");
#ifdef PL_STAMP
    fprintf(stderr, "[NRQ_PROF] round stamps (clocks up to point i, summed over the rounds):");
    for (int k = 0; k < 24; k++) fprintf(stderr, " %d:%llu", k, hp[32 + k]);
    fprintf(stderr, "\n[NRQ_PROF] chained peel: entries %llu, group clocks busy %llu (waiting for the rows %llu), claims %llu, phases %llu clocks %llu; flags trip %llu, subtraction trip %llu, claims %llu\n",
            hp[56], hp[57], hp[58], hp[59], hp[61], hp[60], hp[62], hp[63], hp[54]);
#endif
  }
  HIPCHK(ctx, hipMemcpyAsync(hs + off_hdrs, ds + off_hdrs, (size_t)nblk * sizeof(nrq_plan_hdr), hipMemcpyDeviceToHost, ps)); /* (pl_final_d's second copies) */
  HIPCHK(ctx, hipEventRecord(ctx->pstaged[f], ps));
  HIPCHK(ctx, hipEventRecord(ctx->planned[ab], ps));
  return 0;
}

/* was this run issued for exactly this call? */
static bool plan_run_matches(const PlanRun &r, const DecodeCall &c) {
  const DecodeCall &a = r.call;
  if (c.src.vec || c.rep.vec || c.chunk_blocks) return false; /* (runs are issued for base + stride calls that solve in one launch) */
  if (a.K != c.K || a.Kp != c.Kp || a.T != c.T || a.nblk != c.nblk || a.lost_cap != c.lost_cap || a.rep_cap != c.rep_cap) return false;
  if (!(a.src == c.src) || !(a.rep == c.rep) || !(a.inter == c.inter) || (a.h_avail != nullptr) != (c.h_avail != nullptr)) return false;
  return memcmp(a.h_nlost, c.h_nlost, (size_t)c.nblk * 4) == 0 && memcmp(a.h_nrep, c.h_nrep, (size_t)c.nblk * 4) == 0 &&
         (!c.h_avail || memcmp(a.h_avail, c.h_avail, (size_t)c.nblk * 4) == 0) &&
         memcmp(a.h_lost, c.h_lost, (size_t)c.nblk * c.lost_cap * 4) == 0 &&
         memcmp(a.h_rep_esi, c.h_rep_esi, (size_t)c.nblk * c.rep_cap * 4) == 0;
}

/* decode with the symbolic stage on the GPU: one planner workgroup per block, then the solve */
/* (fallback: set for the blocks that exceeded a planner capacity; the return value 1 says that there are some) */
static int decode_device(nrq_ctx *ctx, const DecodeCall &c, std::vector<uint8_t> *fallback) {
  const uint32_t K = c.K, T = c.T, nblk = c.nblk;
  const double t_begin = now_ms();
  memset(&ctx->stats, 0, sizeof(ctx->stats));
  ctx->stats.planner = 1;
  PlanRun local, *run = &local;
  bool ahead = false;
  while (!ctx->ahead.empty()) {
    PlanRun *f = ctx->ahead.front();
    ctx->ahead.pop_front();
    if (plan_run_matches(*f, c)) {
      run = f; /* the planner run of this very call is already on its way (or done) */
      ahead = true;
      break;
    }
    /* runs are consumed in the order they were issued: one this call was not issued for is over (its arena set is free again
     * once it has run); a later one may still be this call's (a caller that issued a run per reception state) */
    (void)hipEventSynchronize(ctx->planned[f->ab]);
    delete f;
    if (ctx->ahead.empty()) ctx->ahead_hint = 0;
  }
  struct Owner { PlanRun *r; ~Owner() { delete r; } } owner{ahead ? run : nullptr};
  if (!ahead) {
    const int rc0 = plan_launch(ctx, *run, c);
    if (rc0) return rc0;
  }
  const rq_params &p = run->p;
  KConst *kc = run->kc;
  const int ab = run->ab;
  const uint32_t max_nl = run->max_nl;
  hipStream_t ps = run->ps;
  uint8_t *hs = ctx->pstaging[run->f].p;
  const size_t off_hdrs = run->off_hdrs;
  HIPCHK(ctx, hipEventSynchronize(ctx->planned[ab]));
  ctx->stats.plan_ms = now_ms() - t_begin;
  ctx->stats.plan_ahead = ahead ? 1 : 0;
  ctx->stats.plan_wg_threads = run->shape.wg_threads;
  ctx->stats.plan_compact_state = run->shape.compact;
  ctx->stats.plan_segmented = run->shape.segmented;
  const nrq_plan_hdr *hd = reinterpret_cast<const nrq_plan_hdr *>(hs + off_hdrs);
  std::vector<const nrq_plan_hdr *> hdrs;
  std::vector<uint32_t> hblk; /* block of every header in hdrs (pick_and_launch: the batch's two block lists) */
  bool need_fallback = false;
  for (uint32_t b = 0; b < nblk; b++) {
    if (c.h_used) c.h_used[b] = 0;
    if (c.h_nlost[b] == 0) { c.h_status[b] = 1; continue; } /* nothing missing (nanorq.c:605-606) */
    if (hd[b].magic != NRQ_PLAN_MAGIC) return fail(ctx, -11, "device planner produced no header for block %u", b);
    if (hd[b].status == 0) {
      c.h_status[b] = 1;
      if (c.h_used) c.h_used[b] = c.h_nrep[b] + hd[b].reserved[1];
      hdrs.push_back(&hd[b]);
      hblk.push_back(b);
      if (ctx->stats.npiv == 0) {
        ctx->stats.npiv = hd[b].npiv; ctx->stats.u = hd[b].u; ctx->stats.nlev = hd[b].nlev; ctx->stats.nfree = hd[b].nfree;
      }
      ctx->stats.xor_ops += hd[b].n_xor_ops;
      ctx->stats.plan_bytes += hd[b].total_bytes;
      if (hd[b].scan_lists) ctx->stats.plan_scan_lists++; /* (pl_final_d: the lists in row order, offsets from the scan) */
      if (hd[b].off_wout) ctx->stats.out_view++; /* (pl_final_d gave the job the same offset as out_w) */
      else if (hd[b].off_needslot && !c.inter) { /* (the back-substitution of this job takes the needed-pivot view: solve_body.h) */
        if (ctx->stats.need_view++ == 0) ctx->stats.nneed = hd[b].nneed;
      }
    } else if (hd[b].reserved[0] == PL_FAIL_CAPACITY) {
      if (ctx->tune.prof || ctx->tune.diag) fprintf(stderr, "[NRQ_PROF] block %u: device planner capacity exceeded at planner_body.h:%u (npiv %u u %u nlev %u nrows %u M %u nlost %u)\n", b, hd[b].fail_site, hd[b].npiv, hd[b].u, hd[b].nlev, hd[b].nrows, hd[b].M, c.h_nlost[b]);
      (*fallback)[b] = 1;
      need_fallback = true;
      c.h_status[b] = 0;
    } else {
      if (ctx->tune.prof || ctx->tune.diag)
        fprintf(stderr, "[NRQ_PROF] block %u: not decodable: status %u reason %u site %u npiv %u u %u nlev %u nlow %u r2 %u nfree %u taken %u\n", b, hd[b].status,
                hd[b].reserved[0], hd[b].fail_site, hd[b].npiv, hd[b].u, hd[b].nlev, hd[b].nlow, hd[b].r2, hd[b].nfree, hd[b].reserved[1]);
      c.h_status[b] = 0;
    }
  }
  int result = 0;
  if (c.chunk_blocks) {
    /* one planner run, the solve chunk by chunk (nrq_decode_blocks_vc): an event per chunk for the caller's copy streams */
    if (ps != ctx->stream) HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->planned[ab], 0));
    const uint32_t cb = c.chunk_blocks;
    for (uint32_t c0 = 0, ci = 0; c0 < nblk && !result; c0 += cb, ci++) {
      const uint32_t m = nblk - c0 < cb ? nblk - c0 : cb;
      std::vector<const nrq_plan_hdr *> hc;
      std::vector<uint32_t> hcb;
      for (uint32_t b = c0; b < c0 + m; b++)
        if (c.h_nlost[b] != 0 && hd[b].magic == NRQ_PLAN_MAGIC && hd[b].status == 0) { hc.push_back(&hd[b]); hcb.push_back(b - c0); }
      if (c.chunk_up && c.chunk_up[ci]) HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, (hipEvent_t)c.chunk_up[ci], 0));
      if (!hc.empty())
        result = pick_and_launch(ctx, hc, reinterpret_cast<const nrq_job *>(ctx->plan_jobs[ab].p) + c0, m, T, kc->dev.p, (c.inter ? p.L : 0u) + max_nl, c.io_aligned, &hcb);
      if (c.chunk_done && c.chunk_done[ci]) HIPCHK(ctx, hipEventRecord((hipEvent_t)c.chunk_done[ci], ctx->stream));
    }
    HIPCHK(ctx, hipEventRecord(ctx->arena_free[ab], ctx->stream));
    ctx->arena_busy[ab] = true;
  } else if (!hdrs.empty()) {
    if (ps != ctx->stream) HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->planned[ab], 0));
    result = pick_and_launch(ctx, hdrs, reinterpret_cast<const nrq_job *>(ctx->plan_jobs[ab].p), nblk, T, kc->dev.p,
                             (c.inter ? p.L : 0u) + max_nl, c.io_aligned, &hblk);
    /* the launch reads the plan arenas and job records: a later planner run may not overwrite this set before it is done */
    HIPCHK(ctx, hipEventRecord(ctx->arena_free[ab], ctx->stream));
    ctx->arena_busy[ab] = true;
  }
  ctx->stats.host_ms = now_ms() - t_begin;
  if (result) return result;
  return need_fallback ? 1 : 0;
}

/* Issue the planner run of a decode call AHEAD of the call: the symbolic stage needs the reception pattern only, not the
 * symbols -- a receiver that knows which symbols of a batch of blocks it holds (or a pipeline that decodes batch after batch)
 * can have the plan built while earlier work is still being solved; the nrq_decode_blocks / _lazy call with the same arguments
 * then only waits for it.  A call with other arguments discards it. */
int nrq_decode_plan_ahead(nrq_ctx *ctx, uint32_t K, uint32_t Kp, uint32_t T, uint32_t nblk, void *d_src, size_t src_stride,
                          const uint32_t *h_lost, const uint32_t *h_nlost, uint32_t lost_cap, const uint32_t *h_rep_esi,
                          const uint32_t *h_nrep, const uint32_t *h_nrep_avail, uint32_t rep_cap, const void *d_rep, size_t rep_stride,
                          void *d_inter, size_t inter_stride) {
  if (!ctx) return -1;
  if (!d_src || T == 0 || nblk == 0 || !h_nlost || !h_nrep || !h_lost || !h_rep_esi) return fail(ctx, -1, "bad arguments");
  if (!ctx->planner) return 0; /* host planner: nothing to issue ahead */
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (ctx->ahead.size() >= NRQ_PLAN_AHEAD_MAX) return fail(ctx, -6, "nrq_decode_plan_ahead: %u runs are already waiting for their decode calls", (unsigned)NRQ_PLAN_AHEAD_MAX);
  DecodeCall c;
  c.K = K; c.Kp = Kp; c.T = T; c.nblk = nblk;
  c.src = {d_src, src_stride}; c.rep = {d_rep, rep_stride}; c.inter = {d_inter, inter_stride};
  c.h_lost = h_lost; c.h_nlost = h_nlost; c.lost_cap = lost_cap;
  c.h_rep_esi = h_rep_esi; c.h_nrep = h_nrep; c.h_avail = h_nrep_avail; c.rep_cap = rep_cap;
  PlanRun *r = new PlanRun();
  const int rc = plan_launch(ctx, *r, c);
  if (rc) { delete r; return rc; }
  r->lost.assign(h_lost, h_lost + (size_t)nblk * lost_cap);
  r->resi.assign(h_rep_esi, h_rep_esi + (size_t)nblk * rep_cap);
  r->nlost.assign(h_nlost, h_nlost + nblk);
  r->nrep.assign(h_nrep, h_nrep + nblk);
  if (h_nrep_avail) r->avail.assign(h_nrep_avail, h_nrep_avail + nblk);
  r->call = c;
  r->call.h_lost = r->lost.data(); r->call.h_nlost = r->nlost.data(); r->call.h_rep_esi = r->resi.data(); r->call.h_nrep = r->nrep.data();
  if (h_nrep_avail) r->call.h_avail = r->avail.data();
  ctx->ahead.push_back(r);
  if (ctx->ahead.size() > ctx->ahead_hint) ctx->ahead_hint = (uint32_t)ctx->ahead.size();
  return 0;
}

/* every decode entry point ends here, with the call's record (completed here: io_aligned) */
static int decode(nrq_ctx *ctx, DecodeCall &c) {
  if (!c.src || c.T == 0 || c.nblk == 0 || !c.h_nlost || !c.h_nrep || !c.h_status) return fail(ctx, -1, "bad arguments");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const uint32_t K = c.K, nblk = c.nblk;
  c.io_aligned = c.src.aligned(nblk, c.T) && c.rep.aligned(nblk, c.T) && (!c.inter || c.inter.aligned(nblk, c.T));
  /* A call with one or two SMALL blocks (the reference's own harness: one block per call): the planner kernel is a chain of ~120
   * phases that a lone block cannot fill -- 200 us at K=100, 460 at K=1000, whatever the block count up to one per CU -- while the
   * host planner, sequential per block, needs ~0.45 us per source symbol on the GPU box's CPU.  Measured with the reference's
   * benchmark.c (decode column, Gbit/s, device / host planner): K=100 3.5 / 9.3, K=500 8.6 / 23.8, K=1000 16.7 / 23.2, K=1500
   * 20.8 / 24.1, K=2000 22.3 / 21.8, K=2500 25.5 / 23.6, K=3000 25.7 / 23.1, K=4000 34.8 / 17.9.  So the host plans when its estimate is the shorter
   * one (the knob host_plan_auto = 0: never), unless plans were issued ahead or the call solves in chunks.
   * (Several small blocks: decode_host plans them one after the other -- its worker threads cost more to start than such plans take.) */
  const bool host_small = ctx->planner && ctx->tune.host_plan_auto && ctx->ahead.empty() && !c.chunk_blocks &&
                          (uint64_t)38u * nblk * K < (uint64_t)20000u + (uint64_t)28u * K; /* (tools/small_calls.py: host call ~65 us + 0.3-0.4 us x K per block, planner-kernel
                                                                                                      * call ~270 us + 0.28 us x K: one block of K < 2000, two of K < 416, four of K < 161) */
  if (!ctx->planner || host_small) {
    const int rc_ = decode_host(ctx, c, nullptr);
    if (host_small) ctx->stats.host_planned = 0; /* (a choice, not a fallback: tests read host_planned as "the device planner gave up") */
    return rc_;
  }
  std::vector<uint8_t> fallback(nblk, 0);
  int rc = decode_device(ctx, c, &fallback);
  if (rc <= 0) return rc;
  /* blocks that exceeded a device-planner capacity are planned on the host (rare) */
  uint32_t nfb = 0;
  for (uint8_t f : fallback) nfb += f;
  rc = decode_host(ctx, c, fallback.data());
  ctx->stats.host_planned = nfb;
  if (ctx->tune.prof) fprintf(stderr, "[NRQ_PROF] %u of %u blocks re-planned on the host (device planner capacity)\n", nfb, nblk);
  return rc;
}

int nrq_decode_blocks_lazy(nrq_ctx *ctx, uint32_t K, uint32_t Kp, uint32_t T, uint32_t nblk, void *d_src, size_t src_stride,
                           const uint32_t *h_lost, const uint32_t *h_nlost, uint32_t lost_cap, const uint32_t *h_rep_esi,
                           const uint32_t *h_nrep, const uint32_t *h_nrep_avail, uint32_t rep_cap, const void *d_rep,
                           size_t rep_stride, void *d_inter, size_t inter_stride, int *h_status, uint32_t *h_used) {
  if (!ctx) return -1;
  DecodeCall c;
  c.K = K; c.Kp = Kp; c.T = T; c.nblk = nblk;
  c.src = {d_src, src_stride}; c.rep = {d_rep, rep_stride}; c.inter = {d_inter, inter_stride};
  c.h_lost = h_lost; c.h_nlost = h_nlost; c.lost_cap = lost_cap;
  c.h_rep_esi = h_rep_esi; c.h_nrep = h_nrep; c.h_avail = h_nrep_avail; c.rep_cap = rep_cap;
  c.h_status = h_status; c.h_used = h_used;
  return decode(ctx, c);
}

int nrq_decode_blocks(nrq_ctx *ctx, uint32_t K, uint32_t Kp, uint32_t T, uint32_t nblk, void *d_src, size_t src_stride,
                      const uint32_t *h_lost, const uint32_t *h_nlost, uint32_t lost_cap, const uint32_t *h_rep_esi,
                      const uint32_t *h_nrep, uint32_t rep_cap, const void *d_rep, size_t rep_stride, void *d_inter,
                      size_t inter_stride, int *h_status) {
  return nrq_decode_blocks_lazy(ctx, K, Kp, T, nblk, d_src, src_stride, h_lost, h_nlost, lost_cap, h_rep_esi, h_nrep, nullptr,
                                rep_cap, d_rep, rep_stride, d_inter, inter_stride, h_status, nullptr);
}

int nrq_decode_blocks_v(nrq_ctx *ctx, uint32_t K, uint32_t Kp, uint32_t T, uint32_t nblk, const uint64_t *d_src_v, const uint32_t *h_lost,
                        const uint32_t *h_nlost, uint32_t lost_cap, const uint32_t *h_rep_esi, const uint32_t *h_nrep,
                        const uint32_t *h_nrep_avail, uint32_t rep_cap, const uint64_t *d_rep_v, int *h_status, uint32_t *h_used) {
  return nrq_decode_blocks_vi(ctx, K, Kp, T, nblk, d_src_v, h_lost, h_nlost, lost_cap, h_rep_esi, h_nrep, h_nrep_avail, rep_cap, d_rep_v,
                              nullptr, h_status, h_used);
}

int nrq_decode_blocks_vi(nrq_ctx *ctx, uint32_t K, uint32_t Kp, uint32_t T, uint32_t nblk, const uint64_t *d_src_v, const uint32_t *h_lost,
                         const uint32_t *h_nlost, uint32_t lost_cap, const uint32_t *h_rep_esi, const uint32_t *h_nrep,
                         const uint32_t *h_nrep_avail, uint32_t rep_cap, const uint64_t *d_rep_v, const uint64_t *d_inter_v, int *h_status,
                         uint32_t *h_used) {
  if (!ctx || !d_src_v || !d_rep_v) return -1;
  DecodeCall c;
  c.K = K; c.Kp = Kp; c.T = T; c.nblk = nblk;
  c.src.vec = d_src_v; c.rep.vec = d_rep_v; c.inter.vec = d_inter_v;
  c.h_lost = h_lost; c.h_nlost = h_nlost; c.lost_cap = lost_cap;
  c.h_rep_esi = h_rep_esi; c.h_nrep = h_nrep; c.h_avail = h_nrep_avail; c.rep_cap = rep_cap;
  c.h_status = h_status; c.h_used = h_used;
  return decode(ctx, c);
}

int nrq_decode_blocks_vc(nrq_ctx *ctx, uint32_t K, uint32_t Kp, uint32_t T, uint32_t nblk, const uint64_t *d_src_v, const uint32_t *h_lost,
                         const uint32_t *h_nlost, uint32_t lost_cap, const uint32_t *h_rep_esi, const uint32_t *h_nrep,
                         const uint32_t *h_nrep_avail, uint32_t rep_cap, const uint64_t *d_rep_v, int *h_status, uint32_t *h_used,
                         uint32_t chunk_blocks, void *const *chunk_done, void *const *upload_done) {
  if (!ctx || !chunk_blocks || !chunk_done || !d_src_v || !d_rep_v) return -1;
  const uint32_t nchunks = (nblk + chunk_blocks - 1u) / chunk_blocks;
  DecodeCall c;
  c.K = K; c.Kp = Kp; c.T = T; c.nblk = nblk;
  c.src.vec = d_src_v; c.rep.vec = d_rep_v;
  c.h_lost = h_lost; c.h_nlost = h_nlost; c.lost_cap = lost_cap;
  c.h_rep_esi = h_rep_esi; c.h_nrep = h_nrep; c.h_avail = h_nrep_avail; c.rep_cap = rep_cap;
  c.h_status = h_status; c.h_used = h_used;
  if (!ctx->planner) {
    /* host planner: no chunks -- everything is solved by one launch, after all uploads; every event is recorded behind it */
    for (uint32_t i = 0; upload_done && i < nchunks; i++)
      if (upload_done[i]) HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, (hipEvent_t)upload_done[i], 0));
  } else {
    c.chunk_blocks = chunk_blocks; c.chunk_done = chunk_done; c.chunk_up = upload_done;
  }
  const int rc = decode(ctx, c);
  const bool chunked = c.chunk_blocks != 0 && ctx->stats.host_planned == 0;
  if (!chunked) /* (also when blocks were re-planned on the host and solved by a later launch: the events say "all done") */
    for (uint32_t i = 0; i < nchunks; i++)
      if (chunk_done[i]) HIPCHK(ctx, hipEventRecord((hipEvent_t)chunk_done[i], ctx->stream));
  return rc;
}

int nrq_gen_symbols(nrq_ctx *ctx, uint32_t K, uint32_t Kp, uint32_t T, uint32_t nblk, const void *d_inter, size_t inter_stride,
                    uint32_t n, const uint32_t *h_isi, void *d_out, size_t out_stride) {
  if (!ctx) return -1;
  if (!d_inter || !d_out || !h_isi || T == 0 || nblk == 0) return fail(ctx, -1, "bad arguments");
  if (n == 0) return 0;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  rq_params p;
  int rc = block_params(ctx, K, Kp, &p);
  if (rc) return rc;
  const int f = ctx->flip;
  ctx->flip ^= 1;
  HIPCHK(ctx, hipEventSynchronize(ctx->staged[f]));
  if ((rc = ensure_pin(ctx, ctx->staging[f], (size_t)n * 4))) return rc;
  if ((rc = ensure_dev(ctx, ctx->scratch[f], (size_t)n * 4))) return rc;
  memcpy(ctx->staging[f].p, h_isi, (size_t)n * 4);
  HIPCHK(ctx, hipMemcpyAsync(ctx->scratch[f].p, ctx->staging[f].p, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipEventRecord(ctx->staged[f], ctx->stream));
  hipLaunchKernelGGL(nrq_gen_kernel, dim3(n, nblk), dim3(NRQ_GEN_WG), 0, ctx->stream, p, T, (const uint8_t *)d_inter,
                     inter_stride, (const uint32_t *)ctx->scratch[f].p, (uint8_t *)d_out, out_stride);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int nrq_gen_symbols_dev(nrq_ctx *ctx, uint32_t K, uint32_t Kp, uint32_t T, uint32_t nblk, const void *d_inter, size_t inter_stride,
                        uint32_t n, const uint32_t *d_isi, void *d_out, size_t out_stride) {
  if (!ctx) return -1;
  if (!d_inter || !d_out || !d_isi || T == 0 || nblk == 0) return fail(ctx, -1, "bad arguments");
  if (n == 0) return 0;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  rq_params p;
  int rc = block_params(ctx, K, Kp, &p);
  if (rc) return rc;
  hipLaunchKernelGGL(nrq_gen_kernel, dim3(n, nblk), dim3(NRQ_GEN_WG), 0, ctx->stream, p, T, (const uint8_t *)d_inter,
                     inter_stride, d_isi, (uint8_t *)d_out, out_stride);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int nrq_dev_alloc(nrq_ctx *ctx, size_t bytes, void **out) {
  if (!ctx || !out) return -1;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  size_t want = bytes ? bytes : 16;
  want = (want + 4095) & ~(size_t)4095;
  auto it = ctx->pool_free.lower_bound(want);
  if (it != ctx->pool_free.end() && it->first <= want + want / 4 + 65536) {
    *out = it->second;
    ctx->pool_cached -= it->first;
    ctx->pool_free.erase(it);
    return 0;
  }
  if (nrq_inject(ctx)) { *out = nullptr; return fail(ctx, -10, "hipMalloc(%zu) failed: injected fault", want); }
  hipError_t e = hipMalloc(out, want);
  if (e != hipSuccess && !ctx->pool_free.empty()) { /* give the cached blocks back and try once more */
    (void)hipGetLastError();
    nrq_dev_trim(ctx);
    e = hipMalloc(out, want);
  }
  if (e != hipSuccess) { *out = nullptr; return fail(ctx, -10, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e)); }
  ctx->pool_size[*out] = want;
  return 0;
}
int nrq_dev_free(nrq_ctx *ctx, void *p) {
  if (!ctx) return -1;
  if (!p) return 0;
  auto it = ctx->pool_size.find(p);
  if (it == ctx->pool_size.end()) return fail(ctx, -1, "nrq_dev_free: not a block of this context");
  /* a block that is already cached is refused: a second entry would hand it to two owners and nrq_dev_trim would release it twice */
  for (auto r = ctx->pool_free.equal_range(it->second); r.first != r.second; ++r.first)
    if (r.first->second == p) return fail(ctx, -1, "nrq_dev_free: the block was freed already");
  ctx->pool_free.emplace(it->second, p);
  ctx->pool_cached += it->second;
  if (ctx->pool_cached > ((size_t)24 << 30)) nrq_dev_trim(ctx); /* keep the cache bounded */
  return 0;
}
int nrq_dev_pool_books(nrq_ctx *ctx, size_t out[3]) {
  if (!ctx || !out) return -1;
  out[0] = ctx->pool_size.size();
  out[1] = ctx->pool_free.size();
  out[2] = ctx->pool_cached;
  return 0;
}
int nrq_dev_trim(nrq_ctx *ctx) {
  if (!ctx) return -1;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipDeviceSynchronize());
  for (auto &kv : ctx->pool_free) {
    (void)hipFree(kv.second);
    ctx->pool_size.erase(kv.second);
  }
  ctx->pool_free.clear();
  ctx->pool_cached = 0;
  return 0;
}

/* page-locked host memory (what the copy engines read and write at PCIe speed without a staging pass) */
int nrq_host_alloc_pinned(size_t bytes, void **out) {
  if (!out) return -1;
  *out = nullptr;
  return hipHostMalloc(out, bytes ? bytes : 16, hipHostMallocPortable) == hipSuccess ? 0 : -10; /* (every device of the process may DMA it) */
}
void nrq_host_free_pinned(void *p) {
  if (p) (void)hipHostFree(p);
}
int nrq_host_register(void *p, size_t bytes) { return hipHostRegister(p, bytes, hipHostRegisterPortable) == hipSuccess ? 0 : -10; }
void nrq_host_unregister(void *p) {
  if (p) (void)hipHostUnregister(p);
}
int nrq_host_is_pinned(const void *p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return 0; }
  return a.type == hipMemoryTypeHost ? 1 : 0;
}
/* the whole range [p, p + bytes): its first and last byte and a probe every 2 MiB in between (registrations are page
 * granular; a range that is page-locked at both ends and every 2 MiB is taken as page-locked throughout) */
int nrq_host_range_is_pinned(const void *p, size_t bytes) {
  if (!p) return 0;
  if (!bytes) return nrq_host_is_pinned(p);
  const uint8_t *q = static_cast<const uint8_t *>(p);
  if (!nrq_host_is_pinned(q) || !nrq_host_is_pinned(q + bytes - 1)) return 0;
  const size_t step = (size_t)2 << 20;
  for (size_t o = step - (reinterpret_cast<uintptr_t>(q) & (step - 1)); o < bytes; o += step)
    if (!nrq_host_is_pinned(q + o)) return 0;
  return 1;
}

/* the address a kernel reaches page-locked host memory at (hipHostMalloc'ed or hipHostRegister'ed); 0 = it cannot */
uint64_t nrq_host_device_address(const void *p) {
  if (!p || !nrq_host_is_pinned(p)) return 0;
  void *d = nullptr;
  if (hipHostGetDevicePointer(&d, const_cast<void *>(p), 0) != hipSuccess) { (void)hipGetLastError(); return 0; }
  return (uint64_t)(uintptr_t)d;
}

/* streams and events of the object layer's copy pipeline; stream selector: 0 = the context's stream, 1 = upload
 * stream, 2 = download stream */
static hipStream_t sel_stream(nrq_ctx *ctx, int which) {
  return which == 1 ? ctx->aux[0] : which == 2 ? ctx->aux[1] : which == 3 ? ctx->aux[2] : ctx->stream;
}
int nrq_ctl_copy(nrq_ctx *ctx, int stream, void *d_dst, const void *h_pinned, size_t bytes) {
  if (!ctx || !d_dst || !h_pinned || (bytes & 15u) || (((uintptr_t)d_dst | (uintptr_t)h_pinned) & 15u)) return -1;
  if (!bytes) return 0;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const uint32_t n16 = (uint32_t)(bytes / 16u);
  uint32_t g = (n16 + 255u) / 256u;
  if (g > 256u) g = 256u;
  hipLaunchKernelGGL(nrq_ctl_copy_kernel, dim3(g), dim3(256), 0, sel_stream(ctx, stream), reinterpret_cast<uint4 *>(d_dst),
                     reinterpret_cast<const uint4 *>(h_pinned), n16);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}
int nrq_copy_on(nrq_ctx *ctx, int stream, void *dst, const void *src, size_t bytes) {
  if (!ctx) return -1;
  if (!bytes) return 0;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, sel_stream(ctx, stream)));
  return 0;
}
int nrq_memset_on(nrq_ctx *ctx, int stream, void *d_dst, int value, size_t bytes) {
  if (!ctx) return -1;
  if (!bytes) return 0;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipMemsetAsync(d_dst, value, bytes, sel_stream(ctx, stream)));
  return 0;
}
int nrq_event_new(nrq_ctx *ctx, void **out) {
  if (!ctx || !out) return -1;
  hipEvent_t e;
  HIPCHK(ctx, hipSetDevice(ctx->device)); /* (an event belongs to the device that is current when it is created) */
  HIPCHK(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  *out = e;
  return 0;
}
void nrq_event_free(void *ev) {
  if (ev) (void)hipEventDestroy((hipEvent_t)ev);
}
int nrq_event_record(nrq_ctx *ctx, void *ev, int stream) {
  if (!ctx || !ev) return -1;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipEventRecord((hipEvent_t)ev, sel_stream(ctx, stream)));
  return 0;
}
int nrq_stream_wait(nrq_ctx *ctx, int stream, void *ev) {
  if (!ctx || !ev) return -1;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamWaitEvent(sel_stream(ctx, stream), (hipEvent_t)ev, 0));
  return 0;
}
int nrq_event_sync(nrq_ctx *ctx, void *ev) {
  if (!ctx || !ev) return -1;
  HIPCHK(ctx, hipEventSynchronize((hipEvent_t)ev));
  return 0;
}
int nrq_stream_sync(nrq_ctx *ctx, int stream) {
  if (!ctx) return -1;
  HIPCHK(ctx, hipStreamSynchronize(sel_stream(ctx, stream)));
  return 0;
}

int nrq_scatter_symbols(nrq_ctx *ctx, int stream, const void *d_blob, uint32_t n, uint32_t T, const uint64_t *h_dst) {
  if (!ctx || !d_blob || !h_dst || T == 0) return -1;
  if (n == 0) return 0;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const int f = ctx->scat_flip;
  ctx->scat_flip ^= 1;
  HIPCHK(ctx, hipEventSynchronize(ctx->scat_ev[f])); /* the copy out of this pinned image two calls ago */
  int rc;
  if ((rc = ensure_pin(ctx, ctx->scat_pin[f], (size_t)n * 8))) return rc;
  if ((rc = ensure_dev(ctx, ctx->scat_dev[f], (size_t)n * 8))) return rc;
  memcpy(ctx->scat_pin[f].p, h_dst, (size_t)n * 8);
  hipStream_t st = sel_stream(ctx, stream);
  HIPCHK(ctx, hipMemcpyAsync(ctx->scat_dev[f].p, ctx->scat_pin[f].p, (size_t)n * 8, hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipEventRecord(ctx->scat_ev[f], st));
  hipLaunchKernelGGL(nrq_scatter_kernel, dim3(n), dim3(128), 0, st, (const uint8_t *)d_blob, T, (const uint64_t *)ctx->scat_dev[f].p, n);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int nrq_scatter_symbols_dev(nrq_ctx *ctx, int stream, const void *d_blob, uint32_t n, uint32_t T, const uint64_t *d_dst) {
  if (!ctx || !d_blob || !d_dst || T == 0) return -1;
  if (n == 0) return 0;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(nrq_scatter_kernel, dim3(n), dim3(128), 0, sel_stream(ctx, stream), (const uint8_t *)d_blob, T, d_dst, n);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int nrq_move_rows_dev(nrq_ctx *ctx, int stream, const uint64_t *d_pairs, uint32_t n, uint32_t T) {
  if (!ctx || !d_pairs || T == 0) return -1;
  if (n == 0) return 0;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(nrq_move_rows_kernel, dim3(n), dim3(128), 0, sel_stream(ctx, stream), d_pairs, T, n);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int nrq_dev_upload(nrq_ctx *ctx, void *d_dst, const void *h_src, size_t bytes) {
  if (!ctx) return -1;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return 0;
}
int nrq_dev_download(nrq_ctx *ctx, void *h_dst, const void *d_src, size_t bytes) {
  if (!ctx) return -1;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return 0;
}
int nrq_dev_upload_async(nrq_ctx *ctx, void *d_dst, const void *h_src, size_t bytes) {
  if (!ctx) return -1;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, ctx->stream));
  return 0;
}
int nrq_dev_download_async(nrq_ctx *ctx, void *h_dst, const void *d_src, size_t bytes) {
  if (!ctx) return -1;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
  return 0;
}
int nrq_dev_copy(nrq_ctx *ctx, void *d_dst, const void *d_src, size_t bytes) {
  if (!ctx) return -1;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipMemcpyAsync(d_dst, d_src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  return 0;
}
int nrq_dev_memset(nrq_ctx *ctx, void *d_dst, int value, size_t bytes) {
  if (!ctx) return -1;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipMemsetAsync(d_dst, value, bytes, ctx->stream));
  return 0;
}

int nrq_ktime_enable(nrq_ctx *ctx, int on) {
  if (!ctx) return -1;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  ctx->ktime_on = on != 0;
  ctx->ktime_used = 0;
  ctx->ptime_used = 0;
  if (on) {
    if (!ctx->ktime_base) HIPCHK(ctx, hipEventCreate(&ctx->ktime_base.h));
    HIPCHK(ctx, hipEventRecord(ctx->ktime_base, ctx->stream));
  }
  return 0;
}
/* launch intervals [start, start+dur) in ms relative to ref's nrq_ktime_enable (ref may be another context of
 * the same device: kernels of several streams overlap and the caller wants the union of their busy time) */
int nrq_ktime_read_intervals(nrq_ctx *ctx, nrq_ctx *ref, float *start_ms, float *dur_ms, uint32_t cap, uint32_t *count) {
  if (!ctx || !ref || !count || !ref->ktime_base) return -1;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  HIPCHK(ctx, hipEventSynchronize(ref->ktime_base));
  uint32_t n = (uint32_t)ctx->ktime_used;
  for (uint32_t k = 0; k < n && k < cap; k++) {
    HIPCHK(ctx, hipEventElapsedTime(&start_ms[k], ref->ktime_base, ctx->ktime_pool[k].first));
    HIPCHK(ctx, hipEventElapsedTime(&dur_ms[k], ctx->ktime_pool[k].first, ctx->ktime_pool[k].second));
  }
  *count = n;
  ctx->ktime_used = 0;
  return 0;
}
int nrq_ptime_read(nrq_ctx *ctx, float *ms_out, uint32_t cap, uint32_t *count) {
  if (!ctx || !count) return -1;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->plan_stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->plan_stream_b));
  uint32_t n = (uint32_t)ctx->ptime_used;
  for (uint32_t k = 0; k < n && k < cap; k++)
    HIPCHK(ctx, hipEventElapsedTime(&ms_out[k], ctx->ptime_pool[k].first, ctx->ptime_pool[k].second));
  *count = n;
  ctx->ptime_used = 0;
  return 0;
}
int nrq_ktime_read(nrq_ctx *ctx, float *ms_out, uint32_t cap, uint32_t *count) {
  if (!ctx || !count) return -1;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  uint32_t n = (uint32_t)ctx->ktime_used;
  for (uint32_t k = 0; k < n && k < cap; k++)
    HIPCHK(ctx, hipEventElapsedTime(&ms_out[k], ctx->ktime_pool[k].first, ctx->ktime_pool[k].second));
  *count = n;
  ctx->ktime_used = 0;
  return 0;
}

int nrq_timer_start(nrq_ctx *ctx) {
  if (!ctx) return -1;
  HIPCHK(ctx, hipEventRecord(ctx->t0, ctx->stream));
  return 0;
}
int nrq_timer_stop_ms(nrq_ctx *ctx, float *ms) {
  if (!ctx || !ms) return -1;
  HIPCHK(ctx, hipEventRecord(ctx->t1, ctx->stream));
  HIPCHK(ctx, hipEventSynchronize(ctx->t1));
  HIPCHK(ctx, hipEventElapsedTime(ms, ctx->t0, ctx->t1));
  return 0;
}

} /* extern "C" */

/* the per-call device arrays of a reception, a sender or a set: kept from call to call, grown when a call needs more */
struct DevScratch {
  void *p;
  size_t cap;
  int ensure(nrq_ctx *ctx, size_t need) {
    if (cap >= need) return 0;
    if (p) HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); /* (the previous call's kernels may still read it) */
    release(ctx);
    const int rc = nrq_dev_alloc(ctx, need, &p);
    if (!rc) cap = need;
    return rc;
  }
  void release(nrq_ctx *ctx) { /* (the owner has waited for the stream: the pool hands freed blocks out again at once) */
    if (p) nrq_dev_free(ctx, p);
    p = nullptr;
    cap = 0;
  }
};

/* ================================================ a 256-thread workgroup's scans and sums ==== */
/* ps = 256 words of LDS, t = threadIdx.x; every thread of the workgroup calls, each ends with a barrier behind its last write.
 * A caller that goes round again puts a barrier of its own behind its last read of ps. */

/* inclusive scan (Hillis-Steele) of the threads' v: returns v of threads 0 .. t summed, ps[255] is the total */
__device__ __forceinline__ uint32_t wg_scan(uint32_t *ps, uint32_t t, uint32_t v) {
  ps[t] = v;
  __syncthreads();
  for (uint32_t d = 1; d < 256u; d <<= 1) {
    const uint32_t u = t >= d ? ps[t - d] : 0u;
    __syncthreads();
    ps[t] += u;
    __syncthreads();
  }
  return ps[t];
}

/* tree sum of the threads' v, returned to every thread */
__device__ __forceinline__ uint32_t wg_sum(uint32_t *ps, uint32_t t, uint32_t v) {
  ps[t] = v;
  __syncthreads();
  for (uint32_t s = 128; s; s >>= 1) {
    if (t < s) ps[t] += ps[t + s];
    __syncthreads();
  }
  return ps[0];
}

/* a[0 .. n) -> start + its exclusive prefix sums, in place: a run of entries per thread, a scan over the threads' sums.  Returns
 * the sum of the entries. */
__device__ __forceinline__ uint32_t wg_scan_runs(uint32_t *ps, uint32_t t, uint32_t *a, uint32_t n, uint32_t start) {
  const uint32_t per = (n + 255u) / 256u, j0 = min(n, t * per), j1 = min(n, j0 + per);
  uint32_t s = 0;
  for (uint32_t j = j0; j < j1; j++) s += a[j];
  uint32_t run = start + wg_scan(ps, t, s) - s;
  for (uint32_t j = j0; j < j1; j++) { const uint32_t v = a[j]; a[j] = run; run += v; }
  return ps[255];
}

/* ================================================ device-resident receiver (nrq_rx_*, ingest_body.h) ==== */
/* The per-block passes as workgroup bodies of (reception, block): nrq_ing_*_kernel runs them on its by-value reception and
 * blockIdx.x, nrq_ings_*_kernel on the member and block it finds in the set's table (lss_block).  The per-tile ranking of the
 * classify pass is a body too (ing_rank_wg), behind the one-symbol, the several-symbol and the set's classify kernel.  The three
 * tile histogram kernels keep their own few lines: the single forms count in 256 static words, a word per thread, the set's in
 * a dynamic array walked by loops, and one body for both would change the single forms' code. */

/* done: the max and the count of ing_done_part over the block's K source ESIs */
__device__ __forceinline__ void ing_done_wg(const ing_rx *r, uint32_t b, uint32_t *smx, uint32_t *scnt) {
  const uint32_t t = threadIdx.x, K = r->K;
  uint32_t mx = 0, cnt = 0;
  if (r->gaps[b])
    for (uint32_t e = t; e < K; e += 256u) ing_done_part(r, b, e, &mx, &cnt);
  smx[t] = mx;
  scnt[t] = cnt;
  __syncthreads();
  for (uint32_t s = 128; s; s >>= 1) {
    if (t < s) { smx[t] = max(smx[t], smx[t + s]); scnt[t] += scnt[t + s]; }
    __syncthreads();
  }
  if (t == 0) ing_done_finish(r, b, smx[0], scnt[0]);
}

/* scan: the block's nt tile counts -> the row of each tile's first candidate, starting at the rows already used */
__device__ __forceinline__ void ing_scan_wg(const ing_rx *r, uint32_t b, uint32_t *base, uint32_t nt, uint32_t *ps) {
  const uint32_t nrep0 = r->nrep[b]; /* (read by every thread before the scan's barriers, written behind them) */
  const uint32_t total = wg_scan_runs(ps, threadIdx.x, base, nt, nrep0);
  if (threadIdx.x == 0) r->nrep[b] = min(nrep0 + total, r->rep_cap);
}

/* mark: a block a decode recovered: every source ESI counts as seen from now on (what nanorq_repair_block does to the bitmap) */
__device__ __forceinline__ void ing_mark_wg(const ing_rx *r, uint32_t b) {
  const uint32_t nw = ing_src_words(r);
  uint32_t *seen = r->seen + (size_t)b * r->bm_words;
  for (uint32_t w = threadIdx.x; w < nw; w += 256u) seen[w] |= ing_src_mask(r, w);
  if (threadIdx.x == 0) r->gaps[b] = 0;
}

/* list fill: the block's repair ESIs in arrival order, then its missing source ESIs ascending (LSS_ROUND words per round: a scan
 * over their counts places each word's ESIs), to out[0 ..] */
__device__ __forceinline__ void ing_lists_fill_wg(const ing_rx *r, uint32_t b, uint32_t *out, uint32_t *ps) {
  const uint32_t t = threadIdx.x, nrep = r->nrep[b], nw = ing_src_words(r);
  for (uint32_t q = t; q < nrep; q += 256u) out[q] = r->rep_esi[(size_t)b * r->rep_cap + q];
  uint32_t o = nrep;
  for (uint32_t w0 = 0; w0 < nw; w0 += LSS_ROUND) {
    const uint32_t w = w0 + t, miss = lss_miss(r, b, w), cnt = ing_popc(miss);
    lss_put(w, miss, out + o + wg_scan(ps, t, cnt) - cnt);
    o += ps[255];
    __syncthreads();
  }
}

/* rank: the row of the thread's repair candidate (block g of the `stride` the tile counts per wave, or ING_NONE) -- the tile's
 * first row for the block, from the scan, plus the candidate's rank among the block's candidates in the tile, in packet order:
 * wave by wave a ballot per distinct block present in the wave, whose count goes to wc[wave * stride + block] (zeroed by the
 * caller, a barrier behind it) for the waves after it.  ING_NONE for no candidate. */
__device__ __forceinline__ uint32_t ing_rank_wg(uint32_t *wc, uint32_t stride, uint32_t g, const uint32_t *base, uint32_t ntiles) {
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const bool cand = g != ING_NONE;
  uint64_t todo = __ballot(cand);
  uint32_t rank = 0;
  while (todo) { /* (wave-uniform) */
    const int leader = __ffsll((unsigned long long)todo) - 1;
    const uint32_t lg = __shfl(g, leader);
    const bool mine = cand && g == lg;
    const uint64_t m = __ballot(mine);
    if (mine) rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if ((int)lane == leader) wc[w * stride + lg] = (uint32_t)__popcll(m);
    todo &= ~m;
  }
  __syncthreads();
  uint32_t row = ING_NONE;
  if (cand) {
    row = base[(size_t)g * ntiles + blockIdx.x] + rank;
    for (uint32_t w2 = 0; w2 < w; w2++) row += wc[w2 * stride + g];
  }
  return row;
}

__global__ __launch_bounds__(256) void nrq_ing_init_kernel(ing_rx r) {
  const uint32_t b = blockIdx.x * 256u + threadIdx.x;
  if (b < r.nblk) { r.gaps[b] = r.K; r.nrep[b] = 0; }
}

__global__ __launch_bounds__(256) void nrq_ing_first_kernel(ing_rx r, ing_call c) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k < c.n) ing_first(&r, &c, k);
}

/* one workgroup per block */
__global__ __launch_bounds__(256) void nrq_ing_done_kernel(ing_rx r) {
  __shared__ uint32_t smx[256], scnt[256];
  ing_done_wg(&r, blockIdx.x, smx, scnt);
}

/* one workgroup per tile of ING_TILE packets: repair candidates per block */
__global__ __launch_bounds__(256) void nrq_ing_hist_kernel(ing_rx r, ing_call c) {
  __shared__ uint32_t h[256];
  const uint32_t t = threadIdx.x, k = blockIdx.x * ING_TILE + t;
  h[t] = 0;
  __syncthreads();
  if (k < c.n) {
    const uint32_t b = ing_cand(&r, &c, k);
    if (b != ING_NONE) atomicAdd(&h[b], 1u);
  }
  __syncthreads();
  if (t < r.nblk) c.base[(size_t)t * c.ntiles + blockIdx.x] = h[t];
}

/* one workgroup per block: exclusive scan of the block's tile counts, starting at the rows already used */
__global__ __launch_bounds__(256) void nrq_ing_scan_kernel(ing_rx r, ing_call c) {
  __shared__ uint32_t ps[256];
  ing_scan_wg(&r, blockIdx.x, c.base + (size_t)blockIdx.x * c.ntiles, c.ntiles, ps);
}

/* one workgroup per tile: the row of every repair candidate (ing_rank_wg, 256 counters per wave), then the result of every packet */
__global__ __launch_bounds__(256) void nrq_ing_classify_kernel(ing_rx r, ing_call c) {
  __shared__ uint32_t wc[4][256];
  const uint32_t t = threadIdx.x, k = blockIdx.x * ING_TILE + t;
  for (uint32_t i = t; i < 4u * 256u; i += 256u) wc[i >> 8][i & 255u] = 0;
  __syncthreads();
  const uint32_t b = k < c.n ? ing_cand(&r, &c, k) : ING_NONE;
  const uint32_t row = ing_rank_wg(&wc[0][0], 256u, b, c.base, c.ntiles);
  if (k < c.n) ing_classify(&r, &c, k, row);
}

/* one wave per packet: the payload (at payload_off in the packet: 0, or behind an inline header of 4 or 8 bytes) to its row,
 * 16-byte accesses when both ends and T allow (tag mode with a 16-byte stride), else 4-byte (a 4-byte header), else bytes; two
 * accesses in flight per lane */
__global__ __launch_bounds__(256) void nrq_ing_copy_kernel(const uint8_t *__restrict__ pkts, uint64_t pkt_stride, const uint64_t *__restrict__ dst,
                                                           uint32_t n, uint32_t T, uint32_t payload_off) {
  const uint32_t k = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (k >= n) return;
  uint8_t *__restrict__ d = reinterpret_cast<uint8_t *>(dst[k]);
  if (!d) return;
  const uint8_t *__restrict__ s = pkts + (size_t)k * pkt_stride + payload_off;
  const uintptr_t al = reinterpret_cast<uintptr_t>(s) | reinterpret_cast<uintptr_t>(d) | T;
  if ((al & 15u) == 0) {
    for (uint32_t off = lane * 16u; off < T; off += 2u * 1024u) {
      const uint4 v0 = *reinterpret_cast<const uint4 *>(s + off);
      const bool two = off + 1024u < T;
      uint4 v1;
      if (two) v1 = *reinterpret_cast<const uint4 *>(s + off + 1024u);
      *reinterpret_cast<uint4 *>(d + off) = v0;
      if (two) *reinterpret_cast<uint4 *>(d + off + 1024u) = v1;
    }
  } else if ((al & 3u) == 0) {
    for (uint32_t off = lane * 4u; off < T; off += 2u * 256u) {
      const uint32_t v0 = *reinterpret_cast<const uint32_t *>(s + off);
      const bool two = off + 256u < T;
      uint32_t v1 = 0;
      if (two) v1 = *reinterpret_cast<const uint32_t *>(s + off + 256u);
      *reinterpret_cast<uint32_t *>(d + off) = v0;
      if (two) *reinterpret_cast<uint32_t *>(d + off + 256u) = v1;
    }
  } else {
    for (uint32_t off = lane; off < T; off += 64u) d[off] = s[off];
  }
}

__global__ __launch_bounds__(256) void nrq_ing_fold_kernel(ing_rx r, ing_call c) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k < c.n) ing_fold(&r, &c, k);
}

struct ing_mask { uint32_t w[8]; }; /* a bit per block of the reception (nblk <= 256) */
struct tx_sender;
struct nrq_rxset;

/* the blocks a decode recovered: one workgroup per block, at work where the block's bit is set */
__global__ __launch_bounds__(256) void nrq_ing_mark_kernel(ing_rx r, ing_mask m) {
  const uint32_t b = blockIdx.x;
  if ((m.w[b >> 5] >> (b & 31u)) & 1u) ing_mark_wg(&r, b);
}

/* one workgroup per block: the compact lists.  out = gaps[nblk], nrep[nblk], then block by block its repair ESIs (arrival
 * order) and its missing source ESIs (ascending).  One launch: lane 0 sums the counts of the blocks before its own */
__global__ __launch_bounds__(256) void nrq_ing_lists_kernel(ing_rx r, uint32_t *out) {
  __shared__ uint32_t ps[256];
  __shared__ uint32_t s_off;
  const uint32_t b = blockIdx.x, t = threadIdx.x;
  if (t == 0) {
    uint32_t off = 2u * r.nblk;
    for (uint32_t i = 0; i < b; i++) off += r.gaps[i] + r.nrep[i];
    s_off = off;
    out[b] = r.gaps[b];
    out[r.nblk + b] = r.nrep[b];
  }
  __syncthreads();
  ing_lists_fill_wg(&r, b, out + s_off, ps);
}

struct nrq_rx {
  nrq_ctx *ctx;
  ing_rx r;
  uint32_t Kp;
  void *state;          /* first | seen | gaps | nrep | live | rep_esi */
  void *own_src, *own_rep;
  DevScratch scratch;   /* per-call arrays */
  void *lists;          /* nrq_ing_lists_kernel output, written anew by every call that reads it.  rx_list_count borrows its first
                         * nblk + 1 words for the offsets and total of a held or want listing: all users run on the context's
                         * stream and none expects the buffer to survive from one call to the next -- keep it so */
  tx_sender *relay;     /* the relay attached to this reception (nrq_rx_relay / nrq_orx_relay), or null ... */
  uint32_t relay_seg, relay_b0; /* ... in whose table this reception is segment relay_seg, its block 0 the span's block relay_b0 */
  nrq_rxset *set;       /* the reception set this reception is a member of (nrq_rxset_attach), or null */
};

/* the relay's side of a reception (defined with the senders below) */
static uint64_t relay_inter(const tx_sender *tx, uint32_t seg, uint32_t b); /* where block b of segment seg has its intermediate symbols */
static void relay_set(tx_sender *tx, uint32_t b0, uint32_t nblk, bool valid); /* blocks b0 .. b0+nblk-1 of the span: intermediate symbols (not) written */
static void relay_detach(tx_sender *tx);                                    /* a reception of the relay goes away */
static void rxset_drop(nrq_rx *rx);                                         /* a member of a reception set goes away (defined with the sets below) */

static size_t rx_al(size_t x) { return (x + 255u) & ~(size_t)255u; }

static int rx_init_state(nrq_rx *rx) {
  nrq_ctx *ctx = rx->ctx;
  const ing_rx &r = rx->r;
  HIPCHK(ctx, hipMemsetAsync(r.first, 0xFF, (size_t)r.nblk * r.m1 * 4u, ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(r.seen, 0, (size_t)r.nblk * r.bm_words * 4u, ctx->stream));
  hipLaunchKernelGGL(nrq_ing_init_kernel, dim3(1), dim3(256), 0, ctx->stream, r);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

/* What the add calls share once the flags are read and there is something to do: the checks of the packet arguments (G: symbols a
 * packet can carry, 0 in the one-symbol forms, whose texts do not speak of it; pkt_len: the shortest stride a packet fits) and the
 * ing_call over n items -- packets, or slots -- of nblk blocks, its arrays carved out of `scratch` with `tail` more bytes behind them
 * at *tailp for the form's own array. */
static int ing_call_of(nrq_ctx *ctx, DevScratch &scratch, const char *who, const void *d_pkts, size_t pkt_stride, const uint32_t *d_tags,
                       uint32_t n, uint32_t G, size_t pkt_len, bool inl, uint32_t nblk, int32_t *d_results, size_t tail, ing_call *c,
                       uint8_t **tailp) {
  const uint64_t items = (uint64_t)n * (G ? G : 1u);
  if (!d_pkts || items > 0x7FFFFFFFu) return G ? fail(ctx, -1, "%s: bad packets (n=%u, G=%u)", who, n, G) : fail(ctx, -1, "%s: bad packets (n=%u)", who, n);
  if (inl == (d_tags != nullptr)) return fail(ctx, -1, "%s: give either d_tags or NRQ_RX_TAG_INLINE", who);
  if (pkt_stride < pkt_len)
    return G ? fail(ctx, -1, "%s: pkt_stride %zu shorter than a packet of %u symbols", who, pkt_stride, G)
             : fail(ctx, -1, "%s: pkt_stride %zu shorter than a packet", who, pkt_stride);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const uint32_t ni = (uint32_t)items;
  *c = ing_call{};
  c->pkts = (const uint8_t *)d_pkts;
  c->pkt_stride = pkt_stride;
  c->tags = d_tags;
  c->n = ni;
  c->ntiles = (ni + ING_TILE - 1u) / ING_TILE;
  const size_t o_codes = rx_al((size_t)ni * 4u), o_fidx = o_codes + rx_al((size_t)ni * 4u), o_dst = o_fidx + rx_al((size_t)ni * 4u),
               o_base = o_dst + rx_al((size_t)ni * 8u), o_tail = o_base + rx_al((size_t)nblk * c->ntiles * 4u);
  const int rc = scratch.ensure(ctx, o_tail + rx_al(tail));
  if (rc) return rc;
  uint8_t *s = (uint8_t *)scratch.p;
  c->tagv = (uint32_t *)s;
  c->codes = d_results ? d_results : (int32_t *)(s + o_codes);
  c->fidx = (uint32_t *)(s + o_fidx);
  c->dst = (uint64_t *)(s + o_dst);
  c->base = (uint32_t *)(s + o_base);
  if (tailp) *tailp = s + o_tail;
  return 0;
}

extern "C" {

int nrq_rx_create(nrq_ctx *ctx, uint32_t K, uint32_t Kp, uint32_t T, uint32_t nblk, uint32_t sbn0, uint32_t max_esi, uint32_t rep_cap,
                  void *d_src, size_t src_stride, void *d_rep, size_t rep_stride, nrq_rx **out) {
  if (!ctx) return -1;
  if (!out) return fail(ctx, -1, "nrq_rx_create: out is NULL");
  *out = nullptr;
  uint32_t prm[10];
  if (nrq_params(K, prm) != 0) return fail(ctx, -1, "nrq_rx_create: K=%u out of range", K);
  if (Kp == 0) Kp = prm[0];
  if (Kp < prm[0] || nrq_params(Kp, prm) != 0 || prm[0] != Kp) return fail(ctx, -1, "nrq_rx_create: K'=%u is not a table row for K=%u", Kp, K);
  if (max_esi == 0) max_esi = 2u * Kp; /* the object layer's default (nanorq_api.c) */
  if (T == 0 || nblk == 0 || nblk > 256u || sbn0 + nblk > 256u) return fail(ctx, -1, "nrq_rx_create: bad T / nblk / sbn0 (%u %u %u)", T, nblk, sbn0);
  if (max_esi < Kp || max_esi >= (1u << 24)) return fail(ctx, -1, "nrq_rx_create: max_esi %u outside [K', 2^24)", max_esi);
  if (rep_cap == 0) return fail(ctx, -1, "nrq_rx_create: rep_cap is 0");
  if ((d_src && src_stride < (size_t)K * T) || (d_rep && rep_stride < (size_t)rep_cap * T))
    return fail(ctx, -1, "nrq_rx_create: a row stride is shorter than its block");
  nrq_rx *rx = new (std::nothrow) nrq_rx();
  if (!rx) return fail(ctx, -1, "nrq_rx_create: out of host memory");
  rx->ctx = ctx;
  rx->Kp = Kp;
  ing_rx &r = rx->r;
  r.K = K; r.T = T; r.nblk = nblk; r.sbn0 = sbn0; r.max_esi = max_esi; r.rep_cap = rep_cap;
  r.m1 = max_esi + 1u;
  r.bm_words = max_esi / 32u + 1u;
  int rc = 0;
  if (!d_src) {
    src_stride = (size_t)K * T;
    if ((rc = nrq_dev_alloc(ctx, (size_t)nblk * src_stride, &rx->own_src))) goto bad;
    d_src = rx->own_src;
  }
  if (!d_rep) {
    rep_stride = (size_t)rep_cap * T;
    if ((rc = nrq_dev_alloc(ctx, (size_t)nblk * rep_stride, &rx->own_rep))) goto bad;
    d_rep = rx->own_rep;
  }
  r.src = (uint8_t *)d_src; r.src_stride = src_stride;
  r.rep = (uint8_t *)d_rep; r.rep_stride = rep_stride;
  {
    const size_t o_seen = rx_al((size_t)nblk * r.m1 * 4u), o_gaps = o_seen + rx_al((size_t)nblk * r.bm_words * 4u),
                 o_nrep = o_gaps + rx_al(nblk * 4u), o_live = o_nrep + rx_al(nblk * 4u), o_resi = o_live + rx_al(nblk * 4u),
                 total = o_resi + rx_al((size_t)nblk * rep_cap * 4u);
    if ((rc = nrq_dev_alloc(ctx, total, &rx->state))) goto bad;
    uint8_t *s = (uint8_t *)rx->state;
    r.first = (uint32_t *)s; r.seen = (uint32_t *)(s + o_seen); r.gaps = (uint32_t *)(s + o_gaps); r.nrep = (uint32_t *)(s + o_nrep);
    r.live = (uint32_t *)(s + o_live); r.rep_esi = (uint32_t *)(s + o_resi);
  }
  if ((rc = nrq_dev_alloc(ctx, ((size_t)2 * nblk + (size_t)nblk * K + (size_t)nblk * rep_cap) * 4u, &rx->lists))) goto bad;
  if ((rc = rx_init_state(rx))) goto bad;
  *out = rx;
  return 0;
bad:
  nrq_rx_destroy(rx);
  return rc;
}

void nrq_rx_destroy(nrq_rx *rx) {
  if (!rx) return;
  nrq_ctx *ctx = rx->ctx;
  if (rx->relay) relay_detach(rx->relay); /* (its later calls fail with an error text; it frees what it owns itself) */
  if (rx->set) rxset_drop(rx);            /* (the set's table is rewritten without it, behind the work enqueued so far) */
  (void)hipStreamSynchronize(ctx->stream); /* (the pool hands freed blocks out again at once) */
  for (void *p : {rx->own_src, rx->own_rep, rx->state, rx->lists})
    if (p) nrq_dev_free(ctx, p);
  rx->scratch.release(ctx);
  delete rx;
}

int nrq_rx_reset(nrq_rx *rx) {
  if (!rx) return -1;
  HIPCHK(rx->ctx, hipSetDevice(rx->ctx->device));
  if (rx->relay) relay_set(rx->relay, rx->relay_b0, rx->r.nblk, false); /* (emits enqueued before carry their mask by value) */
  return rx_init_state(rx);
}

void *nrq_rx_src(nrq_rx *rx) { return rx ? rx->r.src : nullptr; }
void *nrq_rx_rep(nrq_rx *rx) { return rx ? rx->r.rep : nullptr; }

int nrq_rx_add(nrq_rx *rx, const void *d_pkts, size_t pkt_stride, const uint32_t *d_tags, uint32_t n, uint32_t flags, int32_t *d_results) {
  if (!rx) return -1;
  nrq_ctx *ctx = rx->ctx;
  const ing_rx &r = rx->r;
  const bool inl = (flags & NRQ_RX_TAG_INLINE) != 0;
  if (flags & ~(uint32_t)NRQ_RX_TAG_INLINE) return fail(ctx, -1, "nrq_rx_add: unknown flags 0x%x", flags);
  if (n == 0) return 0;
  ing_call c;
  const int rc = ing_call_of(ctx, rx->scratch, "nrq_rx_add", d_pkts, pkt_stride, d_tags, n, 0, (size_t)r.T + (inl ? 4u : 0u), inl, r.nblk,
                             d_results, 0, &c, nullptr);
  if (rc) return rc;
  hipStream_t st = ctx->stream;
  const uint32_t g = (n + 255u) / 256u;
  hipLaunchKernelGGL(nrq_ing_first_kernel, dim3(g), dim3(256), 0, st, r, c);
  hipLaunchKernelGGL(nrq_ing_done_kernel, dim3(r.nblk), dim3(256), 0, st, r);
  hipLaunchKernelGGL(nrq_ing_hist_kernel, dim3(c.ntiles), dim3(256), 0, st, r, c);
  hipLaunchKernelGGL(nrq_ing_scan_kernel, dim3(r.nblk), dim3(256), 0, st, r, c);
  hipLaunchKernelGGL(nrq_ing_classify_kernel, dim3(c.ntiles), dim3(256), 0, st, r, c);
  hipLaunchKernelGGL(nrq_ing_copy_kernel, dim3((n + 3u) / 4u), dim3(256), 0, st, c.pkts, c.pkt_stride, (const uint64_t *)c.dst, n, r.T,
                     ing_payload_off(&c));
  hipLaunchKernelGGL(nrq_ing_fold_kernel, dim3(g), dim3(256), 0, st, r, c);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int nrq_rx_counts(nrq_rx *rx, uint32_t *h_nlost, uint32_t *h_nrep) {
  if (!rx) return -1;
  nrq_ctx *ctx = rx->ctx;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const uint32_t nb = rx->r.nblk;
  if (h_nlost) HIPCHK(ctx, hipMemcpyAsync(h_nlost, rx->r.gaps, nb * 4u, hipMemcpyDeviceToHost, ctx->stream));
  if (h_nrep) HIPCHK(ctx, hipMemcpyAsync(h_nrep, rx->r.nrep, nb * 4u, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return 0;
}

/* the compact lists, downloaded (counts first, then exactly the list bytes) and spread to strided host arrays */
static int rx_fetch_lists(nrq_rx *rx, std::vector<uint32_t> &cnt, std::vector<uint32_t> &lists) {
  nrq_ctx *ctx = rx->ctx;
  const ing_rx &r = rx->r;
  hipLaunchKernelGGL(nrq_ing_lists_kernel, dim3(r.nblk), dim3(256), 0, ctx->stream, r, (uint32_t *)rx->lists);
  HIPCHK(ctx, hipGetLastError());
  cnt.assign(2u * r.nblk, 0);
  HIPCHK(ctx, hipMemcpyAsync(cnt.data(), rx->lists, cnt.size() * 4u, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  size_t total = 0;
  for (uint32_t v : cnt) total += v;
  lists.assign(total ? total : 1, 0);
  if (total) {
    HIPCHK(ctx, hipMemcpyAsync(lists.data(), (uint32_t *)rx->lists + 2u * r.nblk, total * 4u, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  }
  return 0;
}

int nrq_rx_lists(nrq_rx *rx, uint32_t *h_nlost, uint32_t *h_nrep, uint32_t *h_lost, uint32_t *h_rep_esi) {
  if (!rx) return -1;
  nrq_ctx *ctx = rx->ctx;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const ing_rx &r = rx->r;
  std::vector<uint32_t> cnt, lists;
  int rc = rx_fetch_lists(rx, cnt, lists);
  if (rc) return rc;
  size_t off = 0;
  for (uint32_t b = 0; b < r.nblk; b++) {
    const uint32_t ng = cnt[b], nr = cnt[r.nblk + b];
    if (h_nlost) h_nlost[b] = ng;
    if (h_nrep) h_nrep[b] = nr;
    if (h_rep_esi) memcpy(h_rep_esi + (size_t)b * r.rep_cap, lists.data() + off, (size_t)nr * 4u);
    if (h_lost) memcpy(h_lost + (size_t)b * r.K, lists.data() + off + nr, (size_t)ng * 4u);
    off += (size_t)ng + nr;
  }
  return 0;
}

/* The downloaded lists of some receptions' blocks in the host form both decodes read.  Listed block j is block blk[j] of rx[j],
 * which is member[j] of the caller's rxset_plan_member array; it has ng[j] missing source ESIs and nr[j] repair ESIs, and
 * words[off[j] ..] holds the repair ESIs in arrival order, then the missing source ESIs ascending. */
struct rx_listing {
  std::vector<nrq_rx *> rx;
  std::vector<uint32_t> member, blk, ng, nr;
  std::vector<size_t> off;
  std::vector<uint32_t> words;
  void add(nrq_rx *x, uint32_t m, uint32_t b, uint32_t g, uint32_t r, size_t o) {
    rx.push_back(x); member.push_back(m); blk.push_back(b); ng.push_back(g); nr.push_back(r); off.push_back(o);
  }
};

/* The decode of listed blocks, one nrq_decode_blocks_vi per chunk of their rxset_plan.  h_status / h_used of every listed block:
 * status 1 for a block without gaps, 0 and 0 symbols used for one that is not decoded now, else what its decode call says.  With
 * a relay attached to a block's reception the decode also writes the block's intermediate symbols into the relay's buffer (and
 * so back-substitutes all pivots) and the relay learns of every recovered block; without one it asks for none, as
 * nrq_decode_blocks_v.  `recovered`: the listed blocks whose decode succeeded, for the caller's mark launch.  A failing decode
 * call ends it with that call's code and error text: its chunk's and the later chunks' blocks keep status 0 and their books, the
 * chunks before it are in `recovered`. */
static int rx_decode_listed(nrq_ctx *ctx, const rx_listing &L, const std::vector<rxset_chunk> &chunks, int *h_status, uint32_t *h_used,
                            std::vector<uint32_t> &recovered) {
  for (size_t j = 0; j < L.rx.size(); j++) {
    h_status[j] = L.ng[j] == 0 ? 1 : 0;
    if (h_used) h_used[j] = 0;
  }
  std::vector<uint32_t> lost, resi, nlost, nuse, navail, used;
  std::vector<uint64_t> sv, rv, iv;
  std::vector<int> st;
  for (const rxset_chunk &c : chunks) {
    const size_t ns = c.blocks.size();
    uint32_t lost_cap = 1, rep_cap = 1;
    for (uint32_t j : c.blocks) { lost_cap = std::max(lost_cap, L.ng[j]); rep_cap = std::max(rep_cap, L.nr[j]); }
    lost.assign(ns * lost_cap, 0); resi.assign(ns * rep_cap, 0);
    nlost.resize(ns); nuse.resize(ns); navail.resize(ns); used.assign(ns, 0); sv.resize(ns); rv.resize(ns); st.assign(ns, 0);
    iv.resize(c.has_relay ? ns : 0);
    for (size_t i = 0; i < ns; i++) {
      const uint32_t j = c.blocks[i], b = L.blk[j], ng = L.ng[j], nr = L.nr[j];
      const nrq_rx *rx = L.rx[j];
      const ing_rx &r = rx->r;
      const uint32_t *l = L.words.data() + L.off[j];
      memcpy(resi.data() + i * rep_cap, l, (size_t)nr * 4u);
      memcpy(lost.data() + i * lost_cap, l + nr, (size_t)ng * 4u);
      nlost[i] = ng;
      nuse[i] = rxset_nuse(ng, nr);
      navail[i] = nr;
      sv[i] = (uint64_t)(uintptr_t)(r.src + b * r.src_stride);
      rv[i] = (uint64_t)(uintptr_t)(r.rep + b * r.rep_stride);
      if (c.has_relay) iv[i] = relay_inter(rx->relay, rx->relay_seg, b);
    }
    const int rc = nrq_decode_blocks_vi(ctx, c.K, c.Kp, L.rx[c.blocks[0]]->r.T, (uint32_t)ns, sv.data(), lost.data(), nlost.data(), lost_cap,
                                        resi.data(), nuse.data(), navail.data(), rep_cap, rv.data(), c.has_relay ? iv.data() : nullptr,
                                        st.data(), used.data());
    if (rc) return rc;
    for (size_t i = 0; i < ns; i++) {
      const uint32_t j = c.blocks[i];
      const nrq_rx *rx = L.rx[j];
      h_status[j] = st[i];
      if (h_used) h_used[j] = used[i];
      if (!st[i]) continue;
      recovered.push_back(j);
      if (rx->relay) relay_set(rx->relay, rx->relay_b0 + L.blk[j], 1, true);
    }
  }
  return 0;
}

/* a reception decodes as a set of one member: at most 256 blocks, so its selected blocks are one chunk, one decode call */
static_assert(RXSET_CHUNK_BLOCKS >= 256u, "nrq_rx_decode is one decode call over a reception's up to 256 blocks");

int nrq_rx_decode(nrq_rx *rx, int *h_status, uint32_t *h_used) {
  if (!rx) return -1;
  nrq_ctx *ctx = rx->ctx;
  if (!h_status) return fail(ctx, -1, "nrq_rx_decode: h_status is NULL");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const ing_rx &r = rx->r;
  std::vector<uint32_t> cnt;
  rx_listing L;
  int rc = rx_fetch_lists(rx, cnt, L.words);
  if (rc) return rc;
  size_t off = 0;
  for (uint32_t b = 0; b < r.nblk; b++) { /* (the device format has no offsets: the lists lie one behind the other) */
    L.add(rx, 0, b, cnt[b], cnt[r.nblk + b], off);
    off += (size_t)cnt[b] + cnt[r.nblk + b];
  }
  const rxset_plan_member pm{r.K, rx->Kp, r.max_esi, rx->relay ? 1u : 0u};
  std::vector<uint32_t> recovered;
  rc = rx_decode_listed(ctx, L, rxset_plan(&pm, L.member.data(), L.ng.data(), L.nr.data(), r.nblk), h_status, h_used, recovered);
  if (rc) return rc; /* (of the one chunk: no block is marked) */
  if (!recovered.empty()) {
    ing_mask m{};
    for (uint32_t b : recovered) m.w[b >> 5] |= 1u << (b & 31u);
    hipLaunchKernelGGL(nrq_ing_mark_kernel, dim3(r.nblk), dim3(256), 0, ctx->stream, r, m);
    HIPCHK(ctx, hipGetLastError());
  }
  return 0;
}

} /* extern "C" */

/* ================================================ device-resident emit (nrq_tx_* / nrq_otx_*, emit_body.h) ==== */
#define TX_WAVES 4u        /* waves per emit workgroup */
#define TX_BIN_TILE 4096u  /* packets per workgroup of the bucketing passes */

/* (the payload paths TX_V16 .. TX_BYTE and the rule that picks one per call: tx_emit_path, emit_body.h)
 *
 * Shared by every emit kernel -- the plain, held, several-symbol and set forms, each a kernel of its own so that the older ones'
 * instantiations are compiled from the code they always were -- are the bodies that follow: the payload walk (tx_payload, over one
 * symbol or a run of them), the wave-uniform segment base (TX_SEG_BASE) and the held repair row lookup (tx_held_row). */

/* What a payload walk reads, a compile-time choice: the rows of ONE symbol -- the walk is T bytes long and every word takes the
 * one column list -- or a RUN of cnt symbols of one block with consecutive ESIs (syms_body.h), cnt * T bytes long, where the word
 * at byte off takes the list of slot off / T (slot i's list at cols[i], its length in the low byte of ns[i]; T is a multiple of
 * the word: a word lies in one symbol). */
struct tx_one {
  const uint32_t *cols;
  uint32_t n;
  __device__ __forceinline__ uint32_t len(uint32_t T) const { return T; }
  template <typename W>
  __device__ __forceinline__ W word(const uint8_t *__restrict__ base, uint32_t T, uint64_t off) const {
    return tx_gather<W>(base, T, cols, n, off);
  }
};
struct tx_run {
  const uint32_t (*cols)[TX_COLS];
  const uint32_t *ns;
  uint32_t cnt;
  __device__ __forceinline__ uint32_t len(uint32_t T) const { return cnt * T; }
  template <typename W>
  __device__ __forceinline__ W word(const uint8_t *__restrict__ base, uint32_t T, uint64_t off) const {
    const uint32_t o = (uint32_t)off, i = o / T; /* (cnt * T fits 32 bits: the launcher checked) */
    return tx_gather<W>(base, T, cols[i], ns[i] & 0xFFu, o - i * T);
  }
};

/* the packet of `tag` at P: its payload is, word by word, the XOR of the rows `rows` names from base (one wave; a 16/4/1-byte word
 * per lane) */
template <int MODE, class ROWS>
__device__ __forceinline__ void tx_payload(const uint8_t *__restrict__ base, uint32_t T, const ROWS rows, uint32_t tag,
                                           uint8_t *__restrict__ P, uint32_t inl, uint32_t lane) {
  const uint32_t len = rows.len(T);
  if constexpr (MODE == TX_V16) {
    for (uint32_t off = lane * 16u; off < len; off += 64u * 16u)
      *reinterpret_cast<tx_u128 *>(P + off) = rows.template word<tx_u128>(base, T, off);
  } else if constexpr (MODE == TX_V16_SHIFT) {
    /* packet chunk j (bytes 16j .. 16j+15) = payload dwords 4j-1 .. 4j+2: the previous lane's .w (the header for j = 0, the
     * wave's last lane of the previous round for its first lane) whether or not a symbol boundary lies between the two, then
     * this chunk's .x .y .z; the last .w goes to +len */
    const uint32_t nch = len >> 4;
    uint32_t carry = tx_header_word(tag);
    for (uint32_t j0 = 0; j0 < nch; j0 += 64u) {
      const uint32_t j = j0 + lane;
      const bool act = j < nch;
      tx_u128 v{0u, 0u, 0u, 0u};
      if (act) v = rows.template word<tx_u128>(base, T, (uint64_t)j * 16u);
      uint32_t prev = __shfl_up(v.w, 1u);
      if (lane == 0) prev = carry;
      if (act) *reinterpret_cast<tx_u128 *>(P + (uint64_t)j * 16u) = tx_u128{prev, v.x, v.y, v.z};
      if (j == nch - 1u) *reinterpret_cast<uint32_t *>(P + len) = v.w;
      carry = __shfl(v.w, 63);
    }
  } else if constexpr (MODE == TX_DWORD) {
    if (inl && lane == 0) *reinterpret_cast<uint32_t *>(P) = tx_header_word(tag);
    uint8_t *D = P + (inl ? 4u : 0u);
    for (uint32_t off = lane * 4u; off < len; off += 64u * 4u)
      *reinterpret_cast<uint32_t *>(D + off) = rows.template word<uint32_t>(base, T, off);
  } else {
    if (inl && lane < 4u) P[lane] = (uint8_t)(tx_header_word(tag) >> (8u * lane));
    uint8_t *D = P + (inl ? 4u : 0u);
    for (uint32_t off = lane; off < len; off += 64u) D[off] = rows.template word<uint8_t>(base, T, off);
  }
}

/* the rows of a packet of `tag` in segment sg of the kernel's by-value table s, sg wave-uniform: rebuilt from the kernel arguments (a
 * pointer kept in LDS would come back as a generic one: flat loads, and waits that also cover the LDS reads), and only the chosen
 * segment's fields are read (segment 0's base, replaced after a test, costs two dependent argument loads per packet).  MULTI =
 * false: a one-segment table.  A macro: the same select in a function that takes the table by reference, pointer or value makes
 * the compiler index the table with sg, and the multi-segment kernels then copy their arguments to 344 bytes of scratch. */
#define TX_SEG_BASE(MULTI, s, sg, tag) \
  (!(MULTI) || (sg) == 0u ? tx_base(&(s).seg[0], tag) : (sg) == 1u ? tx_base(&(s).seg[1], tag) : tx_base(&(s).seg[2], tag))

/* the repair row of block b of a reception that holds ESI `esi`, or TX_NONE: each lane probes one entry of the block's repair list
 * per trip (64 consecutive entries, one coalesced load), a ballot gives the wave-uniform row (tx_held_find, a wave at a time) */
__device__ __forceinline__ uint32_t tx_held_row(const tx_held_seg *hs, uint32_t b, uint32_t esi, uint32_t lane) {
  const uint32_t nrep = tx_held_nrep(hs, b);
  uint32_t q = TX_NONE;
  for (uint32_t q0 = 0; q0 < nrep && q == TX_NONE; q0 += 64u) {
    const uint64_t m = __ballot(tx_held_hit(hs, b, q0 + lane, nrep, esi));
    if (m) q = q0 + (uint32_t)__ffsll((unsigned long long)m) - 1u;
  }
  return q;
}

/* One wave per TX_WAVE_PKTS work items, in block-major order: each lane builds the column list of one item into LDS, then the
 * wave writes the items' packets one after the other, a 16/4/1-byte word of the payload per lane (the XOR of the item's rows,
 * four rows in flight).  Each packet's rows come from the table segment of its SBN; MULTI = false is the form for a one-segment
 * table (no segment search, no select, no segment index in LDS). */
template <int MODE, bool MULTI>
__global__ __launch_bounds__(256) void nrq_emit_kernel(tx_src s, tx_call c) {
  __shared__ uint32_t s_cols[TX_WAVES][TX_WAVE_PKTS][TX_COLS];
  __shared__ uint32_t s_n[TX_WAVES][TX_WAVE_PKTS], s_tag[TX_WAVES][TX_WAVE_PKTS], s_k[TX_WAVES][TX_WAVE_PKTS];
  __shared__ uint32_t s_seg[TX_WAVES][TX_WAVE_PKTS]; /* (MULTI only: unused LDS is not allocated) */
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint64_t w0 = ((uint64_t)blockIdx.x * TX_WAVES + wv) * TX_WAVE_PKTS;
  if (w0 + lane < c.n) {
    const uint32_t k = tx_packet_of<MULTI>(&s, &c, (uint32_t)(w0 + lane));
    const uint32_t tag = k < c.n ? tx_tag_of<MULTI>(&s, &c, k) : 0u;
    int32_t code = TX_FOREIGN;
    const uint32_t sg = k < c.n ? tx_admit<MULTI>(&s, tag, &code) : TX_SEGS; /* (k < n always: the work order is a permutation) */
    const tx_blk sb = MULTI ? tx_pick(&s, sg) : s.seg[0];
    const uint32_t n = sg < TX_SEGS ? tx_rows(&sb, tag, s_cols[wv][lane]) : 0u;
    s_n[wv][lane] = n;
    s_tag[wv][lane] = tag;
    s_k[wv][lane] = k;
    if (MULTI) s_seg[wv][lane] = sg;
    if (k < c.n && c.results) c.results[k] = code;
    if (k < c.n && c.tags_out) c.tags_out[k] = tag;
  }
  __syncthreads();
  const uint32_t cnt = w0 >= c.n ? 0u : (uint32_t)min((uint64_t)TX_WAVE_PKTS, c.n - w0);
  const uint32_t T = s.seg[0].T;
  for (uint32_t i = 0; i < cnt; i++) { /* (wave-uniform) */
    const uint32_t n = s_n[wv][i];
    if (!n) continue; /* SBN outside the span, or a block that is not ready: the packet stays untouched */
    const uint32_t tag = s_tag[wv][i];
    const uint32_t sg = MULTI ? __builtin_amdgcn_readfirstlane(s_seg[wv][i]) : 0u;
    tx_payload<MODE>(TX_SEG_BASE(MULTI, s, sg, tag), T, tx_one{s_cols[wv][i], n}, tag, c.pkts + (uint64_t)s_k[wv][i] * c.pkt_stride, c.inl,
                     lane);
  }
}

/* The emit kernel with held symbols (NRQ_TX_HELD; relays only, a tag list only): as nrq_emit_kernel, but a packet of a block that is
 * not ready is still written when the reception holds its symbol (tx_admit_held) -- a copy of the source row, or of the repair
 * row whose ESI it is.  That row is found by the wave that writes the packet (tx_held_row).  A kernel of its own, so that the
 * plain emit's instantiations are compiled from the code they always were. */
template <int MODE, bool MULTI>
__global__ __launch_bounds__(256) void nrq_emit_held_kernel(tx_src s, tx_held h, tx_call c) {
  __shared__ uint32_t s_cols[TX_WAVES][TX_WAVE_PKTS][TX_COLS];
  __shared__ uint32_t s_n[TX_WAVES][TX_WAVE_PKTS], s_tag[TX_WAVES][TX_WAVE_PKTS], s_k[TX_WAVES][TX_WAVE_PKTS];
  __shared__ uint32_t s_seg[TX_WAVES][TX_WAVE_PKTS]; /* (MULTI only: unused LDS is not allocated) */
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint64_t w0 = ((uint64_t)blockIdx.x * TX_WAVES + wv) * TX_WAVE_PKTS;
  if (w0 + lane < c.n) {
    const uint32_t k = tx_packet_of<MULTI>(&s, &c, (uint32_t)(w0 + lane));
    const uint32_t tag = k < c.n ? tx_tag_of<MULTI>(&s, &c, k) : 0u;
    int32_t code = TX_FOREIGN;
    uint32_t kind = TX_READY;
    const uint32_t sg = k < c.n ? tx_admit_held<MULTI>(&s, &h, tag, &code, &kind) : TX_SEGS;
    const tx_blk sb = MULTI ? tx_pick(&s, sg) : s.seg[0];
    uint32_t n = 0;
    if (sg < TX_SEGS) {
      if (kind == TX_HELD_REP) { s_cols[wv][lane][0] = 0u; n = 1u; } /* (row 0 from the base of the row found below) */
      else n = tx_rows(&sb, tag, s_cols[wv][lane]);
    }
    s_n[wv][lane] = n | (kind << 8);
    s_tag[wv][lane] = tag;
    s_k[wv][lane] = k;
    if (MULTI) s_seg[wv][lane] = sg;
    if (k < c.n && c.results && kind != TX_HELD_REP) c.results[k] = code; /* (a held repair packet's: once its row is found) */
  }
  __syncthreads();
  const uint32_t cnt = w0 >= c.n ? 0u : (uint32_t)min((uint64_t)TX_WAVE_PKTS, c.n - w0);
  const uint32_t T = s.seg[0].T;
  for (uint32_t i = 0; i < cnt; i++) { /* (wave-uniform) */
    const uint32_t nk = __builtin_amdgcn_readfirstlane(s_n[wv][i]), n = nk & 0xFFu;
    if (!n) continue; /* SBN outside the span, or a symbol of a block that is not ready which the reception does not hold */
    const uint32_t tag = __builtin_amdgcn_readfirstlane(s_tag[wv][i]);
    const uint32_t sg = MULTI ? __builtin_amdgcn_readfirstlane(s_seg[wv][i]) : 0u;
    const uint8_t *base;
    if ((nk >> 8) == TX_HELD_REP) {
      const tx_held_seg hs = sg == 0u ? h.seg[0] : sg == 1u ? h.seg[1] : h.seg[2];
      const uint32_t b = (tag >> 24) - (sg == 0u ? s.seg[0].sbn0 : sg == 1u ? s.seg[1].sbn0 : s.seg[2].sbn0);
      const uint32_t q = tx_held_row(&hs, b, tag & 0xFFFFFFu, lane);
      if (c.results && lane == 0) c.results[s_k[wv][i]] = q == TX_NONE ? TX_NOT_READY : 0;
      if (q == TX_NONE) continue; /* (the books say otherwise: a marked repair ESI has its row) */
      base = tx_held_rep_base(&hs, b) + (uint64_t)q * T;
    } else {
      base = TX_SEG_BASE(MULTI, s, sg, tag);
    }
    tx_payload<MODE>(base, T, tx_one{s_cols[wv][i], n}, tag, c.pkts + (uint64_t)s_k[wv][i] * c.pkt_stride, c.inl, lane);
  }
}

/* tag-list bucketing over the span of nblk blocks from sbn0: packets per bucket (tx_bin), a histogram in LDS per tile of
 * TX_BIN_TILE packets, added to cnt[] */
__global__ __launch_bounds__(256) void nrq_tx_hist_kernel(uint32_t sbn0, uint32_t nblk, const uint32_t *tags, uint32_t n, uint32_t *cnt) {
  __shared__ uint32_t h[257];
  for (uint32_t i = threadIdx.x; i <= nblk; i += 256u) h[i] = 0;
  __syncthreads();
  const uint32_t k0 = blockIdx.x * TX_BIN_TILE, k1 = min(n, k0 + TX_BIN_TILE);
  for (uint32_t k = k0 + threadIdx.x; k < k1; k += 256u) atomicAdd(&h[tx_bin(sbn0, nblk, tags[k])], 1u);
  __syncthreads();
  for (uint32_t i = threadIdx.x; i <= nblk; i += 256u)
    if (h[i]) atomicAdd(&cnt[i], h[i]);
}

/* counts -> exclusive offsets, in place (nblk + 1 <= 257 buckets: one lane) */
__global__ __launch_bounds__(64) void nrq_tx_scan_kernel(uint32_t nbins, uint32_t *cnt) {
  if (threadIdx.x) return;
  uint32_t run = 0;
  for (uint32_t i = 0; i < nbins; i++) { const uint32_t v = cnt[i]; cnt[i] = run; run += v; }
}

/* each tile reserves its packets' places in every bucket (one atomic per bucket and tile), then writes order[] */
__global__ __launch_bounds__(256) void nrq_tx_place_kernel(uint32_t sbn0, uint32_t nblk, const uint32_t *tags, uint32_t n, uint32_t *cursor,
                                                           uint32_t *order) {
  __shared__ uint32_t h[257], base[257];
  constexpr uint32_t PER = TX_BIN_TILE / 256u;
  for (uint32_t i = threadIdx.x; i <= nblk; i += 256u) h[i] = 0;
  __syncthreads();
  const uint32_t k0 = blockIdx.x * TX_BIN_TILE;
  uint32_t bin[PER], rank[PER];
#pragma unroll
  for (uint32_t r = 0; r < PER; r++) {
    const uint32_t k = k0 + r * 256u + threadIdx.x;
    bin[r] = k < n ? tx_bin(sbn0, nblk, tags[k]) : TX_NONE;
    rank[r] = bin[r] != TX_NONE ? atomicAdd(&h[bin[r]], 1u) : 0u;
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i <= nblk; i += 256u) base[i] = h[i] ? atomicAdd(&cursor[i], h[i]) : 0u;
  __syncthreads();
#pragma unroll
  for (uint32_t r = 0; r < PER; r++)
    if (bin[r] != TX_NONE) order[base[bin[r]] + rank[r]] = k0 + r * 256u + threadIdx.x;
}

/* what both senders are: an emit source and the device buffers behind it.  nrq_tx and nrq_otx (distinct in the header) are this
 * plus, for an object, its parameters; their create calls fill it, everything after that is shared. */
struct tx_sender {
  nrq_ctx *ctx;
  tx_src s;
  void *own[2];          /* device buffers it owns: the intermediate symbols; an object's row images or staged last block */
  bool encoded;
  const char *unencoded; /* the emit calls' refusal before the encode */
  DevScratch scratch;    /* list mode: bucket counts, then the work order */
  /* A relay (nrq_rx_relay / nrq_orx_relay): segment g's source rows are those of the reception from[g], and s.ready has the bit
   * of every block whose intermediate symbols are written -- by a decode of the reception while the relay was attached, or by
   * the relay's encode for a block that is complete (only complete blocks ever get the bit: ready = complete and written). */
  bool relay, detached;  /* detached: a reception was destroyed first; every later call fails */
  nrq_rx *from[2];
  struct nrq_txset *set; /* the sender set this transmission is a member of (nrq_txset_attach), or null */
};
static void txset_drop(tx_sender *tx); /* a member of a sender set goes away (defined with the sets below) */

struct nrq_tx : tx_sender {};

static uint64_t relay_inter(const tx_sender *tx, uint32_t seg, uint32_t b) {
  const tx_blk &t = tx->s.seg[seg];
  return (uint64_t)(uintptr_t)(t.inter + (uint64_t)b * t.inter_stride);
}

static void relay_set(tx_sender *tx, uint32_t b0, uint32_t nblk, bool valid) {
  for (uint32_t b = b0; b < b0 + nblk; b++) {
    if (valid) tx->s.ready[b >> 5] |= 1u << (b & 31u);
    else tx->s.ready[b >> 5] &= ~(1u << (b & 31u));
  }
}

static bool tx_is_ready(const tx_sender *tx, uint32_t b) { return (tx->s.ready[b >> 5] >> (b & 31u)) & 1u; }

static void relay_detach(tx_sender *tx) {
  for (nrq_rx *&r : tx->from) {
    if (r) r->relay = nullptr;
    r = nullptr;
  }
  tx->detached = true;
  memset(tx->s.ready, 0, sizeof(tx->s.ready));
}

template <class S>
static void tx_destroy(S *tx) {
  if (!tx) return;
  nrq_ctx *ctx = tx->ctx;
  if (tx->set) txset_drop(tx); /* (the set's table is rewritten without it, behind the work enqueued so far) */
  for (nrq_rx *r : tx->from)
    if (r) r->relay = nullptr;
  (void)hipStreamSynchronize(ctx->stream); /* (the pool hands freed blocks out again at once) */
  for (void *p : {tx->own[0], tx->own[1]})
    if (p) nrq_dev_free(ctx, p);
  tx->scratch.release(ctx);
  delete tx;
}

/* a relay's blocks that are not ready, as a text ("3, 7, 9 ... (12 of 256)") */
static std::string relay_missing(const tx_sender *tx) {
  std::string out;
  uint32_t n = 0;
  for (uint32_t b = 0; b < tx->s.Z; b++) {
    if (tx_is_ready(tx, b)) continue;
    if (n < 8u) out += (n ? ", " : "") + std::to_string(tx->s.sbn0 + b);
    n++;
  }
  if (n > 8u) out += " ...";
  return out + " (" + std::to_string(n) + " of " + std::to_string(tx->s.Z) + ")";
}

/* a relay's encode: every block that is complete in its reception but has no intermediate symbols yet -- nothing was missing,
 * or it was decoded before the relay was attached -- is solved with the encoder, from the reception's rows; the blocks that are
 * ready are left alone (no launch at all when there is nothing to do).  Waits for the receptions' counts. */
static int relay_encode(tx_sender *tx) {
  nrq_ctx *ctx = tx->ctx;
  for (uint32_t g = 0; g < tx->s.nseg; g++) {
    const tx_blk &t = tx->s.seg[g];
    nrq_rx *rx = tx->from[g];
    std::vector<uint32_t> gaps(t.nblk, 0);
    int rc = nrq_rx_counts(rx, gaps.data(), nullptr);
    if (rc) return rc;
    std::vector<uint32_t> todo;
    std::vector<uint64_t> sv, iv;
    for (uint32_t b = 0; b < t.nblk; b++) {
      if (gaps[b] || tx_is_ready(tx, rx->relay_b0 + b)) continue;
      todo.push_back(b);
      sv.push_back((uint64_t)(uintptr_t)(t.src + (uint64_t)b * t.src_stride));
      iv.push_back(relay_inter(tx, g, b));
    }
    if (todo.empty()) continue;
    rc = encode_blocks(ctx, t.K, t.p.Kp, t.T, (uint32_t)todo.size(), Rows{nullptr, 0, sv.data()}, Rows{nullptr, 0, iv.data()}, 0, nullptr,
                       Rows{});
    if (rc) return rc;
    for (uint32_t b : todo) relay_set(tx, rx->relay_b0 + b, 1, true);
  }
  return 0;
}

/* solve every block of every segment */
static int tx_encode(tx_sender *tx) {
  if (!tx) return -1;
  if (tx->detached) return fail(tx->ctx, -1, "the relay's reception was destroyed");
  if (tx->relay) return relay_encode(tx);
  tx->encoded = false;
  for (uint32_t g = 0; g < tx->s.nseg; g++) {
    const tx_blk &t = tx->s.seg[g];
    const int rc = nrq_encode_blocks(tx->ctx, t.K, t.p.Kp, t.T, t.nblk, t.src, t.src_stride, (void *)t.inter, t.inter_stride, 0, nullptr,
                                     nullptr, 0);
    if (rc) return rc;
  }
  tx->encoded = true;
  return 0;
}

/* checks shared by every emit call; list: the tag-list form, which alone takes NRQ_TX_HELD, and only on a relay */
static int tx_check(tx_sender *tx, const char *who, const void *d_pkts, size_t pkt_stride, uint32_t flags, bool list = false) {
  nrq_ctx *ctx = tx->ctx;
  if (tx->detached) return fail(ctx, -1, "%s: the relay's reception was destroyed", who);
  if (!tx->encoded) return fail(ctx, -1, "%s: %s", who, tx->unencoded);
  if (flags & ~(uint32_t)(NRQ_TX_TAG_INLINE | NRQ_TX_HELD)) return fail(ctx, -1, "%s: unknown flags 0x%x", who, flags);
  if ((flags & NRQ_TX_HELD) && !list) return fail(ctx, -1, "%s: NRQ_TX_HELD goes with a tag list (the range forms map packets to every block)", who);
  if ((flags & NRQ_TX_HELD) && !tx->relay) return fail(ctx, -1, "%s: NRQ_TX_HELD needs a relay (a sender holds no reception)", who);
  if (!d_pkts) return fail(ctx, -1, "%s: d_pkts is NULL", who);
  const bool inl = (flags & NRQ_TX_TAG_INLINE) != 0;
  if (pkt_stride < (size_t)tx->s.seg[0].T + (inl ? 4u : 0u)) return fail(ctx, -1, "%s: pkt_stride %zu shorter than a packet", who, pkt_stride);
  return 0;
}

/* the table beside a relay's source table: per segment the books of the reception it reads (tx_held, emit_body.h) */
static tx_held tx_held_table(const tx_sender *tx) {
  tx_held h{};
  for (uint32_t g = 0; g < tx->s.nseg; g++) {
    const ing_rx &r = tx->from[g]->r;
    tx_held_seg &t = h.seg[g];
    t.seen = r.seen; t.bm_words = r.bm_words;
    t.rep_esi = r.rep_esi; t.nrep = r.nrep; t.rep_cap = r.rep_cap;
    t.rep = r.rep; t.rep_stride = r.rep_stride;
  }
  return h;
}

/* the emit kernel at the widest path the addresses allow, in its one-segment form for a one-segment table; held: the kernel that
 * also answers from the symbols the relay's receptions hold */
static int tx_launch(tx_sender *tx, const tx_call &c, bool held = false) {
  using emit_fn = void (*)(tx_src, tx_call);
  using held_fn = void (*)(tx_src, tx_held, tx_call);
  static const held_fn hkern[2][4] = { /* [multi-segment][mode] */
      {nrq_emit_held_kernel<TX_V16, false>, nrq_emit_held_kernel<TX_V16_SHIFT, false>, nrq_emit_held_kernel<TX_DWORD, false>,
       nrq_emit_held_kernel<TX_BYTE, false>},
      {nrq_emit_held_kernel<TX_V16, true>, nrq_emit_held_kernel<TX_V16_SHIFT, true>, nrq_emit_held_kernel<TX_DWORD, true>,
       nrq_emit_held_kernel<TX_BYTE, true>}};
  static const emit_fn kern[2][4] = { /* [multi-segment][mode] */
      {nrq_emit_kernel<TX_V16, false>, nrq_emit_kernel<TX_V16_SHIFT, false>, nrq_emit_kernel<TX_DWORD, false>,
       nrq_emit_kernel<TX_BYTE, false>},
      {nrq_emit_kernel<TX_V16, true>, nrq_emit_kernel<TX_V16_SHIFT, true>, nrq_emit_kernel<TX_DWORD, true>,
       nrq_emit_kernel<TX_BYTE, true>}};
  nrq_ctx *ctx = tx->ctx;
  const tx_src &s = tx->s;
  const tx_held h = held ? tx_held_table(tx) : tx_held{};
  const int mode = tx_emit_path(tx_align(&s, &c, held ? &h : nullptr), c.inl, ctx->tune.tx_dword ? 1u : 0u);
  const dim3 grid((c.n + TX_WAVES * TX_WAVE_PKTS - 1u) / (TX_WAVES * TX_WAVE_PKTS)), wg(64u * TX_WAVES);
  if (held) hipLaunchKernelGGL(hkern[s.nseg > 1u][mode], grid, wg, 0, ctx->stream, s, h, c);
  else hipLaunchKernelGGL(kern[s.nseg > 1u][mode], grid, wg, 0, ctx->stream, s, c);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

/* a call's packet buffer: n packets at d_pkts, the header form of `flags` */
static tx_call tx_call_of(void *d_pkts, size_t pkt_stride, uint32_t n, uint32_t flags) {
  tx_call c{};
  c.pkts = (uint8_t *)d_pkts;
  c.pkt_stride = pkt_stride;
  c.n = n;
  c.inl = (flags & NRQ_TX_TAG_INLINE) ? 1u : 0u;
  return c;
}

/* list mode: the n tags bucketed by block of the span into the sender's scratch -- bucket counts, then the work order *order */
static int tx_bucket(tx_sender *tx, const uint32_t *d_tags, uint32_t n, const uint32_t **order) {
  nrq_ctx *ctx = tx->ctx;
  const uint32_t sbn0 = tx->s.sbn0, nblk = tx->s.Z, nbins = nblk + 1u;
  const size_t o_order = rx_al((size_t)nbins * 4u), need = o_order + rx_al((size_t)n * 4u);
  const int rc = tx->scratch.ensure(ctx, need);
  if (rc) return rc;
  uint32_t *cnt = (uint32_t *)tx->scratch.p, *ord = (uint32_t *)((uint8_t *)tx->scratch.p + o_order);
  hipStream_t st = ctx->stream;
  const uint32_t tiles = (n + TX_BIN_TILE - 1u) / TX_BIN_TILE;
  HIPCHK(ctx, hipMemsetAsync(cnt, 0, (size_t)nbins * 4u, st));
  hipLaunchKernelGGL(nrq_tx_hist_kernel, dim3(tiles), dim3(256), 0, st, sbn0, nblk, d_tags, n, cnt);
  hipLaunchKernelGGL(nrq_tx_scan_kernel, dim3(1), dim3(64), 0, st, nbins, cnt);
  hipLaunchKernelGGL(nrq_tx_place_kernel, dim3(tiles), dim3(256), 0, st, sbn0, nblk, d_tags, n, cnt, ord);
  HIPCHK(ctx, hipGetLastError());
  *order = ord;
  return 0;
}

/* range mode on a relay: every block of the span must be ready (the packet maps are analytic over all blocks: no holes) */
static int tx_span_ready(tx_sender *tx, const char *who) {
  if (tx->relay)
    for (uint32_t b = 0; b < tx->s.Z; b++)
      if (!tx_is_ready(tx, b)) return fail(tx->ctx, -1, "%s: blocks of the relay are not ready: SBN %s", who, relay_missing(tx).c_str());
  return 0;
}

/* range mode: the packet order a caller asks for */
static int tx_check_order(tx_sender *tx, const char *who, int order) {
  if (order != 0 && order != 1) return fail(tx->ctx, -1, "%s: order %d is neither 0 (block-major) nor 1 (interleaved)", who, order);
  return 0;
}

/* list mode: the tags bucketed by block of the span into the scratch's work order, then the emit */
static int tx_emit_list(tx_sender *tx, const char *who, const uint32_t *d_tags, uint32_t n, void *d_pkts, size_t pkt_stride, uint32_t flags,
                        int32_t *d_results) {
  if (!tx) return -1;
  nrq_ctx *ctx = tx->ctx;
  int rc = tx_check(tx, who, d_pkts, pkt_stride, flags, true);
  if (rc) return rc;
  if (n == 0) return 0;
  if (!d_tags || n > 0x7FFFFFFFu) return fail(ctx, -1, "%s: bad tags (n=%u)", who, n);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  tx_call c = tx_call_of(d_pkts, pkt_stride, n, flags);
  if ((rc = tx_bucket(tx, d_tags, n, &c.order))) return rc;
  c.tags = d_tags;
  c.results = d_results;
  return tx_launch(tx, c, (flags & NRQ_TX_HELD) != 0);
}

/* range mode (the caller has checked its arguments): ESIs esi0 .. esi0+nL-1 of each of the span's first ZL blocks, esi0 ..
 * esi0+nS-1 of the rest, block-major (order 0) or interleaved (1) */
static int tx_emit_span(tx_sender *tx, const char *who, uint32_t esi0, uint32_t nL, uint32_t nS, int order, void *d_pkts, size_t pkt_stride,
                        uint32_t flags, uint32_t *d_tags_out) {
  nrq_ctx *ctx = tx->ctx;
  const int rc = tx_span_ready(tx, who);
  if (rc) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  tx_call c = tx_call_of(d_pkts, pkt_stride, tx->s.ZL * nL + (tx->s.Z - tx->s.ZL) * nS, flags);
  c.esi0 = esi0;
  c.nL = tx->s.ZL ? nL : nS; /* (a table of one class has nL packets per block: the one-segment maps) */
  c.nS = nS;
  c.interleave = (uint32_t)order;
  c.tags_out = d_tags_out;
  return tx_launch(tx, c);
}

extern "C" {

int nrq_tx_create(nrq_ctx *ctx, uint32_t K, uint32_t Kp, uint32_t T, uint32_t nblk, uint32_t sbn0, const void *d_src, size_t src_stride,
                  nrq_tx **out) {
  if (!ctx) return -1;
  if (!out) return fail(ctx, -1, "nrq_tx_create: out is NULL");
  *out = nullptr;
  uint32_t prm[10];
  if (nrq_params(K, prm) != 0) return fail(ctx, -1, "nrq_tx_create: K=%u out of range", K);
  if (Kp == 0) Kp = prm[0];
  if (Kp < prm[0] || nrq_params(Kp, prm) != 0 || prm[0] != Kp) return fail(ctx, -1, "nrq_tx_create: K'=%u is not a table row for K=%u", Kp, K);
  if (T == 0 || nblk == 0 || nblk > 256u || sbn0 + nblk > 256u) return fail(ctx, -1, "nrq_tx_create: bad T / nblk / sbn0 (%u %u %u)", T, nblk, sbn0);
  if (!d_src) return fail(ctx, -1, "nrq_tx_create: d_src is NULL");
  if (src_stride == 0) src_stride = (size_t)K * T;
  if (src_stride < (size_t)K * T) return fail(ctx, -1, "nrq_tx_create: src_stride %zu shorter than a block", src_stride);
  nrq_tx *tx = new (std::nothrow) nrq_tx();
  if (!tx) return fail(ctx, -1, "nrq_tx_create: out of host memory");
  tx->ctx = ctx;
  tx->unencoded = "the transmission is not encoded (nrq_tx_encode)";
  tx->s.nseg = 1;
  tx->s.sbn0 = sbn0; tx->s.Z = tx->s.ZL = nblk;
  memset(tx->s.ready, 0xFF, sizeof(tx->s.ready));
  tx_blk &t = tx->s.seg[0];
  int rc = block_params(ctx, K, Kp, &t.p);
  if (rc) { delete tx; return rc; }
  t.K = K; t.T = T; t.nblk = nblk; t.sbn0 = sbn0;
  t.src = (const uint8_t *)d_src; t.src_stride = src_stride;
  t.inter_stride = (uint64_t)t.p.L * T;
  if ((rc = nrq_dev_alloc(ctx, (size_t)nblk * t.inter_stride, &tx->own[0]))) {
    delete tx;
    return rc;
  }
  t.inter = (const uint8_t *)tx->own[0];
  *out = tx;
  return 0;
}

void nrq_tx_destroy(nrq_tx *tx) { tx_destroy(tx); }

int nrq_tx_encode(nrq_tx *tx) { return tx_encode(tx); }

void *nrq_tx_inter(nrq_tx *tx) { return tx ? (void *)tx->s.seg[0].inter : nullptr; }

static int tx_ready(tx_sender *tx, const char *who, uint32_t *h_ready) {
  if (!tx) return -1;
  if (tx->detached) return fail(tx->ctx, -1, "%s: the relay's reception was destroyed", who);
  if (!h_ready) return fail(tx->ctx, -1, "%s: h_ready is NULL", who);
  for (uint32_t b = 0; b < tx->s.Z; b++) h_ready[b] = tx->relay ? tx_is_ready(tx, b) : tx->encoded;
  return 0;
}

int nrq_tx_ready(nrq_tx *tx, uint32_t *h_ready) { return tx_ready(tx, "nrq_tx_ready", h_ready); }

int nrq_rx_relay(nrq_rx *rx, nrq_tx **out) {
  if (!rx) return -1;
  nrq_ctx *ctx = rx->ctx;
  if (!out) return fail(ctx, -1, "nrq_rx_relay: out is NULL");
  *out = nullptr;
  if (rx->relay) return fail(ctx, -1, "nrq_rx_relay: the reception has a relay already");
  const ing_rx &r = rx->r;
  nrq_tx *tx = new (std::nothrow) nrq_tx();
  if (!tx) return fail(ctx, -1, "nrq_rx_relay: out of host memory");
  tx->ctx = ctx;
  tx->relay = tx->encoded = true; /* (a relay is never "not encoded": its blocks are ready or not, one by one) */
  tx->unencoded = "";
  tx->s.nseg = 1;
  tx->s.sbn0 = r.sbn0; tx->s.Z = tx->s.ZL = r.nblk;
  tx_blk &t = tx->s.seg[0];
  int rc = block_params(ctx, r.K, rx->Kp, &t.p);
  if (rc) { delete tx; return rc; }
  t.K = r.K; t.T = r.T; t.nblk = r.nblk; t.sbn0 = r.sbn0;
  t.src = r.src; t.src_stride = r.src_stride; /* the reception's rows, in place */
  t.inter_stride = (uint64_t)t.p.L * r.T;
  if ((rc = nrq_dev_alloc(ctx, (size_t)r.nblk * t.inter_stride, &tx->own[0]))) {
    delete tx;
    return rc;
  }
  t.inter = (const uint8_t *)tx->own[0];
  tx->from[0] = rx;
  rx->relay = tx; rx->relay_seg = 0; rx->relay_b0 = 0;
  *out = tx;
  return 0;
}

int nrq_tx_emit(nrq_tx *tx, const uint32_t *d_tags, uint32_t n, void *d_pkts, size_t pkt_stride, uint32_t flags, int32_t *d_results) {
  return tx_emit_list(tx, "nrq_tx_emit", d_tags, n, d_pkts, pkt_stride, flags, d_results);
}

int nrq_tx_emit_range(nrq_tx *tx, uint32_t esi0, uint32_t n, int order, void *d_pkts, size_t pkt_stride, uint32_t flags, uint32_t *d_tags_out) {
  if (!tx) return -1;
  nrq_ctx *ctx = tx->ctx;
  int rc = tx_check(tx, "nrq_tx_emit_range", d_pkts, pkt_stride, flags);
  if (rc) return rc;
  if ((rc = tx_check_order(tx, "nrq_tx_emit_range", order))) return rc;
  if (n == 0) return 0;
  if (esi0 >= (1u << 24) || n > (1u << 24) - esi0) return fail(ctx, -1, "nrq_tx_emit_range: ESIs %u + %u reach past 2^24", esi0, n);
  if ((uint64_t)n * tx->s.Z > 0x7FFFFFFFu) return fail(ctx, -1, "nrq_tx_emit_range: %u packets per block is too many", n);
  return tx_emit_span(tx, "nrq_tx_emit_range", esi0, n, n, order, d_pkts, pkt_stride, flags, d_tags_out);
}

} /* extern "C" */

/* ================================================ whole objects on the device (nrq_otx_* / nrq_orx_*, obj_body.h) ==== */
/* the object <-> row-image layout: blockIdx.y = block, OBJ_UNROLL windows of 16 bytes per work item */
template <typename W>
__global__ __launch_bounds__(OBJ_WG) void nrq_obj_layout_kernel(obj_lay l) {
  const uint32_t b = blockIdx.y;
  uint32_t mw = 0; /* (the mask word picked by value: no dynamic index into the kernel arguments) */
#pragma unroll
  for (uint32_t i = 0; i < 8u; i++) mw = i == (b >> 5) ? l.mask[i] : mw;
  if (l.to_obj && !((mw >> (b & 31u)) & 1u)) return;
  obj_move<W>(&l, b, blockIdx.x * (OBJ_WG * OBJ_UNROLL) + threadIdx.x, OBJ_WG);
}

/* the two RFC 6330 section 4.4.1.2 partitions: Partition[Kt, Z] = (KL, KS, ZL, ZS) and Partition[T / Al, N] = (TL, TS, NL, NS) / Al
 * (the emit_all index maps rely on KL = KS + 1 when ZL > 0) */
static bool obj_partition_ok(const nrq_obj_params *p) {
  if (p->Z == 0 || p->N == 0 || p->Al == 0 || p->T % p->Al) return false;
  auto part = [](uint32_t I, uint32_t J, uint32_t &IL, uint32_t &IS, uint32_t &JL, uint32_t &JS) {
    IS = I / J; JL = I - IS * J; JS = J - JL; IL = JL ? IS + 1u : 0u;
  };
  uint32_t IL, IS, JL, JS;
  part(p->Kt, p->Z, IL, IS, JL, JS);
  if (IL != p->KL || IS != p->KS || JL != p->ZL || JS != p->ZS) return false;
  part(p->T / p->Al, p->N, IL, IS, JL, JS);
  return IL * p->Al == p->TL && IS * p->Al == p->TS && JL == p->NL && JS == p->NS;
}

/* the consistency a parameter set from nrq_obj_params_* has (a hand-made one is refused before it can send a kernel astray) */
static int obj_check(nrq_ctx *ctx, const char *who, const nrq_obj_params *p) {
  if (!p) return fail(ctx, -1, "%s: params is NULL", who);
  uint32_t pr[10];
  const bool rowL = p->ZL == 0 || (p->KL && nrq_params(p->KpL, pr) == 0 && pr[0] == p->KpL && p->KpL >= p->KL);
  const bool rowS = p->ZS == 0 || (p->KS && nrq_params(p->KpS, pr) == 0 && pr[0] == p->KpS && p->KpS >= p->KS);
  if (p->Z == 0 || p->Z > 256u || p->ZL + p->ZS != p->Z || p->T == 0 || p->Kt == 0 ||
      (uint64_t)p->ZL * p->KL + (uint64_t)p->ZS * p->KS != p->Kt || p->NL + p->NS != p->N || p->TS == 0 ||
      (uint64_t)p->NL * p->TL + (uint64_t)p->NS * p->TS != p->T || p->F == 0 || p->F > (uint64_t)p->Kt * p->T ||
      p->F <= (uint64_t)(p->Kt - 1u) * p->T || !rowL || !rowS || (uint64_t)std::max(p->KL, p->KS) * p->T > 0xFFFFFFFFull ||
      p->max_esi < std::max(p->KpL, p->KpS) || p->max_esi >= (1u << 24) || !obj_partition_ok(p))
    return fail(ctx, -1, "%s: inconsistent object parameters (use nrq_obj_params_enc / _oti)", who);
  return 0;
}

static obj_lay obj_lay_of(const nrq_obj_params *p, void *obj, void *rows, uint32_t to_obj) {
  obj_lay l{};
  l.obj = (uint8_t *)obj; l.rows = (uint8_t *)rows; l.F = p->F;
  l.T = p->T; l.Z = p->Z; l.ZL = p->ZL; l.KL = p->KL; l.KS = p->KS;
  l.NL = p->NL; l.TL = p->TL; l.NS = p->NS; l.TS = p->TS;
  l.to_obj = to_obj;
  l.obj_vec = (reinterpret_cast<uintptr_t>(obj) & 15u) == 0;
  for (uint32_t &w : l.mask) w = 0xFFFFFFFFu;
  return l;
}

/* enqueue the layout kernel at the widest piece width the shape allows */
static int obj_layout_launch(nrq_ctx *ctx, const obj_lay &l) {
  uint32_t maxw = 0;
  for (uint32_t b = 0; b < l.Z; b++) maxw = std::max(maxw, obj_windows(&l, b));
  const dim3 grid((maxw + OBJ_WG * OBJ_UNROLL - 1u) / (OBJ_WG * OBJ_UNROLL), l.Z), wg(OBJ_WG);
  switch (obj_width(&l)) {
    case 16: hipLaunchKernelGGL(nrq_obj_layout_kernel<tx_u128>, grid, wg, 0, ctx->stream, l); break;
    case 8: hipLaunchKernelGGL(nrq_obj_layout_kernel<uint64_t>, grid, wg, 0, ctx->stream, l); break;
    case 4: hipLaunchKernelGGL(nrq_obj_layout_kernel<uint32_t>, grid, wg, 0, ctx->stream, l); break;
    case 2: hipLaunchKernelGGL(nrq_obj_layout_kernel<uint16_t>, grid, wg, 0, ctx->stream, l); break;
    default: hipLaunchKernelGGL(nrq_obj_layout_kernel<uint8_t>, grid, wg, 0, ctx->stream, l); break;
  }
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

/* the receiver's code for packets of SBN >= Z, as nanorq_decoder_add_symbol gives it (such a block has no symbols, hence no
 * gaps): ING_ERR (NANORQ_SYM_ERR) for an ESI above max_esi, else ING_IGN */
__global__ __launch_bounds__(256) void nrq_orx_foreign_kernel(const uint8_t *pkts, uint64_t pkt_stride, const uint32_t *tags, uint32_t n,
                                                              uint32_t Z, uint32_t max_esi, int32_t *results) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n) return;
  uint32_t tag;
  if (tags) {
    tag = tags[k];
  } else { /* the FEC Payload ID, network byte order */
    const uint8_t *p = pkts + (uint64_t)k * pkt_stride;
    tag = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
  }
  if ((tag >> 24) >= Z) results[k] = (tag & 0xFFFFFFu) > max_esi ? ING_ERR : ING_IGN;
}

struct nrq_otx : tx_sender {
  nrq_obj_params prm;
};

struct nrq_orx {
  nrq_ctx *ctx;
  nrq_obj_params prm;
  nrq_rx *rx[2];   /* class L (SBN 0 ..), class S (SBN ZL ..); null for an empty class */
  void *rows;      /* every block's row image, block b's at + boff(b) */
};

extern "C" {

int nrq_obj_layout(nrq_ctx *ctx, const nrq_obj_params *prm, void *d_obj, void *d_rows, int to_obj) {
  if (!ctx) return -1;
  int rc = obj_check(ctx, "nrq_obj_layout", prm);
  if (rc) return rc;
  if (!d_obj || !d_rows || (to_obj != 0 && to_obj != 1)) return fail(ctx, -1, "nrq_obj_layout: bad buffers or direction");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  return obj_layout_launch(ctx, obj_lay_of(prm, d_obj, d_rows, (uint32_t)to_obj));
}

int nrq_otx_create(nrq_ctx *ctx, const nrq_obj_params *prm, const void *d_obj, nrq_otx **out) {
  if (!ctx) return -1;
  if (!out) return fail(ctx, -1, "nrq_otx_create: out is NULL");
  *out = nullptr;
  int rc = obj_check(ctx, "nrq_otx_create", prm);
  if (rc) return rc;
  if (!d_obj) return fail(ctx, -1, "nrq_otx_create: d_obj is NULL");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const nrq_obj_params &p = *prm;
  rq_params pL{}, pS{};
  if (p.ZL && (rc = block_params(ctx, p.KL, p.KpL, &pL))) return rc;
  if (p.ZS && (rc = block_params(ctx, p.KS, p.KpS, &pS))) return rc;
  nrq_otx *tx = new (std::nothrow) nrq_otx();
  if (!tx) return fail(ctx, -1, "nrq_otx_create: out of host memory");
  tx->ctx = ctx;
  tx->unencoded = "the object is not encoded (nrq_otx_encode)";
  tx->prm = p;
  tx_src &o = tx->s;
  o.sbn0 = 0; o.Z = p.Z; o.ZL = p.ZL;
  memset(o.ready, 0xFF, sizeof(o.ready));
  const uint64_t T = p.T, LL = (uint64_t)pL.L * T, LS = (uint64_t)pS.L * T;
  const uint32_t last = p.Z - 1u, Klast = last < p.ZL ? p.KL : p.KS;
  const uint64_t olast = (uint64_t)(p.Kt - Klast) * T;
  const bool stage = p.N == 1u && p.F < (uint64_t)p.Kt * T;
  const uint8_t *rows = (const uint8_t *)d_obj;
  void *&own_rows = tx->own[1]; /* N > 1: every block's row image; N = 1: the staged last block (or nothing) */
  uint8_t *inter = nullptr;
  if ((rc = nrq_dev_alloc(ctx, (size_t)(p.ZL * LL + p.ZS * LS), &tx->own[0]))) goto bad;
  inter = (uint8_t *)tx->own[0];
  if (p.N > 1u) {
    if ((rc = nrq_dev_alloc(ctx, (size_t)p.Kt * T, &own_rows))) goto bad;
    if ((rc = obj_layout_launch(ctx, obj_lay_of(&p, (void *)d_obj, own_rows, 0)))) goto bad;
    rows = (const uint8_t *)own_rows;
  } else if (stage) {
    const size_t have = (size_t)(p.F - olast), full = (size_t)Klast * T;
    if ((rc = nrq_dev_alloc(ctx, full, &own_rows))) goto bad;
    hipError_t e = nrq_inject(ctx) ? hipErrorUnknown
                                   : hipMemcpyAsync(own_rows, (const uint8_t *)d_obj + olast, have, hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess) e = nrq_inject(ctx) ? hipErrorUnknown : hipMemsetAsync((uint8_t *)own_rows + have, 0, full - have, ctx->stream);
    if (e != hipSuccess) {
      rc = fail(ctx, -10, "nrq_otx_create: staging the last block failed: %s", hipGetErrorString(e));
      goto bad;
    }
  }
  {
    /* segments: class L, class S, each without a staged last block, then that block */
    auto seg = [&](uint32_t sbn0, uint32_t nblk, const rq_params &bp, uint32_t K, const uint8_t *src, uint64_t Lb) {
      if (!nblk) return;
      tx_blk &t = o.seg[o.nseg++];
      t.p = bp; t.K = K; t.T = p.T; t.nblk = nblk; t.sbn0 = sbn0;
      t.src = src; t.src_stride = (uint64_t)K * T;
      t.inter = inter + (sbn0 < p.ZL ? sbn0 * LL : p.ZL * LL + (sbn0 - p.ZL) * LS); t.inter_stride = Lb;
    };
    const uint32_t cutL = stage && last < p.ZL ? 1u : 0u, cutS = stage && last >= p.ZL ? 1u : 0u;
    seg(0, p.ZL - cutL, pL, p.KL, rows, LL);
    seg(p.ZL, p.ZS - cutS, pS, p.KS, rows + (uint64_t)p.ZL * p.KL * T, LS);
    if (stage) seg(last, 1, last < p.ZL ? pL : pS, Klast, (const uint8_t *)own_rows, last < p.ZL ? LL : LS);
  }
  *out = tx;
  return 0;
bad:
  nrq_otx_destroy(tx);
  return rc;
}

void nrq_otx_destroy(nrq_otx *tx) { tx_destroy(tx); }

int nrq_otx_encode(nrq_otx *tx) { return tx_encode(tx); }

int nrq_otx_oti(nrq_otx *tx, uint64_t *common, uint32_t *specific) {
  if (!tx) return -1;
  if (common) *common = tx->prm.oti_common;
  if (specific) *specific = tx->prm.oti_specific;
  return 0;
}

int nrq_otx_ready(nrq_otx *tx, uint32_t *h_ready) { return tx_ready(tx, "nrq_otx_ready", h_ready); }

int nrq_otx_emit(nrq_otx *tx, const uint32_t *d_tags, uint32_t n, void *d_pkts, size_t pkt_stride, uint32_t flags, int32_t *d_results) {
  return tx_emit_list(tx, "nrq_otx_emit", d_tags, n, d_pkts, pkt_stride, flags, d_results);
}

int nrq_otx_emit_all(nrq_otx *tx, uint32_t nrep, int order, void *d_pkts, size_t pkt_stride, uint32_t flags, uint32_t *d_tags_out) {
  if (!tx) return -1;
  nrq_ctx *ctx = tx->ctx;
  int rc = tx_check(tx, "nrq_otx_emit_all", d_pkts, pkt_stride, flags);
  if (rc) return rc;
  if ((rc = tx_check_order(tx, "nrq_otx_emit_all", order))) return rc;
  const nrq_obj_params &p = tx->prm;
  const uint64_t kmax = std::max(p.ZL ? p.KL : 0u, p.KS);
  if (kmax + nrep > (1u << 24)) return fail(ctx, -1, "nrq_otx_emit_all: ESIs up to %llu + %u reach past 2^24", (unsigned long long)kmax, nrep);
  const uint64_t total = (uint64_t)p.ZL * (p.KL + (uint64_t)nrep) + (uint64_t)p.ZS * (p.KS + (uint64_t)nrep);
  if (total > 0x7FFFFFFFu) return fail(ctx, -1, "nrq_otx_emit_all: %llu packets are too many", (unsigned long long)total);
  return tx_emit_span(tx, "nrq_otx_emit_all", 0, p.KL + nrep, p.KS + nrep, order, d_pkts, pkt_stride, flags, d_tags_out);
}

int nrq_orx_create(nrq_ctx *ctx, const nrq_obj_params *prm, uint32_t rep_cap, nrq_orx **out) {
  if (!ctx) return -1;
  if (!out) return fail(ctx, -1, "nrq_orx_create: out is NULL");
  *out = nullptr;
  int rc = obj_check(ctx, "nrq_orx_create", prm);
  if (rc) return rc;
  if (rep_cap == 0) return fail(ctx, -1, "nrq_orx_create: rep_cap is 0");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const nrq_obj_params &p = *prm;
  nrq_orx *rx = new (std::nothrow) nrq_orx();
  if (!rx) return fail(ctx, -1, "nrq_orx_create: out of host memory");
  rx->ctx = ctx;
  rx->prm = p;
  if ((rc = nrq_dev_alloc(ctx, (size_t)p.Kt * p.T, &rx->rows))) goto bad;
  if (p.ZL && (rc = nrq_rx_create(ctx, p.KL, p.KpL, p.T, p.ZL, 0, p.max_esi, rep_cap, rx->rows, (size_t)p.KL * p.T, nullptr, 0, &rx->rx[0])))
    goto bad;
  if (p.ZS && (rc = nrq_rx_create(ctx, p.KS, p.KpS, p.T, p.ZS, p.ZL, p.max_esi, rep_cap, (uint8_t *)rx->rows + (size_t)p.ZL * p.KL * p.T,
                                  (size_t)p.KS * p.T, nullptr, 0, &rx->rx[1])))
    goto bad;
  *out = rx;
  return 0;
bad:
  nrq_orx_destroy(rx);
  return rc;
}

int nrq_orx_relay(nrq_orx *rx, nrq_otx **out) {
  if (!rx) return -1;
  nrq_ctx *ctx = rx->ctx;
  if (!out) return fail(ctx, -1, "nrq_orx_relay: out is NULL");
  *out = nullptr;
  for (nrq_rx *r : rx->rx)
    if (r && r->relay) return fail(ctx, -1, "nrq_orx_relay: the reception has a relay already");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const nrq_obj_params &p = rx->prm;
  int rc = 0;
  rq_params pL{}, pS{};
  if (p.ZL && (rc = block_params(ctx, p.KL, p.KpL, &pL))) return rc;
  if (p.ZS && (rc = block_params(ctx, p.KS, p.KpS, &pS))) return rc;
  nrq_otx *tx = new (std::nothrow) nrq_otx();
  if (!tx) return fail(ctx, -1, "nrq_orx_relay: out of host memory");
  tx->ctx = ctx;
  tx->relay = tx->encoded = true;
  tx->unencoded = "";
  tx->prm = p;
  tx_src &o = tx->s;
  o.sbn0 = 0; o.Z = p.Z; o.ZL = p.ZL;
  const uint64_t T = p.T, LL = (uint64_t)pL.L * T, LS = (uint64_t)pS.L * T;
  if ((rc = nrq_dev_alloc(ctx, (size_t)(p.ZL * LL + p.ZS * LS), &tx->own[0]))) {
    delete tx;
    return rc;
  }
  /* the class table over the receptions' rows (Kt * T bytes, zero-padded behind F by the last packet's sender: no staged last
   * block), the intermediate symbols class L first, class S behind it, as nrq_otx_create lays them out */
  const rq_params *bp[2] = {&pL, &pS};
  const uint64_t Lb[2] = {LL, LS}, ioff[2] = {0, p.ZL * LL};
  for (int c = 0; c < 2; c++) {
    nrq_rx *r = rx->rx[c];
    if (!r) continue;
    const uint32_t g = o.nseg++;
    tx_blk &t = o.seg[g];
    t.p = *bp[c]; t.K = r->r.K; t.T = p.T; t.nblk = r->r.nblk; t.sbn0 = r->r.sbn0;
    t.src = r->r.src; t.src_stride = r->r.src_stride;
    t.inter = (const uint8_t *)tx->own[0] + ioff[c]; t.inter_stride = Lb[c];
    tx->from[g] = r;
    r->relay = tx; r->relay_seg = g; r->relay_b0 = r->r.sbn0;
  }
  *out = tx;
  return 0;
}

void nrq_orx_destroy(nrq_orx *rx) {
  if (!rx) return;
  for (nrq_rx *r : rx->rx) nrq_rx_destroy(r);
  if (rx->rows) nrq_dev_free(rx->ctx, rx->rows); /* (nrq_rx_destroy waited for the stream) */
  delete rx;
}

int nrq_orx_add(nrq_orx *rx, const void *d_pkts, size_t pkt_stride, const uint32_t *d_tags, uint32_t n, uint32_t flags, int32_t *d_results) {
  if (!rx) return -1;
  nrq_ctx *ctx = rx->ctx;
  for (nrq_rx *r : rx->rx) {
    if (!r) continue;
    const int rc = nrq_rx_add(r, d_pkts, pkt_stride, d_tags, n, flags, d_results);
    if (rc) return rc;
  }
  if (n == 0 || !d_results) return 0;
  hipLaunchKernelGGL(nrq_orx_foreign_kernel, dim3((n + 255u) / 256u), dim3(256), 0, ctx->stream, (const uint8_t *)d_pkts,
                     (uint64_t)pkt_stride, d_tags, n, rx->prm.Z, rx->prm.max_esi, d_results);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int nrq_orx_counts(nrq_orx *rx, uint32_t *h_nlost, uint32_t *h_nrep) {
  if (!rx) return -1;
  const uint32_t sbn0[2] = {0, rx->prm.ZL};
  for (int c = 0; c < 2; c++) {
    if (!rx->rx[c]) continue;
    const int rc = nrq_rx_counts(rx->rx[c], h_nlost ? h_nlost + sbn0[c] : nullptr, h_nrep ? h_nrep + sbn0[c] : nullptr);
    if (rc) return rc;
  }
  return 0;
}

int nrq_orx_decode(nrq_orx *rx, int *h_status, uint32_t *h_used) {
  if (!rx) return -1;
  if (!h_status) return fail(rx->ctx, -1, "nrq_orx_decode: h_status is NULL");
  const uint32_t sbn0[2] = {0, rx->prm.ZL};
  for (int c = 0; c < 2; c++) {
    if (!rx->rx[c]) continue;
    const int rc = nrq_rx_decode(rx->rx[c], h_status + sbn0[c], h_used ? h_used + sbn0[c] : nullptr);
    if (rc) return rc;
  }
  return 0;
}

int nrq_orx_write(nrq_orx *rx, void *d_out) {
  if (!rx) return -1;
  nrq_ctx *ctx = rx->ctx;
  if (!d_out) return fail(ctx, -1, "nrq_orx_write: d_out is NULL");
  const uint32_t Z = rx->prm.Z;
  std::vector<uint32_t> gaps(Z, 0);
  int rc = nrq_orx_counts(rx, gaps.data(), nullptr);
  if (rc) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  obj_lay l = obj_lay_of(&rx->prm, d_out, rx->rows, 1);
  int incomplete = 0;
  for (uint32_t &w : l.mask) w = 0;
  for (uint32_t b = 0; b < Z; b++) {
    if (gaps[b]) incomplete++;
    else l.mask[b >> 5] |= 1u << (b & 31u);
  }
  if (incomplete < (int)Z && (rc = obj_layout_launch(ctx, l))) return rc;
  return incomplete;
}

} /* extern "C" */

/* ================================================ packets of several symbols (nrq_*_syms, syms_body.h) ==== */
/* Kernels of their own beside the one-symbol ones: every instantiation of those is compiled from the code it always was.  What is
 * inside them is shared with those: the ranking (ing_rank_wg), the payload walk (tx_payload over a tx_run), the segment base, and
 * on the host the path rule, the bucketing (tx_bucket) and the ingest call (ing_call_of).
 *
 * Ingest: the chain of nrq_rx_add over n * G slots.  Passes 2 and 4 are per block and are nrq_rx_add's kernels; passes 1, 3, 5, 7
 * are these, which ask syms_body.h what a slot is; pass 6 walks a packet's payloads as one contiguous run. */
__global__ __launch_bounds__(256) void nrq_ing_first_syms_kernel(ing_rx r, ing_call c, sy_rx y) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s < c.n) sy_first(&r, &c, &y, s);
}

__global__ __launch_bounds__(256) void nrq_ing_hist_syms_kernel(ing_rx r, ing_call c, sy_rx y) {
  __shared__ uint32_t h[256];
  const uint32_t t = threadIdx.x, s = blockIdx.x * ING_TILE + t;
  h[t] = 0;
  __syncthreads();
  if (s < c.n) {
    const uint32_t b = sy_cand(&r, &c, &y, s);
    if (b != ING_NONE) atomicAdd(&h[b], 1u);
  }
  __syncthreads();
  if (t < r.nblk) c.base[(size_t)t * c.ntiles + blockIdx.x] = h[t];
}

/* (nrq_ing_classify_kernel over slots: the same ranking, in slot order) */
__global__ __launch_bounds__(256) void nrq_ing_classify_syms_kernel(ing_rx r, ing_call c, sy_rx y) {
  __shared__ uint32_t wc[4][256];
  const uint32_t t = threadIdx.x, s = blockIdx.x * ING_TILE + t;
  for (uint32_t i = t; i < 4u * 256u; i += 256u) wc[i >> 8][i & 255u] = 0;
  __syncthreads();
  const uint32_t b = s < c.n ? sy_cand(&r, &c, &y, s) : ING_NONE;
  const uint32_t row = ing_rank_wg(&wc[0][0], 256u, b, c.base, c.ntiles);
  if (s < c.n) sy_classify(&r, &c, &y, s, row);
}

__global__ __launch_bounds__(256) void nrq_ing_fold_syms_kernel(ing_rx r, ing_call c, sy_rx y) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s < c.n) sy_fold(&r, &c, &y, s);
}

/* One wave per packet: lane i holds the destination of slot (k, i); the wave walks the payloads up to the last slot that has
 * one as ONE contiguous run, a W-byte word per lane and trip whatever symbol boundaries fall inside (T is a multiple of W: a
 * word lies in one symbol), and each lane stores its word into the row of the slot it falls into.  A destination of 0: skip.
 * W = the widest word every address of the call allows (sy_copy_word, decided by the launcher). */
template <typename W>
__global__ __launch_bounds__(256) void nrq_ing_copy_syms_kernel(const uint8_t *__restrict__ pkts, uint64_t pkt_stride,
                                                                const uint64_t *__restrict__ dst, uint32_t n, uint32_t G, uint32_t T,
                                                                uint32_t payload_off) {
  const uint32_t k = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (k >= n) return; /* (wave-uniform) */
  const uint64_t d = lane < G ? dst[(uint64_t)k * G + lane] : 0ull;
  const uint64_t m = __ballot(d != 0ull);
  if (!m) return;
  const uint32_t len = (64u - (uint32_t)__clzll((long long)m)) * T; /* (G * T fits 32 bits: the launcher checked) */
  const uint32_t dlo = (uint32_t)d, dhi = (uint32_t)(d >> 32);
  const uint8_t *__restrict__ s = pkts + (size_t)k * pkt_stride + payload_off;
  constexpr uint32_t WB = (uint32_t)sizeof(W);
  for (uint32_t o0 = 0; o0 < len; o0 += 64u * WB) { /* (wave-uniform: every lane takes part in the shuffles) */
    const uint32_t off = o0 + lane * WB;
    const bool act = off < len;
    const uint32_t i = act ? off / T : 0u;
    const uint64_t di = ((uint64_t)(uint32_t)__shfl((int)dhi, (int)i) << 32) | (uint32_t)__shfl((int)dlo, (int)i);
    if (act && di) *reinterpret_cast<W *>(reinterpret_cast<uint8_t *>(di) + (off - i * T)) = *reinterpret_cast<const W *>(s + off);
  }
}

/* the codes of an object's packets of SBN >= Z, slot by slot (nrq_orx_foreign_kernel's rule over the expansion) */
__global__ __launch_bounds__(256) void nrq_orx_foreign_syms_kernel(const uint8_t *pkts, uint64_t pkt_stride, const uint32_t *tags, uint32_t n,
                                                                   uint32_t G, const uint8_t *nsym, uint32_t Z, uint32_t max_esi,
                                                                   int32_t *results) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= n * G) return;
  const uint32_t k = s / G, i = s - k * G;
  ing_call c{};
  c.pkts = pkts; c.pkt_stride = pkt_stride; c.tags = tags;
  const uint32_t tag = sy_first_tag(&c, k);
  if ((tag >> 24) < Z) return;
  const uint32_t cnt = nsym ? nsym[k] : G;
  if (cnt == 0u || cnt > G) {
    if (i == 0u) results[s] = ING_ERR;
  } else if (i < cnt) {
    results[s] = (tag & SY_ESI_MAX) + i > max_esi ? ING_ERR : ING_IGN;
  }
}

/* Emit.  The wave shape of nrq_emit_kernel with SLOTS as work items: a wave takes 64 / G packets of the work order (block-major;
 * a tag list bucketed by block), lane l the slot (l / G, l % G) -- a packet's slots are adjacent and never split across waves.
 * Each lane admits its packet (sy_tx_admit: per packet, so every lane of a packet decides alike) and builds its slot's column
 * list into LDS; then the wave writes the admitted packets one after the other, each as ONE run of c_k * T bytes with lanes across
 * the symbol boundaries: a lane gathers with the column list of the slot its word lies in (tx_payload over a tx_run; a packet of
 * one symbol takes the one-symbol walk: no boundary to look for). */
template <int MODE, bool MULTI>
__global__ __launch_bounds__(256) void nrq_emit_syms_kernel(tx_src s, tx_call c, sy_tx y) {
  __shared__ uint32_t s_cols[TX_WAVES][TX_WAVE_PKTS][TX_COLS];
  __shared__ uint32_t s_n[TX_WAVES][TX_WAVE_PKTS], s_tag[TX_WAVES][TX_WAVE_PKTS], s_k[TX_WAVES][TX_WAVE_PKTS];
  __shared__ uint32_t s_seg[TX_WAVES][TX_WAVE_PKTS]; /* (MULTI only: unused LDS is not allocated) */
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint32_t G = y.G, per = 64u / G, p = lane / G, i = lane - p * G;
  const uint64_t w0 = ((uint64_t)blockIdx.x * TX_WAVES + wv) * per; /* the wave's first packet in the work order */
  {
    uint32_t n = 0, cnt = 0, tag0 = 0, k = 0, sg = TX_SEGS;
    if (p < per && w0 + p < c.n) {
      k = tx_packet_of<MULTI>(&s, &c, (uint32_t)(w0 + p));
      if (k < c.n) { /* (always: the work order is a permutation) */
        bool ranged;
        int32_t code;
        tag0 = sy_tx_packet<MULTI>(&s, &c, &y, k, &cnt, &ranged);
        sg = sy_tx_admit<MULTI>(&s, &y, tag0, k, ranged, &code, &cnt);
        const tx_blk sb = MULTI ? tx_pick(&s, sg) : s.seg[0];
        if (sg < TX_SEGS && i < cnt) n = tx_rows(&sb, tag0 + i, s_cols[wv][lane]);
        if (i == 0u) {
          if (c.results) c.results[k] = code;
          if (c.tags_out) c.tags_out[k] = tag0;
          if (y.nsym_out) y.nsym_out[k] = (uint8_t)cnt;
        }
      }
    }
    s_n[wv][lane] = n | (cnt << 8); /* (cnt = 0: the packet stays untouched) */
    s_tag[wv][lane] = tag0;
    s_k[wv][lane] = k;
    if (MULTI) s_seg[wv][lane] = sg;
  }
  __syncthreads();
  const uint32_t T = s.seg[0].T;
  for (uint32_t q = 0; q < per && w0 + q < c.n; q++) { /* (wave-uniform) */
    const uint32_t l0 = q * G;
    const uint32_t nk = __builtin_amdgcn_readfirstlane(s_n[wv][l0]), cnt = nk >> 8;
    if (!cnt) continue;
    const uint32_t tag = __builtin_amdgcn_readfirstlane(s_tag[wv][l0]);
    const uint32_t sg = MULTI ? __builtin_amdgcn_readfirstlane(s_seg[wv][l0]) : 0u;
    const uint8_t *base = TX_SEG_BASE(MULTI, s, sg, tag);
    uint8_t *P = c.pkts + (uint64_t)s_k[wv][l0] * c.pkt_stride;
    if (cnt == 1u) tx_payload<MODE>(base, T, tx_one{s_cols[wv][l0], nk & 0xFFu}, tag, P, c.inl, lane);
    else tx_payload<MODE>(base, T, tx_run{&s_cols[wv][l0], &s_n[wv][l0], cnt}, tag, P, c.inl, lane);
  }
}

/* The tag-list emit of several symbols with held symbols (NRQ_TX_HELD; relays only): the wave shape of nrq_emit_syms_kernel, a
 * kernel of its own so that its instantiations and nrq_emit_held_kernel's are compiled from the code they always were.  Admission
 * (hs_packet, runs_body.h): a ready block's packet goes the usual way; one of a block that is not ready is written iff the
 * reception holds EVERY one of its symbols -- each lane asks for its slot's seen bit, a ballot over the packet's lanes decides, so
 * a packet is written whole or not at all.  Held source symbols are source rows e .. e+c-1.  The rows of held repair symbols are
 * found per packet by the wave that writes it: one walk over the block's repair list in trips of 64, a lane whose entry lies in
 * [e, e+c) stores its row index into the LDS word of slot entry - e (the head of that slot's column list); the packet is then one
 * run over single-row lists from the base of the block's repair rows. */
template <int MODE, bool MULTI>
__global__ __launch_bounds__(256) void nrq_emit_held_syms_kernel(tx_src s, tx_held h, tx_call c, sy_tx y) {
  __shared__ uint32_t s_cols[TX_WAVES][TX_WAVE_PKTS][TX_COLS];
  __shared__ uint32_t s_n[TX_WAVES][TX_WAVE_PKTS], s_tag[TX_WAVES][TX_WAVE_PKTS], s_k[TX_WAVES][TX_WAVE_PKTS];
  __shared__ uint32_t s_seg[TX_WAVES][TX_WAVE_PKTS]; /* (MULTI only: unused LDS is not allocated) */
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint32_t G = y.G, per = 64u / G, p = lane / G, i = lane - p * G;
  const uint64_t w0 = ((uint64_t)blockIdx.x * TX_WAVES + wv) * per; /* the wave's first packet in the work order */
  {
    uint32_t n = 0, cnt = 0, tag0 = 0, k = 0, sg = TX_SEGS, ready = 0, kind = TX_READY;
    int32_t code = TX_FOREIGN;
    const bool mine = p < per && w0 + p < c.n;
    if (mine) {
      k = c.order[w0 + p];
      tag0 = c.tags[k];
      sg = hs_packet<MULTI>(&s, &y, tag0, k, &code, &cnt, &ready);
    }
    const tx_blk sb = MULTI ? tx_pick(&s, sg) : s.seg[0];
    const uint32_t e = tag0 & SY_ESI_MAX;
    /* all or nothing: every slot of a packet of a block that is not ready must be held (every lane of the wave takes the ballot) */
    bool ok = true;
    if (sg < TX_SEGS && !ready && i < cnt) { /* (a branch per segment: a select over the by-value table would be indexed from scratch) */
      const uint32_t b = tx_block(&sb, tag0);
      if (!MULTI || sg == 0u) ok = hs_slot_held(&h.seg[0], b, e + i);
      else if (sg == 1u) ok = hs_slot_held(&h.seg[1], b, e + i);
      else ok = hs_slot_held(&h.seg[2], b, e + i);
    }
    const uint64_t held = __ballot(ok), pmask = (cnt >= 64u ? ~0ull : (1ull << cnt) - 1ull) << (p * G);
    if (sg < TX_SEGS && !ready) {
      if ((held & pmask) != pmask) { code = TX_NOT_READY; cnt = 0u; sg = TX_SEGS; }
      else kind = e < sb.K ? TX_HELD_SRC : TX_HELD_REP;
    }
    if (sg < TX_SEGS && i < cnt) {
      if (kind == TX_HELD_REP) { s_cols[wv][lane][0] = TX_NONE; n = 1u; } /* (the row index: found below) */
      else n = tx_rows(&sb, tag0 + i, s_cols[wv][lane]);                  /* (a held source symbol: row e + i, as a ready one) */
    }
    if (mine && i == 0u && c.results && kind != TX_HELD_REP) c.results[k] = code; /* (held repair symbols: once the rows are found) */
    s_n[wv][lane] = n | (cnt << 8) | (kind << 16); /* (cnt = 0: the packet stays untouched) */
    s_tag[wv][lane] = tag0;
    s_k[wv][lane] = k;
    if (MULTI) s_seg[wv][lane] = sg;
  }
  __syncthreads();
  const uint32_t T = s.seg[0].T;
  for (uint32_t q = 0; q < per && w0 + q < c.n; q++) { /* (wave-uniform) */
    const uint32_t l0 = q * G;
    const uint32_t nk = __builtin_amdgcn_readfirstlane(s_n[wv][l0]), cnt = (nk >> 8) & 0xFFu;
    if (!cnt) continue;
    const uint32_t tag = __builtin_amdgcn_readfirstlane(s_tag[wv][l0]);
    const uint32_t sg = MULTI ? __builtin_amdgcn_readfirstlane(s_seg[wv][l0]) : 0u;
    const uint8_t *base;
    if ((nk >> 16) == TX_HELD_REP) {
      const tx_held_seg hs = sg == 0u ? h.seg[0] : sg == 1u ? h.seg[1] : h.seg[2];
      const uint32_t b = (tag >> 24) - (sg == 0u ? s.seg[0].sbn0 : sg == 1u ? s.seg[1].sbn0 : s.seg[2].sbn0);
      const uint32_t nrep = tx_held_nrep(&hs, b), e = tag & SY_ESI_MAX;
      for (uint32_t q0 = 0; q0 < nrep; q0 += 64u) {
        const uint32_t x = q0 + lane < nrep ? hs.rep_esi[(uint64_t)b * hs.rep_cap + q0 + lane] - e : TX_NONE;
        if (x < cnt) s_cols[wv][l0 + x][0] = q0 + lane;
      }
      /* the wave reads what its other lanes wrote: LDS operations of one wave complete in order; the fence keeps the compiler from
       * moving the reads above the writes */
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      const bool found = lane >= cnt || s_cols[wv][l0 + lane][0] != TX_NONE;
      const bool all = __ballot(!found) == 0ull;
      if (c.results && lane == 0) c.results[s_k[wv][l0]] = all ? 0 : TX_NOT_READY;
      if (!all) continue; /* (the books say otherwise: a marked repair ESI has its row) */
      base = tx_held_rep_base(&hs, b);
    } else {
      base = TX_SEG_BASE(MULTI, s, sg, tag);
    }
    uint8_t *P = c.pkts + (uint64_t)s_k[wv][l0] * c.pkt_stride;
    if (cnt == 1u) tx_payload<MODE>(base, T, tx_one{s_cols[wv][l0], nk & 0xFFu}, tag, P, c.inl, lane);
    else tx_payload<MODE>(base, T, tx_run{&s_cols[wv][l0], &s_n[wv][l0], cnt}, tag, P, c.inl, lane);
  }
}

static int rx_add_syms(nrq_rx *rx, const char *who, const void *d_pkts, size_t pkt_stride, const uint32_t *d_tags, uint32_t n, uint32_t G,
                       const uint8_t *d_nsym, uint32_t flags, int32_t *d_results) {
  nrq_ctx *ctx = rx->ctx;
  const ing_rx &r = rx->r;
  const bool inl = (flags & NRQ_RX_TAG_INLINE) != 0;
  if (flags & ~(uint32_t)NRQ_RX_TAG_INLINE) return fail(ctx, -1, "%s: unknown flags 0x%x", who, flags);
  if (G == 0 || G > NRQ_PKT_SYMS_MAX) return fail(ctx, -1, "%s: G=%u outside 1..%u", who, G, NRQ_PKT_SYMS_MAX);
  if (n == 0) return 0;
  const size_t pkt_len = (uint64_t)G * r.T > 0xFFFFFFFFu ? SIZE_MAX : (size_t)G * r.T + (inl ? 4u : 0u);
  const uint32_t ns = n * G;
  ing_call c;
  sy_rx y{};
  y.G = G; y.nsym = d_nsym;
  const int rc = ing_call_of(ctx, rx->scratch, who, d_pkts, pkt_stride, d_tags, n, G, pkt_len, inl, r.nblk, d_results, ns, &c, &y.kind);
  if (rc) return rc;
  const uint32_t hdr = ing_payload_off(&c);
  const uint32_t word = sy_copy_word(reinterpret_cast<uintptr_t>(d_pkts) | pkt_stride | hdr | r.T | reinterpret_cast<uintptr_t>(r.src) |
                                     r.src_stride | reinterpret_cast<uintptr_t>(r.rep) | r.rep_stride);
  hipStream_t st = ctx->stream;
  const uint32_t g = (ns + 255u) / 256u;
  hipLaunchKernelGGL(nrq_ing_first_syms_kernel, dim3(g), dim3(256), 0, st, r, c, y);
  hipLaunchKernelGGL(nrq_ing_done_kernel, dim3(r.nblk), dim3(256), 0, st, r);
  hipLaunchKernelGGL(nrq_ing_hist_syms_kernel, dim3(c.ntiles), dim3(256), 0, st, r, c, y);
  hipLaunchKernelGGL(nrq_ing_scan_kernel, dim3(r.nblk), dim3(256), 0, st, r, c);
  hipLaunchKernelGGL(nrq_ing_classify_syms_kernel, dim3(c.ntiles), dim3(256), 0, st, r, c, y);
  const dim3 cg((n + 3u) / 4u);
  if (word == 16u)
    hipLaunchKernelGGL(nrq_ing_copy_syms_kernel<uint4>, cg, dim3(256), 0, st, c.pkts, c.pkt_stride, (const uint64_t *)c.dst, n, G, r.T, hdr);
  else if (word == 4u)
    hipLaunchKernelGGL(nrq_ing_copy_syms_kernel<uint32_t>, cg, dim3(256), 0, st, c.pkts, c.pkt_stride, (const uint64_t *)c.dst, n, G, r.T, hdr);
  else
    hipLaunchKernelGGL(nrq_ing_copy_syms_kernel<uint8_t>, cg, dim3(256), 0, st, c.pkts, c.pkt_stride, (const uint64_t *)c.dst, n, G, r.T, hdr);
  hipLaunchKernelGGL(nrq_ing_fold_syms_kernel, dim3(g), dim3(256), 0, st, r, c, y);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

/* checks of the several-symbol emits on top of tx_check; list: the tag-list form, which alone takes NRQ_TX_HELD, and only on a relay
 * (tx_check says so for a range form and for a sender) */
static int sy_tx_check(tx_sender *tx, const char *who, const void *d_pkts, size_t pkt_stride, uint32_t G, uint32_t flags, bool list = false) {
  nrq_ctx *ctx = tx->ctx;
  int rc = tx_check(tx, who, d_pkts, pkt_stride, flags, list);
  if (rc) return rc;
  if (G == 0 || G > NRQ_PKT_SYMS_MAX) return fail(ctx, -1, "%s: G=%u outside 1..%u", who, G, NRQ_PKT_SYMS_MAX);
  const uint32_t T = tx->s.seg[0].T;
  if ((uint64_t)G * T > 0xFFFFFFFFu || pkt_stride < (size_t)G * T + ((flags & NRQ_TX_TAG_INLINE) ? 4u : 0u))
    return fail(ctx, -1, "%s: pkt_stride %zu shorter than a packet of %u symbols", who, pkt_stride, G);
  return 0;
}

static int sy_tx_launch(tx_sender *tx, const tx_call &c, const sy_tx &y, bool held = false) {
  using emit_fn = void (*)(tx_src, tx_call, sy_tx);
  using held_fn = void (*)(tx_src, tx_held, tx_call, sy_tx);
  static const held_fn hkern[2][4] = { /* [multi-segment][path] */
      {nrq_emit_held_syms_kernel<TX_V16, false>, nrq_emit_held_syms_kernel<TX_V16_SHIFT, false>, nrq_emit_held_syms_kernel<TX_DWORD, false>,
       nrq_emit_held_syms_kernel<TX_BYTE, false>},
      {nrq_emit_held_syms_kernel<TX_V16, true>, nrq_emit_held_syms_kernel<TX_V16_SHIFT, true>, nrq_emit_held_syms_kernel<TX_DWORD, true>,
       nrq_emit_held_syms_kernel<TX_BYTE, true>}};
  static const emit_fn kern[2][4] = { /* [multi-segment][path] */
      {nrq_emit_syms_kernel<TX_V16, false>, nrq_emit_syms_kernel<TX_V16_SHIFT, false>, nrq_emit_syms_kernel<TX_DWORD, false>,
       nrq_emit_syms_kernel<TX_BYTE, false>},
      {nrq_emit_syms_kernel<TX_V16, true>, nrq_emit_syms_kernel<TX_V16_SHIFT, true>, nrq_emit_syms_kernel<TX_DWORD, true>,
       nrq_emit_syms_kernel<TX_BYTE, true>}};
  nrq_ctx *ctx = tx->ctx;
  const tx_src &s = tx->s;
  const tx_held h = held ? tx_held_table(tx) : tx_held{};
  const int mode = tx_emit_path(tx_align(&s, &c, held ? &h : nullptr), c.inl, ctx->tune.tx_dword ? 1u : 0u); /* (held: the repair rows too) */
  const uint32_t per = 64u / y.G, waves = (c.n + per - 1u) / per;
  const dim3 grid((waves + TX_WAVES - 1u) / TX_WAVES), wg(64u * TX_WAVES);
  if (held) hipLaunchKernelGGL(hkern[s.nseg > 1u][mode], grid, wg, 0, ctx->stream, s, h, c, y);
  else hipLaunchKernelGGL(kern[s.nseg > 1u][mode], grid, wg, 0, ctx->stream, s, c, y);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

static int sy_emit_list(tx_sender *tx, const char *who, const uint32_t *d_tags, uint32_t n, uint32_t G, const uint8_t *d_nsym, void *d_pkts,
                        size_t pkt_stride, uint32_t flags, int32_t *d_results) {
  if (!tx) return -1;
  nrq_ctx *ctx = tx->ctx;
  int rc = sy_tx_check(tx, who, d_pkts, pkt_stride, G, flags, true);
  if (rc) return rc;
  if (n == 0) return 0;
  if (!d_tags || (uint64_t)n * G > 0x7FFFFFFFu) return fail(ctx, -1, "%s: bad tags (n=%u, G=%u)", who, n, G);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  tx_call c = tx_call_of(d_pkts, pkt_stride, n, flags);
  if ((rc = tx_bucket(tx, d_tags, n, &c.order))) return rc;
  c.tags = d_tags;
  c.results = d_results;
  sy_tx y{};
  y.G = G; y.nsym = d_nsym;
  return sy_tx_launch(tx, c, y, (flags & NRQ_TX_HELD) != 0);
}

/* range mode: ESIs esi0 .. esi0+eL-1 of the blocks of K = KL, esi0 .. esi0+eS-1 of those of K = KS, packetised per block */
static int sy_emit_span(tx_sender *tx, const char *who, uint32_t KL, uint32_t KS, uint32_t esi0, uint32_t eL, uint32_t eS, uint32_t G, int order,
                        void *d_pkts, size_t pkt_stride, uint32_t flags, uint32_t *d_tags_out, uint8_t *d_nsym_out, uint32_t *h_npkt) {
  nrq_ctx *ctx = tx->ctx;
  const int rc = tx_span_ready(tx, who);
  if (rc) return rc;
  const uint32_t ZL = tx->s.ZL, ZS = tx->s.Z - ZL;
  if (!ZL) { KL = KS; eL = eS; } /* (a table of one class has its counts in both: the one-segment maps) */
  const uint32_t pL = sy_pkt_count(KL, esi0, eL, G), pS = ZS ? sy_pkt_count(KS, esi0, eS, G) : pL;
  const uint64_t total = (uint64_t)ZL * pL + (uint64_t)ZS * pS;
  if (total * G > 0x7FFFFFFFu) return fail(ctx, -1, "%s: %llu packets of %u symbols are too many", who, (unsigned long long)total, G);
  if (h_npkt) *h_npkt = (uint32_t)total;
  if (total == 0) return 0;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  tx_call c = tx_call_of(d_pkts, pkt_stride, (uint32_t)total, flags);
  c.esi0 = esi0;
  c.nL = ZL ? pL : pS;
  c.nS = pS;
  c.interleave = (uint32_t)order;
  c.tags_out = d_tags_out;
  sy_tx y{};
  y.G = G; y.nsym_out = d_nsym_out; y.eL = eL; y.eS = eS;
  return sy_tx_launch(tx, c, y);
}

extern "C" {

uint32_t nrq_pkt_count(uint32_t K, uint32_t esi0, uint32_t n, uint32_t G) { return G ? sy_pkt_count(K, esi0, n, G) : 0u; }

int nrq_rx_add_syms(nrq_rx *rx, const void *d_pkts, size_t pkt_stride, const uint32_t *d_tags, uint32_t n, uint32_t G, const uint8_t *d_nsym,
                    uint32_t flags, int32_t *d_results) {
  if (!rx) return -1;
  return rx_add_syms(rx, "nrq_rx_add_syms", d_pkts, pkt_stride, d_tags, n, G, d_nsym, flags, d_results);
}

int nrq_orx_add_syms(nrq_orx *rx, const void *d_pkts, size_t pkt_stride, const uint32_t *d_tags, uint32_t n, uint32_t G, const uint8_t *d_nsym,
                     uint32_t flags, int32_t *d_results) {
  if (!rx) return -1;
  nrq_ctx *ctx = rx->ctx;
  for (nrq_rx *r : rx->rx) {
    if (!r) continue;
    const int rc = rx_add_syms(r, "nrq_orx_add_syms", d_pkts, pkt_stride, d_tags, n, G, d_nsym, flags, d_results);
    if (rc) return rc;
  }
  if (n == 0 || !d_results) return 0;
  hipLaunchKernelGGL(nrq_orx_foreign_syms_kernel, dim3((n * G + 255u) / 256u), dim3(256), 0, ctx->stream, (const uint8_t *)d_pkts,
                     (uint64_t)pkt_stride, d_tags, n, G, d_nsym, rx->prm.Z, rx->prm.max_esi, d_results);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int nrq_tx_emit_syms(nrq_tx *tx, const uint32_t *d_tags, uint32_t n, uint32_t G, const uint8_t *d_nsym, void *d_pkts, size_t pkt_stride,
                     uint32_t flags, int32_t *d_results) {
  return sy_emit_list(tx, "nrq_tx_emit_syms", d_tags, n, G, d_nsym, d_pkts, pkt_stride, flags, d_results);
}

int nrq_otx_emit_syms(nrq_otx *tx, const uint32_t *d_tags, uint32_t n, uint32_t G, const uint8_t *d_nsym, void *d_pkts, size_t pkt_stride,
                      uint32_t flags, int32_t *d_results) {
  return sy_emit_list(tx, "nrq_otx_emit_syms", d_tags, n, G, d_nsym, d_pkts, pkt_stride, flags, d_results);
}

int nrq_tx_emit_range_syms(nrq_tx *tx, uint32_t esi0, uint32_t n, uint32_t G, int order, void *d_pkts, size_t pkt_stride, uint32_t flags,
                           uint32_t *d_tags_out, uint8_t *d_nsym_out, uint32_t *h_npkt) {
  if (!tx) return -1;
  nrq_ctx *ctx = tx->ctx;
  const char *who = "nrq_tx_emit_range_syms";
  if (h_npkt) *h_npkt = 0;
  int rc = sy_tx_check(tx, who, d_pkts, pkt_stride, G, flags);
  if (rc) return rc;
  if ((rc = tx_check_order(tx, who, order))) return rc;
  if (n == 0) return 0;
  if (esi0 >= (1u << 24) || n > (1u << 24) - esi0) return fail(ctx, -1, "%s: ESIs %u + %u reach past 2^24", who, esi0, n);
  const uint32_t K = tx->s.seg[0].K;
  return sy_emit_span(tx, who, K, K, esi0, n, n, G, order, d_pkts, pkt_stride, flags, d_tags_out, d_nsym_out, h_npkt);
}

int nrq_otx_emit_all_syms(nrq_otx *tx, uint32_t nrep, uint32_t G, int order, void *d_pkts, size_t pkt_stride, uint32_t flags,
                          uint32_t *d_tags_out, uint8_t *d_nsym_out, uint32_t *h_npkt) {
  if (!tx) return -1;
  nrq_ctx *ctx = tx->ctx;
  const char *who = "nrq_otx_emit_all_syms";
  if (h_npkt) *h_npkt = 0;
  int rc = sy_tx_check(tx, who, d_pkts, pkt_stride, G, flags);
  if (rc) return rc;
  if ((rc = tx_check_order(tx, who, order))) return rc;
  const nrq_obj_params &p = tx->prm;
  const uint64_t kmax = std::max(p.ZL ? p.KL : 0u, p.KS);
  if (kmax + nrep > (1u << 24)) return fail(ctx, -1, "%s: ESIs up to %llu + %u reach past 2^24", who, (unsigned long long)kmax, nrep);
  return sy_emit_span(tx, who, p.KL, p.KS, 0, p.KL + nrep, p.KS + nrep, G, order, d_pkts, pkt_stride, flags, d_tags_out, d_nsym_out, h_npkt);
}

} /* extern "C" */

/* ================================================ what a reception holds (nrq_rx_held / nrq_orx_held, held_body.h) ==== */
/* The listing passes as workgroup bodies of (reception, block): nrq_held_*_kernel runs them on its by-value reception and
 * blockIdx.x, nrq_ings_held_*_kernel on the member and block it finds in a set's table (ps: 256 words of LDS). */
/* count: seen source ESIs plus repair rows used -> cnt[g] */
__device__ __forceinline__ void hl_count_wg(const ing_rx *r, uint32_t b, uint32_t *cnt, uint32_t g, uint32_t *ps) {
  const uint32_t t = threadIdx.x, nw = ing_src_words(r);
  uint32_t n = 0;
  for (uint32_t w = t; w < nw; w += 256u) n += ing_popc(hl_have(r, b, w));
  n = wg_sum(ps, t, n);
  if (t == 0) cnt[g] = n + hl_nrep(r, b);
}

/* fill: the block's tags to out[o ..] -- the seen source ESIs ascending (256 words per round: a scan over their counts places
 * each word's tags), then the repair ESIs in arrival order */
__device__ __forceinline__ void hl_fill_wg(const ing_rx *r, uint32_t b, uint32_t *out, uint32_t o, uint32_t *ps) {
  const uint32_t t = threadIdx.x, nw = ing_src_words(r);
  for (uint32_t w0 = 0; w0 < nw; w0 += 256u) {
    const uint32_t w = w0 + t;
    const uint32_t have = w < nw ? hl_have(r, b, w) : 0u, cnt = ing_popc(have);
    hl_put(r, b, w, have, out + o + wg_scan(ps, t, cnt) - cnt);
    o += ps[255];
    __syncthreads();
  }
  const uint32_t nrep = hl_nrep(r, b);
  for (uint32_t q = t; q < nrep; q += 256u) out[o + q] = hl_rep_tag(r, b, q);
}

/* one workgroup per block: seen source ESIs plus repair rows used -> cnt[b] */
__global__ __launch_bounds__(256) void nrq_held_count_kernel(ing_rx r, uint32_t *cnt) {
  __shared__ uint32_t ps[256];
  hl_count_wg(&r, blockIdx.x, cnt, blockIdx.x, ps);
}

/* one workgroup per block: its tags to out + off[b] */
__global__ __launch_bounds__(256) void nrq_held_fill_kernel(ing_rx r, const uint32_t *off, uint32_t *out) {
  __shared__ uint32_t ps[256];
  hl_fill_wg(&r, blockIdx.x, out, off[blockIdx.x], ps);
}

/* count and scan, enqueued: the blocks' exclusive offsets and, behind them, the total, in the reception's list buffer.
 * `count(rx, cnt)` launches the kernel that writes a count per block.
 * That buffer is the output of nrq_ing_lists_kernel (nrq_rx.lists), of whose 2 * nblk + ... words this takes the first nblk + 1,
 * for a held and for a want listing alike.  The rule for every user: write the words anew in the call that reads them, read them
 * on the context's stream within that call, expect nothing of them afterwards.  rx_fetch_lists launches its kernel again before it
 * reads, the fill kernels read the offsets on the same stream before anything later can overwrite them, so the uses cannot meet.
 * A caller that kept the lists on the device across calls would break this. */
template <class Count>
static int rx_list_count(nrq_rx *rx, Count count) {
  nrq_ctx *ctx = rx->ctx;
  const ing_rx &r = rx->r;
  uint32_t *cnt = (uint32_t *)rx->lists;
  HIPCHK(ctx, hipMemsetAsync(cnt + r.nblk, 0, 4u, ctx->stream));
  count(rx, cnt);
  hipLaunchKernelGGL(nrq_tx_scan_kernel, dim3(1), dim3(64), 0, ctx->stream, r.nblk + 1u, cnt);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

/* a listing (`what`: "held", "wanted") of up to two receptions, one behind the other: count per reception, the totals downloaded,
 * then `fill(i, rx, off, out)` launches the kernel that writes reception i's tags to out[off[b] ..] */
template <class Count, class Fill>
static int rx_list(nrq_ctx *ctx, const char *who, const char *what, nrq_rx *const *rxs, int nrx, uint32_t *d_tags, uint32_t cap, uint32_t *h_n,
                   Count count, Fill fill) {
  HIPCHK(ctx, hipSetDevice(ctx->device));
  uint32_t n[2] = {0, 0};
  for (int i = 0; i < nrx; i++) {
    if (!rxs[i]) continue;
    const int rc = rx_list_count(rxs[i], [&](nrq_rx *rx, uint32_t *cnt) { count(i, rx, cnt); });
    if (rc) return rc;
    HIPCHK(ctx, hipMemcpyAsync(&n[i], (uint32_t *)rxs[i]->lists + rxs[i]->r.nblk, 4u, hipMemcpyDeviceToHost, ctx->stream));
  }
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  *h_n = n[0] + n[1];
  if (!d_tags) return 0;
  if (cap < *h_n) return fail(ctx, -1, "%s: %u symbols are %s, d_tags has room for %u", who, *h_n, what, cap);
  uint32_t at = 0;
  for (int i = 0; i < nrx; i++) {
    if (!rxs[i]) continue;
    if (n[i]) fill(i, rxs[i], (const uint32_t *)rxs[i]->lists, d_tags + at);
    at += n[i];
  }
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

/* the held tags of up to two receptions */
static int held_list(nrq_ctx *ctx, const char *who, nrq_rx *const *rxs, int nrx, uint32_t *d_tags, uint32_t cap, uint32_t *h_n) {
  if (!h_n) return fail(ctx, -1, "%s: h_n is NULL", who);
  *h_n = 0;
  hipStream_t st = ctx->stream;
  return rx_list(
      ctx, who, "held", rxs, nrx, d_tags, cap, h_n,
      [&](int, nrq_rx *rx, uint32_t *cnt) { hipLaunchKernelGGL(nrq_held_count_kernel, dim3(rx->r.nblk), dim3(256), 0, st, rx->r, cnt); },
      [&](int, nrq_rx *rx, const uint32_t *off, uint32_t *out) {
        hipLaunchKernelGGL(nrq_held_fill_kernel, dim3(rx->r.nblk), dim3(256), 0, st, rx->r, off, out);
      });
}

extern "C" {

int nrq_rx_held(nrq_rx *rx, uint32_t *d_tags, uint32_t cap, uint32_t *h_n) {
  if (!rx) return -1;
  return held_list(rx->ctx, "nrq_rx_held", &rx, 1, d_tags, cap, h_n);
}

int nrq_orx_held(nrq_orx *rx, uint32_t *d_tags, uint32_t cap, uint32_t *h_n) {
  if (!rx) return -1;
  return held_list(rx->ctx, "nrq_orx_held", rx->rx, 2, d_tags, cap, h_n); /* (class L, then class S: SBN order) */
}

} /* extern "C" */

/* ================================================ what a reception wants (nrq_rx_want / nrq_orx_want, want_body.h) ==== */
/* The listing passes as workgroup bodies of (reception, query, block), as hl_count_wg / hl_fill_wg above. */
/* count: the tags the block lists -> cnt[g].  Rounds of 256 seen words from the word of ESI lo, until `need` wanted ESIs are found
 * or the range ends: in repair mode that is one round unless thousands of symbols are asked for, whatever max_esi */
__device__ __forceinline__ void wn_count_wg(const ing_rx *r, const wn_q *q, uint32_t b, uint32_t *cnt, uint32_t g, uint32_t *ps) {
  const uint32_t t = threadIdx.x, w_end = wn_end(q), need = wn_need(r, q, b);
  uint32_t found = 0;
  for (uint32_t w0 = wn_first(q); w0 < w_end && found < need; w0 += WN_ROUND) { /* (found and need are the same in every thread) */
    const uint32_t w = w0 + t;
    found += wg_sum(ps, t, w < w_end ? ing_popc(wn_bits(r, q, b, w)) : 0u);
    __syncthreads();
  }
  if (t == 0) cnt[g] = min(found, need);
}

/* fill: the block's tags to out[*off ..], ascending -- per round a scan over the 256 words' counts gives each word the rank of its
 * first wanted ESI in the block, and the word writes those of rank below `need` */
__device__ __forceinline__ void wn_fill_wg(const ing_rx *r, const wn_q *q, uint32_t b, uint32_t *out, const uint32_t *off, uint32_t *ps) {
  const uint32_t t = threadIdx.x, w_end = wn_end(q), need = wn_need(r, q, b);
  uint32_t *dst = out + *off;
  uint32_t placed = 0;
  for (uint32_t w0 = wn_first(q); w0 < w_end && placed < need; w0 += WN_ROUND) {
    const uint32_t w = w0 + t;
    const uint32_t bits = w < w_end ? wn_bits(r, q, b, w) : 0u, c = ing_popc(bits);
    wn_put(r, b, w, bits, placed + wg_scan(ps, t, c) - c, need, dst);
    placed += ps[255];
    __syncthreads();
  }
}

/* one workgroup per block: the tags it lists -> cnt[b] */
__global__ __launch_bounds__(256) void nrq_want_count_kernel(ing_rx r, wn_q q, uint32_t *cnt) {
  __shared__ uint32_t ps[256];
  wn_count_wg(&r, &q, blockIdx.x, cnt, blockIdx.x, ps);
}

/* one workgroup per block: its tags to out + off[b] */
__global__ __launch_bounds__(256) void nrq_want_fill_kernel(ing_rx r, wn_q q, const uint32_t *off, uint32_t *out) {
  __shared__ uint32_t ps[256];
  wn_fill_wg(&r, &q, blockIdx.x, out, off + blockIdx.x, ps);
}

/* the wanted tags of up to two receptions */
static int want_list(nrq_ctx *ctx, const char *who, nrq_rx *const *rxs, int nrx, uint32_t flags, uint32_t extra, uint32_t esi_from,
                     uint32_t *d_tags, uint32_t cap, uint32_t *h_n) {
  if (!h_n) return fail(ctx, -1, "%s: h_n is NULL", who);
  *h_n = 0;
  switch (wn_check(flags, extra, esi_from)) {
    case 1: return fail(ctx, -1, "%s: unknown flags 0x%x", who, flags);
    case 2: return fail(ctx, -1, "%s: NRQ_WANT_SOURCE takes neither extra nor esi_from (%u, %u)", who, extra, esi_from);
    case 3: return fail(ctx, -1, "%s: extra %u is above 2^24", who, extra);
    default: break;
  }
  wn_q q[2] = {};
  for (int i = 0; i < nrx; i++)
    if (rxs[i]) q[i] = wn_query(&rxs[i]->r, flags, extra, esi_from);
  hipStream_t st = ctx->stream;
  return rx_list(
      ctx, who, "wanted", rxs, nrx, d_tags, cap, h_n,
      [&](int i, nrq_rx *rx, uint32_t *cnt) { hipLaunchKernelGGL(nrq_want_count_kernel, dim3(rx->r.nblk), dim3(256), 0, st, rx->r, q[i], cnt); },
      [&](int i, nrq_rx *rx, const uint32_t *off, uint32_t *out) {
        hipLaunchKernelGGL(nrq_want_fill_kernel, dim3(rx->r.nblk), dim3(256), 0, st, rx->r, q[i], off, out);
      });
}

extern "C" {

int nrq_rx_want(nrq_rx *rx, uint32_t flags, uint32_t extra, uint32_t esi_from, uint32_t *d_tags, uint32_t cap, uint32_t *h_n) {
  if (!rx) return -1;
  return want_list(rx->ctx, "nrq_rx_want", &rx, 1, flags, extra, esi_from, d_tags, cap, h_n);
}

int nrq_orx_want(nrq_orx *rx, uint32_t flags, uint32_t extra, uint32_t esi_from, uint32_t *d_tags, uint32_t cap, uint32_t *h_n) {
  if (!rx) return -1;
  return want_list(rx->ctx, "nrq_orx_want", rx->rx, 2, flags, extra, esi_from, d_tags, cap, h_n); /* (class L, then class S: SBN order) */
}

} /* extern "C" */

/* ================================================ want and held lists as runs (nrq_rx_want_syms / nrq_rx_held_syms, runs_body.h) ==== */
/* The listings above in the packet form of syms_body.h: (first tag, count) per packet of up to G symbols.  Kernels of their own in
 * the same count / scan / fill shape -- one workgroup of 256 per block, rounds of WN_ROUND words or rows -- so that the one-symbol
 * listings are compiled from the code they always were.  What a round adds to those: the run start entering each word (a max-scan
 * beside the sum-scan), carried across rounds with the symbols found and the packets placed. */

/* inclusive sum-scan of the threads' v and inclusive max-scan of their m in one pass (Hillis-Steele over two arrays of 256 words):
 * returns the sum, *mx = the maximum of threads 0 .. t; ps[255] and pm[255] are the totals.  Ends with a barrier behind its last
 * write, as wg_scan. */
__device__ __forceinline__ uint32_t wg_scan_sum_max(uint32_t *ps, uint32_t *pm, uint32_t t, uint32_t v, uint32_t m, uint32_t *mx) {
  ps[t] = v;
  pm[t] = m;
  __syncthreads();
  for (uint32_t d = 1; d < 256u; d <<= 1) {
    const uint32_t u = t >= d ? ps[t - d] : 0u, x = t >= d ? pm[t - d] : 0u;
    __syncthreads();
    ps[t] += u;
    pm[t] = max(pm[t], x);
    __syncthreads();
  }
  *mx = pm[t];
  return ps[t];
}

/* The bitmap walk of one block (rn_walk): per round each thread takes a word, the scans give it the rank of its first listed ESI
 * and the run start entering it, rn_word_pkts the packets that start in it.  out == NULL: count -- returns the packets, *syms = the
 * symbols listed (both the same in every thread).  Else the packets are written to tags[at ..] / nsym[at ..]; returns `at` behind
 * them. */
__device__ __forceinline__ uint32_t rn_bits_wg(const ing_rx *r, const rn_walk *k, uint32_t G, uint32_t *tags, uint8_t *nsym, uint32_t at,
                                               uint32_t *syms, uint32_t *ps, uint32_t *pm) {
  const uint32_t t = threadIdx.x;
  uint32_t found = 0, pk = 0, S = k->lo;
  for (uint32_t w0 = k->w_first; w0 < k->w_end && found < k->need; w0 += WN_ROUND) { /* (found, need: the same in every thread) */
    const uint32_t w = w0 + t;
    const uint32_t bits = rn_word(r, k, w), c = ing_popc(bits);
    uint32_t mx;
    const uint32_t rank = found + wg_scan_sum_max(ps, pm, t, c, rn_mark(w, bits), &mx) - c;
    const uint32_t Sin = max(S, t ? pm[t - 1u] : 0u);
    const uint32_t tot = ps[255], smax = pm[255];
    __syncthreads();
    const uint32_t n = rn_word_pkts(r, k, G, w, bits, Sin, rank, nullptr, nullptr);
    if (tags) {
      const uint32_t o = at + pk + wg_scan(ps, t, n) - n;
      rn_word_pkts(r, k, G, w, bits, Sin, rank, tags + o, nsym + o);
      pk += ps[255];
    } else {
      pk += wg_sum(ps, t, n);
    }
    __syncthreads();
    found += tot;
    S = max(S, smax);
  }
  if (syms) *syms = min(found, k->need);
  return tags ? at + pk : pk;
}

/* The row walk of one block: the repair part of its held list, a row per thread and round; as rn_bits_wg. */
__device__ __forceinline__ uint32_t rn_rows_wg(const ing_rx *r, uint32_t b, uint32_t G, uint32_t *tags, uint8_t *nsym, uint32_t at, uint32_t *ps,
                                               uint32_t *pm) {
  const uint32_t t = threadIdx.x, nrep = hl_nrep(r, b);
  uint32_t pk = 0, M = 0;
  for (uint32_t q0 = 0; q0 < nrep; q0 += WN_ROUND) {
    const uint32_t q = q0 + t;
    uint32_t mx;
    (void)wg_scan_sum_max(ps, pm, t, 0u, rn_rep_mark(r, b, q, nrep), &mx);
    const uint32_t smax = pm[255];
    __syncthreads();
    const uint32_t n = rn_rep_starts(q, nrep, max(M, mx) - 1u, G) ? 1u : 0u; /* (row 0 begins a run: the maximum is at least 1) */
    if (tags) {
      const uint32_t o = at + pk + wg_scan(ps, t, n) - n;
      if (n) rn_rep_put(r, b, q, nrep, G, tags + o, nsym + o);
      pk += ps[255];
    } else {
      pk += wg_sum(ps, t, n);
    }
    __syncthreads();
    M = max(M, smax);
  }
  return tags ? at + pk : pk;
}

/* one workgroup per block: the packets it lists -> cnt[b], its symbols added to *nsym_total */
__global__ __launch_bounds__(256) void nrq_want_syms_count_kernel(ing_rx r, wn_q q, uint32_t G, uint32_t *cnt, uint32_t *nsym_total) {
  __shared__ uint32_t ps[256], pm[256];
  const rn_walk k = rn_walk_want(&r, &q, blockIdx.x);
  uint32_t syms;
  const uint32_t pk = rn_bits_wg(&r, &k, G, nullptr, nullptr, 0u, &syms, ps, pm);
  if (threadIdx.x == 0) {
    cnt[blockIdx.x] = pk;
    if (syms) atomicAdd(nsym_total, syms);
  }
}

/* one workgroup per block: its packets to tags / nsym + off[b] */
__global__ __launch_bounds__(256) void nrq_want_syms_fill_kernel(ing_rx r, wn_q q, uint32_t G, const uint32_t *off, uint32_t *tags, uint8_t *nsym) {
  __shared__ uint32_t ps[256], pm[256];
  const rn_walk k = rn_walk_want(&r, &q, blockIdx.x);
  (void)rn_bits_wg(&r, &k, G, tags, nsym, off[blockIdx.x], nullptr, ps, pm);
}

/* one workgroup per block: the packets of its source part and of its repair part -> cnt[b], its symbols added to *nsym_total */
__global__ __launch_bounds__(256) void nrq_held_syms_count_kernel(ing_rx r, uint32_t G, uint32_t *cnt, uint32_t *nsym_total) {
  __shared__ uint32_t ps[256], pm[256];
  const uint32_t b = blockIdx.x;
  const rn_walk k = rn_walk_held(&r, b);
  uint32_t syms;
  uint32_t pk = rn_bits_wg(&r, &k, G, nullptr, nullptr, 0u, &syms, ps, pm);
  pk += rn_rows_wg(&r, b, G, nullptr, nullptr, 0u, ps, pm);
  if (threadIdx.x == 0) {
    cnt[b] = pk;
    syms += hl_nrep(&r, b);
    if (syms) atomicAdd(nsym_total, syms);
  }
}

/* one workgroup per block: the packets of its source part, then those of its repair part, to tags / nsym + off[b] */
__global__ __launch_bounds__(256) void nrq_held_syms_fill_kernel(ing_rx r, uint32_t G, const uint32_t *off, uint32_t *tags, uint8_t *nsym) {
  __shared__ uint32_t ps[256], pm[256];
  const uint32_t b = blockIdx.x;
  const rn_walk k = rn_walk_held(&r, b);
  const uint32_t at = rn_bits_wg(&r, &k, G, tags, nsym, off[b], nullptr, ps, pm);
  (void)rn_rows_wg(&r, b, G, tags, nsym, at, ps, pm);
}

/* A listing in packets of up to two receptions, one behind the other (rx_list's shape).  Per reception the list buffer holds, under
 * rx_list_count's rule, nblk + 2 words: the blocks' packet counts, scanned in place into exclusive offsets with the packet total
 * behind them, and the symbol total the count kernel adds up (2 * nblk + nblk * K words are there: enough for any nblk, K >= 1).
 * Both totals of both receptions come down in ONE wait.  `count(i, rx, cnt, nsym_total)` and `fill(i, rx, off, tags, nsym)` launch
 * the kernels. */
template <class Count, class Fill>
static int rx_list_syms(nrq_ctx *ctx, const char *who, const char *what, nrq_rx *const *rxs, int nrx, uint32_t *d_tags, uint8_t *d_nsym,
                        uint32_t cap, uint32_t *h_npkt, uint32_t *h_nsym, Count count, Fill fill) {
  HIPCHK(ctx, hipSetDevice(ctx->device));
  uint32_t n[2][2] = {{0, 0}, {0, 0}}; /* per reception: packets, symbols */
  for (int i = 0; i < nrx; i++) {
    if (!rxs[i]) continue;
    uint32_t *cnt = (uint32_t *)rxs[i]->lists;
    const uint32_t nblk = rxs[i]->r.nblk;
    HIPCHK(ctx, hipMemsetAsync(cnt + nblk, 0, 8u, ctx->stream));
    count(i, rxs[i], cnt, cnt + nblk + 1u);
    hipLaunchKernelGGL(nrq_tx_scan_kernel, dim3(1), dim3(64), 0, ctx->stream, nblk + 1u, cnt);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(n[i], cnt + nblk, 8u, hipMemcpyDeviceToHost, ctx->stream));
  }
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  *h_npkt = n[0][0] + n[1][0];
  if (h_nsym) *h_nsym = n[0][1] + n[1][1];
  if (!d_tags) return 0;
  if (cap < *h_npkt) return fail(ctx, -1, "%s: %u packets are %s, d_tags and d_nsym have room for %u", who, *h_npkt, what, cap);
  uint32_t at = 0;
  for (int i = 0; i < nrx; i++) {
    if (!rxs[i]) continue;
    if (n[i][0]) fill(i, rxs[i], (const uint32_t *)rxs[i]->lists, d_tags + at, d_nsym + at);
    at += n[i][0];
  }
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

/* what every listing in packets refuses beside its one-symbol form's arguments */
static int rn_check(nrq_ctx *ctx, const char *who, uint32_t G, const uint32_t *d_tags, const uint8_t *d_nsym, uint32_t *h_npkt, uint32_t *h_nsym) {
  if (!h_npkt) return fail(ctx, -1, "%s: h_npkt is NULL", who);
  *h_npkt = 0;
  if (h_nsym) *h_nsym = 0;
  if (G == 0 || G > NRQ_PKT_SYMS_MAX) return fail(ctx, -1, "%s: G=%u outside 1..%u", who, G, NRQ_PKT_SYMS_MAX);
  if (!d_tags != !d_nsym) return fail(ctx, -1, "%s: d_tags and d_nsym go together (both, or neither for the counts alone)", who);
  return 0;
}

static int want_list_syms(nrq_ctx *ctx, const char *who, nrq_rx *const *rxs, int nrx, uint32_t flags, uint32_t extra, uint32_t esi_from,
                          uint32_t G, uint32_t *d_tags, uint8_t *d_nsym, uint32_t cap, uint32_t *h_npkt, uint32_t *h_nsym) {
  const int rc = rn_check(ctx, who, G, d_tags, d_nsym, h_npkt, h_nsym);
  if (rc) return rc;
  switch (wn_check(flags, extra, esi_from)) {
    case 1: return fail(ctx, -1, "%s: unknown flags 0x%x", who, flags);
    case 2: return fail(ctx, -1, "%s: NRQ_WANT_SOURCE takes neither extra nor esi_from (%u, %u)", who, extra, esi_from);
    case 3: return fail(ctx, -1, "%s: extra %u is above 2^24", who, extra);
    default: break;
  }
  wn_q q[2] = {};
  for (int i = 0; i < nrx; i++)
    if (rxs[i]) q[i] = wn_query(&rxs[i]->r, flags, extra, esi_from);
  hipStream_t st = ctx->stream;
  return rx_list_syms(
      ctx, who, "wanted", rxs, nrx, d_tags, d_nsym, cap, h_npkt, h_nsym,
      [&](int i, nrq_rx *rx, uint32_t *cnt, uint32_t *tot) {
        hipLaunchKernelGGL(nrq_want_syms_count_kernel, dim3(rx->r.nblk), dim3(256), 0, st, rx->r, q[i], G, cnt, tot);
      },
      [&](int i, nrq_rx *rx, const uint32_t *off, uint32_t *tags, uint8_t *nsym) {
        hipLaunchKernelGGL(nrq_want_syms_fill_kernel, dim3(rx->r.nblk), dim3(256), 0, st, rx->r, q[i], G, off, tags, nsym);
      });
}

static int held_list_syms(nrq_ctx *ctx, const char *who, nrq_rx *const *rxs, int nrx, uint32_t G, uint32_t *d_tags, uint8_t *d_nsym,
                          uint32_t cap, uint32_t *h_npkt, uint32_t *h_nsym) {
  const int rc = rn_check(ctx, who, G, d_tags, d_nsym, h_npkt, h_nsym);
  if (rc) return rc;
  hipStream_t st = ctx->stream;
  return rx_list_syms(
      ctx, who, "held", rxs, nrx, d_tags, d_nsym, cap, h_npkt, h_nsym,
      [&](int, nrq_rx *rx, uint32_t *cnt, uint32_t *tot) {
        hipLaunchKernelGGL(nrq_held_syms_count_kernel, dim3(rx->r.nblk), dim3(256), 0, st, rx->r, G, cnt, tot);
      },
      [&](int, nrq_rx *rx, const uint32_t *off, uint32_t *tags, uint8_t *nsym) {
        hipLaunchKernelGGL(nrq_held_syms_fill_kernel, dim3(rx->r.nblk), dim3(256), 0, st, rx->r, G, off, tags, nsym);
      });
}

extern "C" {

int nrq_rx_want_syms(nrq_rx *rx, uint32_t flags, uint32_t extra, uint32_t esi_from, uint32_t G, uint32_t *d_tags, uint8_t *d_nsym, uint32_t cap,
                     uint32_t *h_npkt, uint32_t *h_nsym) {
  if (!rx) return -1;
  return want_list_syms(rx->ctx, "nrq_rx_want_syms", &rx, 1, flags, extra, esi_from, G, d_tags, d_nsym, cap, h_npkt, h_nsym);
}

int nrq_orx_want_syms(nrq_orx *rx, uint32_t flags, uint32_t extra, uint32_t esi_from, uint32_t G, uint32_t *d_tags, uint8_t *d_nsym, uint32_t cap,
                      uint32_t *h_npkt, uint32_t *h_nsym) {
  if (!rx) return -1;
  return want_list_syms(rx->ctx, "nrq_orx_want_syms", rx->rx, 2, flags, extra, esi_from, G, d_tags, d_nsym, cap, h_npkt, h_nsym);
}

int nrq_rx_held_syms(nrq_rx *rx, uint32_t G, uint32_t *d_tags, uint8_t *d_nsym, uint32_t cap, uint32_t *h_npkt, uint32_t *h_nsym) {
  if (!rx) return -1;
  return held_list_syms(rx->ctx, "nrq_rx_held_syms", &rx, 1, G, d_tags, d_nsym, cap, h_npkt, h_nsym);
}

int nrq_orx_held_syms(nrq_orx *rx, uint32_t G, uint32_t *d_tags, uint8_t *d_nsym, uint32_t cap, uint32_t *h_npkt, uint32_t *h_nsym) {
  if (!rx) return -1;
  return held_list_syms(rx->ctx, "nrq_orx_held_syms", rx->rx, 2, G, d_tags, d_nsym, cap, h_npkt, h_nsym); /* (class L, then class S) */
}

} /* extern "C" */

/* ================================================ reception sets (nrq_rxset_*, ingest_set_body.h) ==== */
/* The seven passes of the ingest above over a member table in device memory: one chain of kernels for the packets of all
 * members.  Per-block passes run one workgroup per GLOBAL block, find its member from the block offsets and run the single
 * form's workgroup body on it; the copy pass is the single form's kernel; per-packet and per-tile passes are kernels of their own
 * (they read the table and count per global block in LDS sized by the set's block total: dynamic, a set of 256 blocks pays what
 * a reception of 256 blocks pays). */
__global__ __launch_bounds__(256) void nrq_ings_first_kernel(const ings_tab *__restrict__ t, ings_call s) {
  __shared__ uint32_t skey[INGS_MAX_MEMBERS], ssbn0[INGS_MAX_MEMBERS], scnt[INGS_MAX_MEMBERS], sobjZ[INGS_MAX_MEMBERS];
  const uint32_t nmem = t->nmem, i = threadIdx.x;
  if (i < nmem) { skey[i] = t->key[i]; ssbn0[i] = t->sbn0[i]; scnt[i] = t->cnt[i]; sobjZ[i] = t->objZ[i]; }
  __syncthreads();
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= s.c.n) return;
  uint32_t key, tag;
  ings_decode(&s, k, &key, &tag);
  ings_first(t, &s, k, tag, ings_find(skey, ssbn0, scnt, sobjZ, nmem, key, tag >> 24));
}

__global__ __launch_bounds__(256) void nrq_ings_done_kernel(const ings_tab *__restrict__ t) {
  __shared__ uint32_t smx[256], scnt[256];
  uint32_t b;
  const ing_rx *r = lss_block(t, blockIdx.x, &b);
  ing_done_wg(r, b, smx, scnt);
}

/* dynamic LDS: t->nblk counters */
__global__ __launch_bounds__(256) void nrq_ings_hist_kernel(const ings_tab *__restrict__ t, ings_call s) {
  extern __shared__ uint32_t ings_h[];
  const uint32_t i = threadIdx.x, k = blockIdx.x * ING_TILE + i, nb = t->nblk;
  for (uint32_t g = i; g < nb; g += 256u) ings_h[g] = 0;
  __syncthreads();
  if (k < s.c.n) {
    const uint32_t g = ings_cand(t, &s, k);
    if (g != ING_NONE) atomicAdd(&ings_h[g], 1u);
  }
  __syncthreads();
  for (uint32_t g = i; g < nb; g += 256u) s.c.base[(size_t)g * s.c.ntiles + blockIdx.x] = ings_h[g];
}

__global__ __launch_bounds__(256) void nrq_ings_scan_kernel(const ings_tab *__restrict__ t, ings_call s) {
  __shared__ uint32_t ps[256];
  uint32_t b;
  const ing_rx *r = lss_block(t, blockIdx.x, &b);
  ing_scan_wg(r, b, s.c.base + (size_t)blockIdx.x * s.c.ntiles, s.c.ntiles, ps);
}

/* dynamic LDS: 4 * t->nblk counters (per wave, per global block).  The ranking is ing_rank_wg with the global block in place of
 * the local one: a wave may hold candidates of several members. */
__global__ __launch_bounds__(256) void nrq_ings_classify_kernel(const ings_tab *__restrict__ t, ings_call s) {
  extern __shared__ uint32_t ings_wc[];
  const uint32_t i = threadIdx.x, k = blockIdx.x * ING_TILE + i, nb = t->nblk;
  for (uint32_t j = i; j < 4u * nb; j += 256u) ings_wc[j] = 0;
  __syncthreads();
  const uint32_t g = k < s.c.n ? ings_cand(t, &s, k) : ING_NONE;
  const uint32_t row = ing_rank_wg(ings_wc, nb, g, s.c.base, s.c.ntiles);
  if (k < s.c.n) ings_classify(t, &s, k, row);
}

__global__ __launch_bounds__(256) void nrq_ings_fold_kernel(const ings_tab *__restrict__ t, ings_call s) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k < s.c.n) ings_fold(t, &s, k);
}

static_assert(NRQ_RXSET_MAX_MEMBERS == INGS_MAX_MEMBERS && NRQ_RXSET_MAX_BLOCKS == INGS_MAX_BLOCKS, "the header's caps are the kernels'");

struct rxset_member {
  uint32_t key;
  nrq_rx *rx;
  uint32_t objZ; /* a block class of an attached object of Z blocks; 0: a plain reception */
};

struct nrq_rxset {
  nrq_ctx *ctx;
  uint32_t T;
  std::vector<rxset_member> mem; /* sorted by (key, sbn0): the order of the device table */
  uint32_t nblk;                 /* blocks over all members */
  void *tab;                     /* struct ings_tab in device memory */
  DevScratch scratch;            /* per-call arrays */
  void *lists;                   /* the listing passes' output (lists_set_body.h), sized for the worst case of the members.  The rule of
                                  * rx_list_count holds: written anew by every call that reads it, read on the context's stream
                                  * within that call, nothing expected of it afterwards */
  size_t lists_cap;
};

/* the member table as `mem` has it, into device memory.  Waits for the stream first: an ingest enqueued before still reads the
 * old table. */
static int rxset_upload(nrq_rxset *set, const std::vector<rxset_member> &mem) {
  nrq_ctx *ctx = set->ctx;
  std::vector<ings_tab> hv(1);
  ings_tab &h = hv[0];
  memset(&h, 0, sizeof(h));
  h.nmem = (uint32_t)mem.size();
  for (uint32_t i = 0; i < h.nmem; i++) {
    const ing_rx &r = mem[i].rx->r;
    h.key[i] = mem[i].key; h.sbn0[i] = r.sbn0; h.cnt[i] = r.nblk; h.objZ[i] = mem[i].objZ;
    h.blk0[i] = h.nblk;
    h.nblk += r.nblk;
    h.r[i] = r;
  }
  h.blk0[h.nmem] = h.nblk;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  HIPCHK(ctx, hipMemcpy(set->tab, &h, sizeof(h), hipMemcpyHostToDevice));
  return 0;
}

/* take `mem` as the set's members (sorted here); on failure the set keeps the ones it had */
static int rxset_commit(nrq_rxset *set, std::vector<rxset_member> &mem) {
  std::sort(mem.begin(), mem.end(), [](const rxset_member &a, const rxset_member &b) {
    return a.key != b.key ? a.key < b.key : a.rx->r.sbn0 < b.rx->r.sbn0;
  });
  /* the list buffer: every block's K + rep_cap list words at most, gaps and offsets of all blocks, the total */
  size_t words = 1;
  for (const rxset_member &m : mem) words += (size_t)m.rx->r.nblk * ((size_t)m.rx->r.K + m.rx->r.rep_cap + 2u);
  void *lists = nullptr;
  int rc = words * 4u > set->lists_cap ? nrq_dev_alloc(set->ctx, words * 4u, &lists) : 0;
  if (rc) return rc;
  rc = rxset_upload(set, mem);
  if (rc) {
    if (lists) nrq_dev_free(set->ctx, lists);
    return rc;
  }
  if (lists) { /* (the upload has waited for the stream: nothing reads the old buffer any more) */
    if (set->lists) nrq_dev_free(set->ctx, set->lists);
    set->lists = lists;
    set->lists_cap = words * 4u;
  }
  for (const rxset_member &m : set->mem) m.rx->set = nullptr;
  set->mem.swap(mem);
  set->nblk = 0;
  for (const rxset_member &m : set->mem) { m.rx->set = set; set->nblk += m.rx->r.nblk; }
  return 0;
}

/* a reception goes away (nrq_rx_destroy): it leaves its set first */
static void rxset_drop(nrq_rx *rx) {
  nrq_rxset *set = rx->set;
  std::vector<rxset_member> mem;
  for (const rxset_member &m : set->mem)
    if (m.rx != rx) mem.push_back(m);
  if (rxset_commit(set, mem) != 0) { /* (the table could not be written: an empty host list keeps every later ingest off the stale one) */
    for (const rxset_member &m : set->mem) m.rx->set = nullptr;
    set->mem.clear();
    set->nblk = 0;
  }
}

static int rxset_attach(nrq_rxset *set, const char *who, uint32_t key, nrq_rx *const *rxs, int nrx, uint32_t objZ) {
  nrq_ctx *ctx = set->ctx;
  std::vector<rxset_member> mem = set->mem;
  uint32_t nblk = set->nblk;
  for (int i = 0; i < nrx; i++) {
    nrq_rx *rx = rxs[i];
    if (!rx) continue;
    const ing_rx &r = rx->r;
    if (rx->ctx != ctx) return fail(ctx, -1, "%s: the reception belongs to another context", who);
    if (r.T != set->T) return fail(ctx, -1, "%s: the reception's T %u is not the set's %u", who, r.T, set->T);
    if (rx->set) return fail(ctx, -1, "%s: the reception is in a set already", who);
    for (const rxset_member &m : set->mem) {
      if (m.key != key) continue;
      if (objZ || m.objZ) return fail(ctx, -1, "%s: key %u has members already, and an object owns its key", who, key);
      const ing_rx &o = m.rx->r;
      if (r.sbn0 < o.sbn0 + o.nblk && o.sbn0 < r.sbn0 + r.nblk)
        return fail(ctx, -1, "%s: SBNs %u..%u under key %u overlap a member's %u..%u", who, r.sbn0, r.sbn0 + r.nblk - 1u, key, o.sbn0,
                    o.sbn0 + o.nblk - 1u);
    }
    if (mem.size() >= NRQ_RXSET_MAX_MEMBERS) return fail(ctx, -1, "%s: a set holds at most %u receptions", who, NRQ_RXSET_MAX_MEMBERS);
    if (nblk + r.nblk > NRQ_RXSET_MAX_BLOCKS) return fail(ctx, -1, "%s: a set holds at most %u blocks", who, NRQ_RXSET_MAX_BLOCKS);
    nblk += r.nblk;
    mem.push_back(rxset_member{key, rx, objZ});
  }
  if (mem.size() == set->mem.size()) return fail(ctx, -1, "%s: nothing to attach", who);
  return rxset_commit(set, mem);
}

extern "C" {

int nrq_rxset_create(nrq_ctx *ctx, uint32_t T, nrq_rxset **out) {
  if (!ctx) return -1;
  if (!out) return fail(ctx, -1, "nrq_rxset_create: out is NULL");
  *out = nullptr;
  if (T == 0) return fail(ctx, -1, "nrq_rxset_create: T is 0");
  nrq_rxset *set = new (std::nothrow) nrq_rxset();
  if (!set) return fail(ctx, -1, "nrq_rxset_create: out of host memory");
  set->ctx = ctx;
  set->T = T;
  const int rc = nrq_dev_alloc(ctx, sizeof(ings_tab), &set->tab);
  if (rc) {
    delete set;
    return rc;
  }
  *out = set;
  return 0;
}

void nrq_rxset_destroy(nrq_rxset *set) {
  if (!set) return;
  nrq_ctx *ctx = set->ctx;
  for (const rxset_member &m : set->mem) m.rx->set = nullptr;
  (void)hipStreamSynchronize(ctx->stream); /* (the pool hands freed blocks out again at once) */
  for (void *p : {set->tab, set->lists})
    if (p) nrq_dev_free(ctx, p);
  set->scratch.release(ctx);
  delete set;
}

int nrq_rxset_attach(nrq_rxset *set, uint32_t key, nrq_rx *rx) {
  if (!set) return -1;
  if (!rx) return fail(set->ctx, -1, "nrq_rxset_attach: the reception is NULL");
  return rxset_attach(set, "nrq_rxset_attach", key, &rx, 1, 0);
}

int nrq_rxset_attach_obj(nrq_rxset *set, uint32_t key, nrq_orx *orx) {
  if (!set) return -1;
  if (!orx) return fail(set->ctx, -1, "nrq_rxset_attach_obj: the object receiver is NULL");
  return rxset_attach(set, "nrq_rxset_attach_obj", key, orx->rx, 2, orx->prm.Z);
}

int nrq_rxset_detach(nrq_rxset *set, uint32_t key) {
  if (!set) return -1;
  std::vector<rxset_member> mem;
  for (const rxset_member &m : set->mem)
    if (m.key != key) mem.push_back(m);
  if (mem.size() == set->mem.size()) return fail(set->ctx, -1, "nrq_rxset_detach: no member under key %u", key);
  return rxset_commit(set, mem);
}

int nrq_rxset_add(nrq_rxset *set, const void *d_pkts, size_t pkt_stride, const uint32_t *d_keys, const uint32_t *d_tags, uint32_t n,
                  uint32_t flags, int32_t *d_results) {
  if (!set) return -1;
  nrq_ctx *ctx = set->ctx;
  const bool inl = (flags & NRQ_RX_TAG_INLINE) != 0, kinl = (flags & NRQ_RX_KEY_INLINE) != 0;
  if (flags & ~(uint32_t)(NRQ_RX_TAG_INLINE | NRQ_RX_KEY_INLINE)) return fail(ctx, -1, "nrq_rxset_add: unknown flags 0x%x", flags);
  if (kinl && !inl) return fail(ctx, -1, "nrq_rxset_add: NRQ_RX_KEY_INLINE needs NRQ_RX_TAG_INLINE");
  if (kinl && d_keys) return fail(ctx, -1, "nrq_rxset_add: give either d_keys or NRQ_RX_KEY_INLINE");
  if (n == 0 || set->mem.empty()) return 0;
  const uint32_t poff = kinl ? 8u : inl ? 4u : 0u;
  ings_call s{};
  ing_call &c = s.c;
  uint8_t *mem; /* (the packets' members: the set's own array, behind the call's) */
  const int rc = ing_call_of(ctx, set->scratch, "nrq_rxset_add", d_pkts, pkt_stride, d_tags, n, 0, (size_t)set->T + poff, inl, set->nblk,
                             d_results, (size_t)n * 4u, &c, &mem);
  if (rc) return rc;
  s.keys = d_keys;
  s.key_inline = kinl ? 1u : 0u;
  s.mem = (uint32_t *)mem;
  const ings_tab *t = (const ings_tab *)set->tab;
  hipStream_t st = ctx->stream;
  const uint32_t g = (n + 255u) / 256u, nb = set->nblk;
  hipLaunchKernelGGL(nrq_ings_first_kernel, dim3(g), dim3(256), 0, st, t, s);
  hipLaunchKernelGGL(nrq_ings_done_kernel, dim3(nb), dim3(256), 0, st, t);
  hipLaunchKernelGGL(nrq_ings_hist_kernel, dim3(c.ntiles), dim3(256), nb * 4u, st, t, s);
  hipLaunchKernelGGL(nrq_ings_scan_kernel, dim3(nb), dim3(256), 0, st, t, s);
  hipLaunchKernelGGL(nrq_ings_classify_kernel, dim3(c.ntiles), dim3(256), nb * 16u, st, t, s);
  hipLaunchKernelGGL(nrq_ing_copy_kernel, dim3((n + 3u) / 4u), dim3(256), 0, st, c.pkts, c.pkt_stride, (const uint64_t *)c.dst, n, set->T, poff);
  hipLaunchKernelGGL(nrq_ings_fold_kernel, dim3(g), dim3(256), 0, st, t, s);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

} /* extern "C" */

/* ================================================ a set's counts, lists and decode (lists_set_body.h, rxset_plan.h) ==== */
/* nrq_rx_counts, nrq_rx_lists and nrq_rx_decode over all members of a set at once, in the order of the table's global block
 * numbers.  The lists are made as the held / want listings are -- count, one scan, fill -- because the single form's serial sum
 * over all earlier blocks, in one lane of every workgroup, is 1024 dependent loads through the table at a full set. */
__global__ __launch_bounds__(256) void nrq_ings_counts_kernel(const ings_tab *__restrict__ t, uint32_t *__restrict__ out) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x, nb = t->nblk;
  if (g >= nb) return;
  uint32_t ng, nr;
  lss_counts(t, g, &ng, &nr);
  out[g] = ng;
  out[nb + g] = nr;
}

__global__ __launch_bounds__(256) void nrq_ings_lists_count_kernel(const ings_tab *__restrict__ t, uint32_t *__restrict__ buf) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g < t->nblk) lss_list_count(t, g, buf);
}

/* counts -> exclusive offsets, in place, n <= 1025 entries (nrq_tx_scan_kernel is one lane over at most 257): one workgroup */
__global__ __launch_bounds__(256) void nrq_ings_lists_scan_kernel(uint32_t n, uint32_t *cnt) {
  __shared__ uint32_t ps[256];
  (void)wg_scan_runs(ps, threadIdx.x, cnt, n, 0u);
}

/* one workgroup per global block: its list to the block's offset behind the 2 * nblk + 1 words of gaps and offsets */
__global__ __launch_bounds__(256) void nrq_ings_lists_fill_kernel(const ings_tab *__restrict__ t, uint32_t *buf) {
  __shared__ uint32_t ps[256];
  const uint32_t g = blockIdx.x, nb = t->nblk;
  uint32_t b;
  const ing_rx *r = lss_block(t, g, &b);
  ing_lists_fill_wg(r, b, buf + 2u * nb + 1u + buf[nb + g], ps);
}

struct ings_mask { uint32_t w[INGS_MAX_BLOCKS / 32u]; }; /* a bit per global block of the set */

/* nrq_ing_mark_kernel over the table: one workgroup per global block, at work where the block's bit is set */
__global__ __launch_bounds__(256) void nrq_ings_mark_kernel(const ings_tab *__restrict__ t, ings_mask m) {
  const uint32_t g = blockIdx.x;
  if (!((m.w[g >> 5] >> (g & 31u)) & 1u)) return;
  uint32_t b;
  const ing_rx *r = lss_block(t, g, &b);
  ing_mark_wg(r, b);
}

/* the lists of all members: head = gaps[nb], offsets[nb + 1] (the last one the total), lists = exactly the list words.  One
 * listing pass; the head comes down first, then the list bytes, as in rx_fetch_lists. */
static int rxset_fetch_lists(nrq_rxset *set, std::vector<uint32_t> &head, std::vector<uint32_t> &lists) {
  nrq_ctx *ctx = set->ctx;
  const uint32_t nb = set->nblk;
  const ings_tab *t = (const ings_tab *)set->tab;
  uint32_t *buf = (uint32_t *)set->lists;
  hipLaunchKernelGGL(nrq_ings_lists_count_kernel, dim3((nb + 255u) / 256u), dim3(256), 0, ctx->stream, t, buf);
  hipLaunchKernelGGL(nrq_ings_lists_scan_kernel, dim3(1), dim3(256), 0, ctx->stream, nb + 1u, buf + nb);
  hipLaunchKernelGGL(nrq_ings_lists_fill_kernel, dim3(nb), dim3(256), 0, ctx->stream, t, buf);
  HIPCHK(ctx, hipGetLastError());
  head.assign(2u * (size_t)nb + 1u, 0);
  HIPCHK(ctx, hipMemcpyAsync(head.data(), buf, head.size() * 4u, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  const size_t total = head[2u * (size_t)nb];
  lists.assign(total ? total : 1, 0);
  if (total) {
    HIPCHK(ctx, hipMemcpyAsync(lists.data(), buf + 2u * (size_t)nb + 1u, total * 4u, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  }
  return 0;
}

extern "C" {

int nrq_rxset_blocks(nrq_rxset *set, uint32_t *h_keys, uint32_t *h_sbn, uint32_t cap, uint32_t *h_n) {
  if (!set) return -1;
  if (!h_n) return fail(set->ctx, -1, "nrq_rxset_blocks: h_n is NULL");
  *h_n = set->nblk;
  if (!h_keys && !h_sbn) return 0;
  if (cap < set->nblk) return fail(set->ctx, -1, "nrq_rxset_blocks: the set has %u blocks, the arrays have room for %u", set->nblk, cap);
  uint32_t j = 0;
  for (const rxset_member &m : set->mem)
    for (uint32_t b = 0; b < m.rx->r.nblk; b++, j++) {
      if (h_keys) h_keys[j] = m.key;
      if (h_sbn) h_sbn[j] = m.rx->r.sbn0 + b;
    }
  return 0;
}

int nrq_rxset_counts(nrq_rxset *set, uint32_t *h_nlost, uint32_t *h_nrep) {
  if (!set) return -1;
  nrq_ctx *ctx = set->ctx;
  const uint32_t nb = set->nblk;
  if (nb == 0) return 0;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(nrq_ings_counts_kernel, dim3((nb + 255u) / 256u), dim3(256), 0, ctx->stream, (const ings_tab *)set->tab, (uint32_t *)set->lists);
  HIPCHK(ctx, hipGetLastError());
  std::vector<uint32_t> cnt(2u * (size_t)nb);
  HIPCHK(ctx, hipMemcpyAsync(cnt.data(), set->lists, cnt.size() * 4u, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (h_nlost) memcpy(h_nlost, cnt.data(), (size_t)nb * 4u);
  if (h_nrep) memcpy(h_nrep, cnt.data() + nb, (size_t)nb * 4u);
  return 0;
}

int nrq_rxset_lists(nrq_rxset *set, uint32_t *h_nlost, uint32_t *h_nrep, uint32_t *h_lists, size_t cap, size_t *h_total) {
  if (!set) return -1;
  nrq_ctx *ctx = set->ctx;
  const uint32_t nb = set->nblk;
  if (h_total) *h_total = 0;
  if (nb == 0) return 0;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::vector<uint32_t> head, lists;
  const int rc = rxset_fetch_lists(set, head, lists);
  if (rc) return rc;
  const size_t total = head[2u * (size_t)nb];
  if (h_total) *h_total = total;
  for (uint32_t j = 0; j < nb; j++) {
    if (h_nlost) h_nlost[j] = head[j];
    if (h_nrep) h_nrep[j] = head[nb + j + 1u] - head[nb + j] - head[j];
  }
  if (!h_lists) return 0;
  if (cap < total) return fail(ctx, -1, "nrq_rxset_lists: the lists have %zu words, h_lists has room for %zu", total, cap);
  memcpy(h_lists, lists.data(), total * 4u);
  return 0;
}

int nrq_rxset_decode(nrq_rxset *set, int *h_status, uint32_t *h_used) {
  if (!set) return -1;
  nrq_ctx *ctx = set->ctx;
  if (!h_status) return fail(ctx, -1, "nrq_rxset_decode: h_status is NULL");
  const uint32_t nb = set->nblk;
  if (nb == 0) return 0;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::vector<uint32_t> head;
  rx_listing L;
  int rc = rxset_fetch_lists(set, head, L.words);
  if (rc) return rc;
  std::vector<rxset_plan_member> pm(set->mem.size());
  uint32_t j = 0;
  for (size_t m = 0; m < set->mem.size(); m++) {
    nrq_rx *rx = set->mem[m].rx;
    pm[m] = rxset_plan_member{rx->r.K, rx->Kp, rx->r.max_esi, rx->relay ? 1u : 0u};
    for (uint32_t b = 0; b < rx->r.nblk; b++, j++) L.add(rx, (uint32_t)m, b, head[j], head[nb + j + 1u] - head[nb + j] - head[j], head[nb + j]);
  }
  std::vector<uint32_t> recovered;
  rc = rx_decode_listed(ctx, L, rxset_plan(pm.data(), L.member.data(), L.ng.data(), L.nr.data(), nb), h_status, h_used, recovered);
  if (!recovered.empty()) { /* (also behind a failed chunk: the chunks before it stay marked, the error text is that chunk's) */
    ings_mask mask{};
    for (uint32_t g : recovered) mask.w[g >> 5] |= 1u << (g & 31u);
    hipLaunchKernelGGL(nrq_ings_mark_kernel, dim3(nb), dim3(256), 0, ctx->stream, (const ings_tab *)set->tab, mask);
    if (!rc) HIPCHK(ctx, hipGetLastError());
  }
  return rc;
}

} /* extern "C" */

/* ================================================ what a set's members want and hold (nrq_rxset_want / _held, want_set_body.h) ==== */
/* nrq_rx_want and nrq_rx_held over all members of a set at once, with the member's key beside every tag: three launches and one
 * download for the whole set where the members' own calls make three launches, a download and a wait EACH.  One workgroup per
 * GLOBAL block finds its member (lss_block: wave-uniform, the table is read through the uniform pointer) and runs the single
 * form's workgroup body on it -- a want call forms that member's wn_q from the call's three words, since K, max_esi and rep_cap
 * are the member's own.  The counts and offsets are the first nb + 1 words of the set's list buffer, under rx_list_count's rule. */
__global__ __launch_bounds__(256) void nrq_ings_want_count_kernel(const ings_tab *__restrict__ t, wns_call c, uint32_t *__restrict__ cnt) {
  __shared__ uint32_t ps[256];
  const uint32_t g = blockIdx.x;
  uint32_t b;
  const ing_rx *r = lss_block(t, g, &b);
  const wn_q q = wns_query(r, &c);
  wn_count_wg(r, &q, b, cnt, g, ps);
  if (threadIdx.x == 0) wns_count_end(t, g, cnt);
}

__global__ __launch_bounds__(256) void nrq_ings_held_count_kernel(const ings_tab *__restrict__ t, uint32_t *__restrict__ cnt) {
  __shared__ uint32_t ps[256];
  const uint32_t g = blockIdx.x;
  uint32_t b;
  const ing_rx *r = lss_block(t, g, &b);
  hl_count_wg(r, b, cnt, g, ps);
  if (threadIdx.x == 0) wns_count_end(t, g, cnt);
}

/* one workgroup per global block: its tags to tags[off[g] .. off[g + 1]), then its key to the same entries of keys (nullable) --
 * all 256 threads stride over them, so the key stores are coalesced instead of one beside every scattered tag store.  A block
 * that lists nothing (complete, or nothing held) is left at once. */
__global__ __launch_bounds__(256) void nrq_ings_want_fill_kernel(const ings_tab *__restrict__ t, wns_call c, const uint32_t *__restrict__ off,
                                                                 uint32_t *__restrict__ tags, uint32_t *__restrict__ keys) {
  __shared__ uint32_t ps[256];
  const uint32_t g = blockIdx.x, lo = off[g], hi = off[g + 1u];
  if (lo == hi) return; /* (the same in every thread) */
  uint32_t b, key;
  const ing_rx *r = wns_block(t, g, &b, &key);
  const wn_q q = wns_query(r, &c);
  wn_fill_wg(r, &q, b, tags, off + g, ps);
  if (keys) wns_put_keys(keys, lo, hi, key, threadIdx.x, 256u);
}

__global__ __launch_bounds__(256) void nrq_ings_held_fill_kernel(const ings_tab *__restrict__ t, const uint32_t *__restrict__ off,
                                                                 uint32_t *__restrict__ tags, uint32_t *__restrict__ keys) {
  __shared__ uint32_t ps[256];
  const uint32_t g = blockIdx.x, lo = off[g], hi = off[g + 1u];
  if (lo == hi) return;
  uint32_t b, key;
  const ing_rx *r = wns_block(t, g, &b, &key);
  hl_fill_wg(r, b, tags, lo, ps);
  if (keys) wns_put_keys(keys, lo, hi, key, threadIdx.x, 256u);
}

/* a listing (`what`: "held", "wanted") of all members with keys, shaped like rx_list: `count(cnt)` launches the kernel that
 * writes a count per global block and 0 behind them, ONE scan, ONE download (the nb + 1 offsets when the per-block counts are
 * asked for, else the total alone) and wait, then `fill(off)` launches the kernel that writes tags and keys */
template <class Count, class Fill>
static int rxset_list(nrq_rxset *set, const char *who, const char *what, uint32_t *d_tags, uint32_t cap, uint32_t *h_cnt, uint32_t *h_n,
                      Count count, Fill fill) {
  nrq_ctx *ctx = set->ctx;
  const uint32_t nb = set->nblk;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  uint32_t *off = (uint32_t *)set->lists;
  count(off);
  hipLaunchKernelGGL(nrq_ings_lists_scan_kernel, dim3(1), dim3(256), 0, ctx->stream, nb + 1u, off);
  HIPCHK(ctx, hipGetLastError());
  std::vector<uint32_t> h(h_cnt ? (size_t)nb + 1u : 1u, 0);
  HIPCHK(ctx, hipMemcpyAsync(h.data(), h_cnt ? off : off + nb, h.size() * 4u, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  *h_n = h.back();
  if (h_cnt)
    for (uint32_t g = 0; g < nb; g++) h_cnt[g] = h[g + 1u] - h[g];
  if (!d_tags) return 0;
  if (cap < *h_n) return fail(ctx, -1, "%s: %u symbols are %s, d_tags has room for %u", who, *h_n, what, cap);
  if (*h_n == 0) return 0;
  fill((const uint32_t *)off);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

extern "C" {

int nrq_rxset_want(nrq_rxset *set, uint32_t flags, uint32_t extra, uint32_t esi_from, uint32_t *d_keys, uint32_t *d_tags, uint32_t cap,
                   uint32_t *h_cnt, uint32_t *h_n) {
  if (!set) return -1;
  nrq_ctx *ctx = set->ctx;
  const char *who = "nrq_rxset_want";
  if (!h_n) return fail(ctx, -1, "%s: h_n is NULL", who);
  *h_n = 0;
  switch (wn_check(flags, extra, esi_from)) {
    case 1: return fail(ctx, -1, "%s: unknown flags 0x%x", who, flags);
    case 2: return fail(ctx, -1, "%s: NRQ_WANT_SOURCE takes neither extra nor esi_from (%u, %u)", who, extra, esi_from);
    case 3: return fail(ctx, -1, "%s: extra %u is above 2^24", who, extra);
    default: break;
  }
  if (d_keys && !d_tags) return fail(ctx, -1, "%s: d_keys without d_tags", who);
  const uint32_t nb = set->nblk;
  if (nb == 0) return 0;
  const ings_tab *t = (const ings_tab *)set->tab;
  const wns_call c{flags, extra, esi_from};
  hipStream_t st = ctx->stream;
  return rxset_list(
      set, who, "wanted", d_tags, cap, h_cnt, h_n,
      [&](uint32_t *cnt) { hipLaunchKernelGGL(nrq_ings_want_count_kernel, dim3(nb), dim3(256), 0, st, t, c, cnt); },
      [&](const uint32_t *off) { hipLaunchKernelGGL(nrq_ings_want_fill_kernel, dim3(nb), dim3(256), 0, st, t, c, off, d_tags, d_keys); });
}

int nrq_rxset_held(nrq_rxset *set, uint32_t *d_keys, uint32_t *d_tags, uint32_t cap, uint32_t *h_cnt, uint32_t *h_n) {
  if (!set) return -1;
  nrq_ctx *ctx = set->ctx;
  const char *who = "nrq_rxset_held";
  if (!h_n) return fail(ctx, -1, "%s: h_n is NULL", who);
  *h_n = 0;
  if (d_keys && !d_tags) return fail(ctx, -1, "%s: d_keys without d_tags", who);
  const uint32_t nb = set->nblk;
  if (nb == 0) return 0;
  const ings_tab *t = (const ings_tab *)set->tab;
  hipStream_t st = ctx->stream;
  return rxset_list(
      set, who, "held", d_tags, cap, h_cnt, h_n,
      [&](uint32_t *cnt) { hipLaunchKernelGGL(nrq_ings_held_count_kernel, dim3(nb), dim3(256), 0, st, t, cnt); },
      [&](const uint32_t *off) { hipLaunchKernelGGL(nrq_ings_held_fill_kernel, dim3(nb), dim3(256), 0, st, t, off, d_tags, d_keys); });
}

} /* extern "C" */

/* ================================================ a set's want and held lists as runs (nrq_rxset_want_syms / _held_syms) ==== */
/* The two layers above put together: nrq_rx_want_syms and nrq_rx_held_syms over all members of a set at once, with the member's
 * key beside every packet -- the (keys, tags, nsym) form nrq_txset_emit_syms takes.  Kernels of their own in the count / scan /
 * fill shape of nrq_ings_want_*_kernel, so that the one-symbol set listings and the single-reception runs kernels are compiled
 * from the code they always were: one workgroup of 256 per GLOBAL block finds its member and key (lss_block / wns_block), forms
 * that member's wn_q (wns_query) and runs the workgroup walks of the single form on it (rn_bits_wg, for held rn_rows_wg behind
 * it).  The set's list buffer holds, under rx_list_count's rule, nb + 2 words: the blocks' packet counts, scanned in place into
 * exclusive offsets with the packet total behind them, and the symbol total the count kernel adds up. */
__global__ __launch_bounds__(256) void nrq_ings_want_syms_count_kernel(const ings_tab *__restrict__ t, wns_call c, uint32_t G,
                                                                       uint32_t *__restrict__ cnt, uint32_t *__restrict__ nsym_total) {
  __shared__ uint32_t ps[256], pm[256];
  const uint32_t g = blockIdx.x;
  uint32_t b;
  const ing_rx *r = lss_block(t, g, &b);
  const wn_q q = wns_query(r, &c);
  const rn_walk k = rn_walk_want(r, &q, b);
  uint32_t syms;
  const uint32_t pk = rn_bits_wg(r, &k, G, nullptr, nullptr, 0u, &syms, ps, pm);
  if (threadIdx.x == 0) {
    cnt[g] = pk;
    wns_count_end(t, g, cnt);
    if (syms) atomicAdd(nsym_total, syms);
  }
}

__global__ __launch_bounds__(256) void nrq_ings_held_syms_count_kernel(const ings_tab *__restrict__ t, uint32_t G, uint32_t *__restrict__ cnt,
                                                                       uint32_t *__restrict__ nsym_total) {
  __shared__ uint32_t ps[256], pm[256];
  const uint32_t g = blockIdx.x;
  uint32_t b;
  const ing_rx *r = lss_block(t, g, &b);
  const rn_walk k = rn_walk_held(r, b);
  uint32_t syms;
  uint32_t pk = rn_bits_wg(r, &k, G, nullptr, nullptr, 0u, &syms, ps, pm);
  pk += rn_rows_wg(r, b, G, nullptr, nullptr, 0u, ps, pm);
  if (threadIdx.x == 0) {
    cnt[g] = pk;
    wns_count_end(t, g, cnt);
    syms += hl_nrep(r, b);
    if (syms) atomicAdd(nsym_total, syms);
  }
}

/* one workgroup per global block: its packets to tags / nsym [off[g] .. off[g + 1]), then its key to the same entries of keys
 * (nullable), the stores coalesced as in nrq_ings_want_fill_kernel.  A block that lists nothing is left at once. */
__global__ __launch_bounds__(256) void nrq_ings_want_syms_fill_kernel(const ings_tab *__restrict__ t, wns_call c, uint32_t G,
                                                                      const uint32_t *__restrict__ off, uint32_t *__restrict__ tags,
                                                                      uint8_t *__restrict__ nsym, uint32_t *__restrict__ keys) {
  __shared__ uint32_t ps[256], pm[256];
  const uint32_t g = blockIdx.x, lo = off[g], hi = off[g + 1u];
  if (lo == hi) return; /* (the same in every thread) */
  uint32_t b, key;
  const ing_rx *r = wns_block(t, g, &b, &key);
  const wn_q q = wns_query(r, &c);
  const rn_walk k = rn_walk_want(r, &q, b);
  (void)rn_bits_wg(r, &k, G, tags, nsym, lo, nullptr, ps, pm);
  if (keys) wns_put_keys(keys, lo, hi, key, threadIdx.x, 256u);
}

__global__ __launch_bounds__(256) void nrq_ings_held_syms_fill_kernel(const ings_tab *__restrict__ t, uint32_t G, const uint32_t *__restrict__ off,
                                                                      uint32_t *__restrict__ tags, uint8_t *__restrict__ nsym,
                                                                      uint32_t *__restrict__ keys) {
  __shared__ uint32_t ps[256], pm[256];
  const uint32_t g = blockIdx.x, lo = off[g], hi = off[g + 1u];
  if (lo == hi) return;
  uint32_t b, key;
  const ing_rx *r = wns_block(t, g, &b, &key);
  const rn_walk k = rn_walk_held(r, b);
  const uint32_t at = rn_bits_wg(r, &k, G, tags, nsym, lo, nullptr, ps, pm);
  (void)rn_rows_wg(r, b, G, tags, nsym, at, ps, pm);
  if (keys) wns_put_keys(keys, lo, hi, key, threadIdx.x, 256u);
}

/* a listing in packets of all members with keys, shaped like rxset_list: the symbol total zeroed, `count(cnt, nsym_total)`, ONE
 * scan, ONE download (the nb + 1 offsets when the per-block counts are asked for, and the two totals) and wait, then `fill(off)` */
template <class Count, class Fill>
static int rxset_list_syms(nrq_rxset *set, const char *who, const char *what, uint32_t *d_tags, uint32_t cap, uint32_t *h_cnt, uint32_t *h_npkt,
                           uint32_t *h_nsym, Count count, Fill fill) {
  nrq_ctx *ctx = set->ctx;
  const uint32_t nb = set->nblk;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  uint32_t *off = (uint32_t *)set->lists;
  HIPCHK(ctx, hipMemsetAsync(off + nb + 1u, 0, 4u, ctx->stream));
  count(off, off + nb + 1u);
  hipLaunchKernelGGL(nrq_ings_lists_scan_kernel, dim3(1), dim3(256), 0, ctx->stream, nb + 1u, off);
  HIPCHK(ctx, hipGetLastError());
  std::vector<uint32_t> h(h_cnt ? (size_t)nb + 2u : 2u, 0); /* (the last two words: packets, symbols) */
  HIPCHK(ctx, hipMemcpyAsync(h.data(), h_cnt ? off : off + nb, h.size() * 4u, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  *h_npkt = h[h.size() - 2u];
  if (h_nsym) *h_nsym = h.back();
  if (h_cnt)
    for (uint32_t g = 0; g < nb; g++) h_cnt[g] = h[g + 1u] - h[g];
  if (!d_tags) return 0;
  if (cap < *h_npkt) return fail(ctx, -1, "%s: %u packets are %s, d_tags and d_nsym have room for %u", who, *h_npkt, what, cap);
  if (*h_npkt == 0) return 0;
  fill((const uint32_t *)off);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

extern "C" {

int nrq_rxset_want_syms(nrq_rxset *set, uint32_t flags, uint32_t extra, uint32_t esi_from, uint32_t G, uint32_t *d_keys, uint32_t *d_tags,
                        uint8_t *d_nsym, uint32_t cap, uint32_t *h_cnt, uint32_t *h_npkt, uint32_t *h_nsym) {
  if (!set) return -1;
  nrq_ctx *ctx = set->ctx;
  const char *who = "nrq_rxset_want_syms";
  const int rc = rn_check(ctx, who, G, d_tags, d_nsym, h_npkt, h_nsym);
  if (rc) return rc;
  switch (wn_check(flags, extra, esi_from)) {
    case 1: return fail(ctx, -1, "%s: unknown flags 0x%x", who, flags);
    case 2: return fail(ctx, -1, "%s: NRQ_WANT_SOURCE takes neither extra nor esi_from (%u, %u)", who, extra, esi_from);
    case 3: return fail(ctx, -1, "%s: extra %u is above 2^24", who, extra);
    default: break;
  }
  if (d_keys && !d_tags) return fail(ctx, -1, "%s: d_keys without d_tags", who);
  const uint32_t nb = set->nblk;
  if (nb == 0) return 0;
  const ings_tab *t = (const ings_tab *)set->tab;
  const wns_call c{flags, extra, esi_from};
  hipStream_t st = ctx->stream;
  return rxset_list_syms(
      set, who, "wanted", d_tags, cap, h_cnt, h_npkt, h_nsym,
      [&](uint32_t *cnt, uint32_t *tot) { hipLaunchKernelGGL(nrq_ings_want_syms_count_kernel, dim3(nb), dim3(256), 0, st, t, c, G, cnt, tot); },
      [&](const uint32_t *off) {
        hipLaunchKernelGGL(nrq_ings_want_syms_fill_kernel, dim3(nb), dim3(256), 0, st, t, c, G, off, d_tags, d_nsym, d_keys);
      });
}

int nrq_rxset_held_syms(nrq_rxset *set, uint32_t G, uint32_t *d_keys, uint32_t *d_tags, uint8_t *d_nsym, uint32_t cap, uint32_t *h_cnt,
                        uint32_t *h_npkt, uint32_t *h_nsym) {
  if (!set) return -1;
  nrq_ctx *ctx = set->ctx;
  const char *who = "nrq_rxset_held_syms";
  const int rc = rn_check(ctx, who, G, d_tags, d_nsym, h_npkt, h_nsym);
  if (rc) return rc;
  if (d_keys && !d_tags) return fail(ctx, -1, "%s: d_keys without d_tags", who);
  const uint32_t nb = set->nblk;
  if (nb == 0) return 0;
  const ings_tab *t = (const ings_tab *)set->tab;
  hipStream_t st = ctx->stream;
  return rxset_list_syms(
      set, who, "held", d_tags, cap, h_cnt, h_npkt, h_nsym,
      [&](uint32_t *cnt, uint32_t *tot) { hipLaunchKernelGGL(nrq_ings_held_syms_count_kernel, dim3(nb), dim3(256), 0, st, t, G, cnt, tot); },
      [&](const uint32_t *off) { hipLaunchKernelGGL(nrq_ings_held_syms_fill_kernel, dim3(nb), dim3(256), 0, st, t, G, off, d_tags, d_nsym, d_keys); });
}

} /* extern "C" */

/* ================================================ sender sets (nrq_txset_*, emit_set_body.h) ==== */
/* The tag-list emit over a segment table in device memory: one chain of kernels writes the packets of all members into one
 * buffer.  Three bucketing passes make the block-major work order over the set's global blocks -- the histogram pass also finds
 * each packet's segment (a linear search over the compact arrays staged in LDS; every lane reads the same entry) and leaves it
 * in c.seg[] for the passes behind it -- then nrq_emit_set_kernel writes the packets.  Kernels of their own: every nrq_emit_kernel
 * and nrq_emit_held_kernel instantiation is compiled from the code it always was.  The payload walk (tx_payload, under
 * txs_payload's key word) and the held repair row lookup (tx_held_row) are those kernels' bodies. */
enum : int { TXS_V16_KEY = 4 }; /* beside TX_V16 .. TX_BYTE: 16-byte loads and stores under the 8-byte header (key, FEC Payload ID) */
static_assert(TXS_V16_KEY == 4, "sys_emit_path (syms_set_body.h) names this path by its number");

__global__ __launch_bounds__(256) void nrq_txs_hist_kernel(const txs_tab *__restrict__ t, txs_call c, uint32_t *__restrict__ cnt) {
  __shared__ uint32_t skey[TXS_MAX_SEGS], ssbn0[TXS_MAX_SEGS], scnt[TXS_MAX_SEGS], sblk0[TXS_MAX_SEGS];
  __shared__ uint32_t h[TXS_MAX_BLOCKS + 1u];
  const uint32_t nseg = min(t->nseg, TXS_MAX_SEGS), nb = min(t->nblk, TXS_MAX_BLOCKS), i = threadIdx.x;
  if (i < nseg) { skey[i] = t->key[i]; ssbn0[i] = t->sbn0[i]; scnt[i] = t->cnt[i]; sblk0[i] = t->blk0[i]; }
  for (uint32_t g = i; g <= nb; g += 256u) h[g] = 0;
  __syncthreads();
  const uint32_t k0 = blockIdx.x * TX_BIN_TILE, k1 = min(c.n, k0 + TX_BIN_TILE);
  for (uint32_t k = k0 + i; k < k1; k += 256u) {
    const uint32_t tag = c.tags[k], sg = txs_find(skey, ssbn0, scnt, nseg, txs_key_of(&c, k), tag >> 24);
    c.seg[k] = sg;
    atomicAdd(&h[txs_bin(ssbn0, sblk0, nb, sg, tag)], 1u);
  }
  __syncthreads();
  for (uint32_t g = i; g <= nb; g += 256u)
    if (h[g]) atomicAdd(&cnt[g], h[g]);
}

/* each tile reserves its packets' places in every bucket (one atomic per bucket and tile), then writes order[] */
__global__ __launch_bounds__(256) void nrq_txs_place_kernel(const txs_tab *__restrict__ t, txs_call c, uint32_t *__restrict__ cursor) {
  __shared__ uint32_t ssbn0[TXS_MAX_SEGS], sblk0[TXS_MAX_SEGS];
  __shared__ uint32_t h[TXS_MAX_BLOCKS + 1u], base[TXS_MAX_BLOCKS + 1u];
  constexpr uint32_t PER = TX_BIN_TILE / 256u;
  const uint32_t nseg = min(t->nseg, TXS_MAX_SEGS), nb = min(t->nblk, TXS_MAX_BLOCKS), i = threadIdx.x;
  if (i < nseg) { ssbn0[i] = t->sbn0[i]; sblk0[i] = t->blk0[i]; }
  for (uint32_t g = i; g <= nb; g += 256u) h[g] = 0;
  __syncthreads();
  const uint32_t k0 = blockIdx.x * TX_BIN_TILE;
  uint32_t bin[PER], rank[PER];
#pragma unroll
  for (uint32_t r = 0; r < PER; r++) {
    const uint32_t k = k0 + r * 256u + i;
    bin[r] = TX_NONE;
    if (k < c.n) {
      const uint32_t sg = c.seg[k];
      bin[r] = sg < nseg ? txs_bin(ssbn0, sblk0, nb, sg, c.tags[k]) : nb;
    }
    rank[r] = bin[r] != TX_NONE ? atomicAdd(&h[bin[r]], 1u) : 0u;
  }
  __syncthreads();
  for (uint32_t g = i; g <= nb; g += 256u) base[g] = h[g] ? atomicAdd(&cursor[g], h[g]) : 0u;
  __syncthreads();
#pragma unroll
  for (uint32_t r = 0; r < PER; r++)
    if (bin[r] != TX_NONE) c.order[base[bin[r]] + rank[r]] = k0 + r * 256u + i;
}

/* the packet of (key, tag) at P in the call's header form (hdr = 0 / 4 / 8): tx_payload under the key word, or the 16-byte form
 * of the 8-byte header; `rows` as in tx_payload (one symbol, or a run of them: the payloads of a run are contiguous, so the carry
 * crosses a symbol boundary as it crosses any chunk boundary) */
template <int MODE, class ROWS>
__device__ __forceinline__ void txs_payload(const uint8_t *__restrict__ base, uint32_t T, const ROWS rows, uint32_t key, uint32_t tag,
                                            uint8_t *__restrict__ P, uint32_t hdr, uint32_t lane) {
  if constexpr (MODE == TXS_V16_KEY) {
    /* packet chunk j (bytes 16j .. 16j+15) = payload dwords 4j-2 .. 4j+1: the previous lane's .z .w (the key word and the header
     * for j = 0, the wave's last lane of the previous round for its first lane), then this chunk's .x .y; the last .z .w go to +len */
    const uint32_t len = rows.len(T), nch = len >> 4;
    uint32_t cz = txs_key_word(key), cw = tx_header_word(tag);
    for (uint32_t j0 = 0; j0 < nch; j0 += 64u) {
      const uint32_t j = j0 + lane;
      const bool act = j < nch;
      tx_u128 v{0u, 0u, 0u, 0u};
      if (act) v = rows.template word<tx_u128>(base, T, (uint64_t)j * 16u);
      uint32_t pz = __shfl_up(v.z, 1u), pw = __shfl_up(v.w, 1u);
      if (lane == 0) { pz = cz; pw = cw; }
      if (act) *reinterpret_cast<tx_u128 *>(P + (uint64_t)j * 16u) = tx_u128{pz, pw, v.x, v.y};
      if (j == nch - 1u) *reinterpret_cast<uint2 *>(P + len) = make_uint2(v.z, v.w);
      cz = __shfl(v.z, 63);
      cw = __shfl(v.w, 63);
    }
  } else if constexpr (MODE == TX_DWORD) {
    if (hdr == 8u) {
      if (lane == 0) *reinterpret_cast<uint32_t *>(P) = txs_key_word(key);
      P += 4;
    }
    tx_payload<TX_DWORD>(base, T, rows, tag, P, hdr ? 1u : 0u, lane);
  } else if constexpr (MODE == TX_BYTE) {
    if (hdr == 8u) {
      if (lane < 4u) P[lane] = (uint8_t)(txs_key_word(key) >> (8u * lane));
      P += 4;
    }
    tx_payload<TX_BYTE>(base, T, rows, tag, P, hdr ? 1u : 0u, lane);
  } else {
    tx_payload<MODE>(base, T, rows, tag, P, hdr ? 1u : 0u, lane); /* (TX_V16: hdr = 0; TX_V16_SHIFT: hdr = 4) */
  }
}

/* The wave shape of nrq_emit_kernel over the table: one wave per TX_WAVE_PKTS work items in block-major order.  Each lane admits
 * one item and builds its column list into LDS from its segment's parameters, read from the table (lanes of one block read the
 * same entry); then the wave writes the items' packets one after the other, the segment index made wave-uniform so that its
 * fields come through the uniform table pointer.  HELD: a packet of a block that is not ready is still written when the segment's
 * reception holds its symbol, the repair row found as in nrq_emit_held_kernel (tx_held_row). */
template <int MODE, bool HELD>
__global__ __launch_bounds__(256) void nrq_emit_set_kernel(const txs_tab *__restrict__ t, txs_ready rdy, txs_call c) {
  __shared__ uint32_t s_cols[TX_WAVES][TX_WAVE_PKTS][TX_COLS];
  __shared__ uint32_t s_n[TX_WAVES][TX_WAVE_PKTS], s_tag[TX_WAVES][TX_WAVE_PKTS], s_k[TX_WAVES][TX_WAVE_PKTS];
  __shared__ uint32_t s_seg[TX_WAVES][TX_WAVE_PKTS], s_key[TX_WAVES][TX_WAVE_PKTS];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint64_t w0 = ((uint64_t)blockIdx.x * TX_WAVES + wv) * TX_WAVE_PKTS;
  if (w0 + lane < c.n) {
    const uint32_t k = c.order[w0 + lane];
    uint32_t n = 0, kind = TX_READY, tag = 0, sg = TXS_NONE, key = 0;
    if (k < c.n) { /* (always: the work order is a permutation) */
      tag = c.tags[k];
      key = txs_key_of(&c, k);
      sg = c.seg[k];
      int32_t code = TX_FOREIGN;
      if (sg < TXS_MAX_SEGS) {
        const txs_seg *S = &t->seg[sg];
        if (txs_admit(S, &rdy, HELD, tag, &code, &kind)) {
          if (kind == TX_HELD_REP) { s_cols[wv][lane][0] = 0u; n = 1u; } /* (row 0 from the base of the row found below) */
          else n = tx_rows(&S->b, tag, s_cols[wv][lane]);
        }
      }
      if (c.results && kind != TX_HELD_REP) c.results[k] = code; /* (a held repair packet's: once its row is found) */
    }
    s_n[wv][lane] = n | (kind << 8);
    s_tag[wv][lane] = tag;
    s_k[wv][lane] = k;
    s_seg[wv][lane] = sg;
    s_key[wv][lane] = key;
  }
  __syncthreads();
  const uint32_t cnt = w0 >= c.n ? 0u : (uint32_t)min((uint64_t)TX_WAVE_PKTS, c.n - w0);
  const uint32_t T = c.T;
  for (uint32_t i = 0; i < cnt; i++) { /* (wave-uniform) */
    const uint32_t nk = __builtin_amdgcn_readfirstlane(s_n[wv][i]), n = nk & 0xFFu;
    if (!n) continue; /* no member, or a symbol of a block that is not ready which is not held */
    const uint32_t tag = __builtin_amdgcn_readfirstlane(s_tag[wv][i]);
    const uint32_t k = __builtin_amdgcn_readfirstlane(s_k[wv][i]);
    const uint32_t key = __builtin_amdgcn_readfirstlane(s_key[wv][i]);
    const txs_seg *S = &t->seg[__builtin_amdgcn_readfirstlane(s_seg[wv][i])];
    const uint8_t *base;
    if (HELD && (nk >> 8) == TX_HELD_REP) {
      const tx_held_seg *hs = &S->h;
      const uint32_t b = (tag >> 24) - S->b.sbn0;
      const uint32_t q = tx_held_row(hs, b, tag & 0xFFFFFFu, lane);
      if (c.results && lane == 0) c.results[k] = q == TX_NONE ? TX_NOT_READY : 0;
      if (q == TX_NONE) continue; /* (the books say otherwise: a marked repair ESI has its row) */
      base = tx_held_rep_base(hs, b) + (uint64_t)q * T;
    } else {
      base = tx_base(&S->b, tag);
    }
    txs_payload<MODE>(base, T, tx_one{s_cols[wv][i], n}, key, tag, c.pkts + (uint64_t)k * c.pkt_stride, c.hdr, lane);
  }
}

struct txset_member {
  uint32_t key;
  tx_sender *tx;
  bool obj; /* an object: it owns its key */
};
struct txset_seg { /* one row of the device table, as the host remembers it */
  tx_sender *tx;
  uint32_t g;      /* segment of tx->s */
};

struct nrq_txset {
  nrq_ctx *ctx;
  uint32_t T;
  std::vector<txset_member> mem; /* sorted by (key, first SBN) */
  std::vector<txset_seg> segs;   /* sorted by (key, sbn0): the order of the device table */
  uint32_t nblk;                 /* blocks over all members */
  void *tab;                     /* struct txs_tab in device memory */
  DevScratch scratch;            /* per-call arrays: bucket counts, the packets' segments, the work order */
};

static uint32_t txset_key_of(const nrq_txset *set, const tx_sender *tx) {
  for (const txset_member &m : set->mem)
    if (m.tx == tx) return m.key;
  return 0;
}

/* the table rows of `mem` (sorted), in table order */
static std::vector<txset_seg> txset_rows(const std::vector<txset_member> &mem) {
  std::vector<txset_seg> rows;
  for (const txset_member &m : mem) {
    std::vector<txset_seg> own;
    for (uint32_t g = 0; g < m.tx->s.nseg; g++) own.push_back(txset_seg{m.tx, g});
    std::sort(own.begin(), own.end(), [](const txset_seg &a, const txset_seg &b) { return a.tx->s.seg[a.g].sbn0 < b.tx->s.seg[b.g].sbn0; });
    rows.insert(rows.end(), own.begin(), own.end());
  }
  return rows;
}

/* the segment table of `rows` into device memory.  Waits for the stream first: an emit enqueued before still reads the old
 * table. */
static int txset_upload(nrq_txset *set, const std::vector<txset_member> &mem, const std::vector<txset_seg> &rows) {
  nrq_ctx *ctx = set->ctx;
  std::vector<txs_tab> hv(1);
  txs_tab &h = hv[0];
  memset(&h, 0, sizeof(h));
  h.nseg = (uint32_t)rows.size();
  for (uint32_t i = 0; i < h.nseg; i++) {
    const tx_sender *tx = rows[i].tx;
    const uint32_t g = rows[i].g;
    txs_seg &S = h.seg[i];
    S.b = tx->s.seg[g];
    if (tx->relay && !tx->detached && tx->from[g]) S.h = tx_held_table(tx).seg[g];
    for (const txset_member &m : mem)
      if (m.tx == tx) S.key = m.key;
    S.blk0 = h.nblk;
    h.key[i] = S.key; h.sbn0[i] = S.b.sbn0; h.cnt[i] = S.b.nblk; h.blk0[i] = S.blk0;
    h.nblk += S.b.nblk;
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  HIPCHK(ctx, hipMemcpy(set->tab, &h, sizeof(h), hipMemcpyHostToDevice));
  return 0;
}

/* take `mem` as the set's members (sorted here); on failure the set keeps the ones it had */
static int txset_commit(nrq_txset *set, std::vector<txset_member> &mem) {
  std::sort(mem.begin(), mem.end(), [](const txset_member &a, const txset_member &b) {
    return a.key != b.key ? a.key < b.key : a.tx->s.sbn0 < b.tx->s.sbn0;
  });
  std::vector<txset_seg> rows = txset_rows(mem);
  const int rc = txset_upload(set, mem, rows);
  if (rc) return rc;
  for (const txset_member &m : set->mem) m.tx->set = nullptr;
  set->mem.swap(mem);
  set->segs.swap(rows);
  set->nblk = 0;
  for (const txset_member &m : set->mem) { m.tx->set = set; set->nblk += m.tx->s.Z; }
  return 0;
}

/* a transmission goes away (nrq_tx_destroy / nrq_otx_destroy): it leaves its set first */
static void txset_drop(tx_sender *tx) {
  nrq_txset *set = tx->set;
  std::vector<txset_member> mem;
  for (const txset_member &m : set->mem)
    if (m.tx != tx) mem.push_back(m);
  if (txset_commit(set, mem) != 0) { /* (the table could not be written: an empty host list keeps every later emit off the stale one) */
    for (const txset_member &m : set->mem) m.tx->set = nullptr;
    set->mem.clear();
    set->segs.clear();
    set->nblk = 0;
  }
}

static int txset_attach(nrq_txset *set, const char *who, uint32_t key, tx_sender *tx, bool obj) {
  nrq_ctx *ctx = set->ctx;
  const tx_src &s = tx->s;
  if (tx->ctx != ctx) return fail(ctx, -1, "%s: the transmission belongs to another context", who);
  if (s.seg[0].T != set->T) return fail(ctx, -1, "%s: the transmission's T %u is not the set's %u", who, s.seg[0].T, set->T);
  if (tx->set) return fail(ctx, -1, "%s: the transmission is in a set already", who);
  for (const txset_member &m : set->mem) {
    if (m.key != key) continue;
    if (obj || m.obj) return fail(ctx, -1, "%s: key %u has members already, and an object owns its key", who, key);
    const tx_src &o = m.tx->s;
    if (s.sbn0 < o.sbn0 + o.Z && o.sbn0 < s.sbn0 + s.Z)
      return fail(ctx, -1, "%s: SBNs %u..%u under key %u overlap a member's %u..%u", who, s.sbn0, s.sbn0 + s.Z - 1u, key, o.sbn0,
                  o.sbn0 + o.Z - 1u);
  }
  if (set->segs.size() + s.nseg > NRQ_TXSET_MAX_SEGS) return fail(ctx, -1, "%s: a set holds at most %u table segments", who, NRQ_TXSET_MAX_SEGS);
  if (set->nblk + s.Z > NRQ_TXSET_MAX_BLOCKS) return fail(ctx, -1, "%s: a set holds at most %u blocks", who, NRQ_TXSET_MAX_BLOCKS);
  std::vector<txset_member> mem = set->mem;
  mem.push_back(txset_member{key, tx, obj});
  return txset_commit(set, mem);
}

/* What every emit of the set does first once its own arguments are checked -- the list route (txset_call_of) and the range route
 * (txset_range): the members' state, the set's scratch grown to `need` bytes, the ready bits of the global blocks, the payload path
 * (*mode: TX_V16 .. TX_BYTE or TXS_V16_KEY).  Nothing is enqueued here. */
static int txset_prepare(nrq_txset *set, const char *who, size_t need, void *d_pkts, size_t pkt_stride, uint32_t hdr, bool held, txs_ready *rdyp,
                         int *mode) {
  nrq_ctx *ctx = set->ctx;
  for (const txset_member &m : set->mem) {
    if (m.tx->detached) return fail(ctx, -1, "%s: the reception of the relay under key %u was destroyed", who, m.key);
    if (!m.tx->encoded) return fail(ctx, -1, "%s: the member under key %u is not encoded (%s)", who, m.key, m.tx->unencoded);
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const int rc = set->scratch.ensure(ctx, need);
  if (rc) return rc;
  /* the ready bits of the global blocks as the members have them NOW, by value into this call's kernel arguments: a relay's mask
   * changes in decodes, encodes and resets without any call on the set, and an emit still queued keeps the bits it was given */
  txs_ready rdy{};
  uintptr_t al = reinterpret_cast<uintptr_t>(d_pkts) | pkt_stride | set->T;
  uint32_t g0 = 0;
  for (const txset_seg &r : set->segs) {
    const tx_sender *tx = r.tx;
    const tx_blk &t = tx->s.seg[r.g];
    for (uint32_t b = 0; b < t.nblk; b++)
      if (!tx->relay || tx_is_ready(tx, t.sbn0 + b - tx->s.sbn0)) rdy.w[(g0 + b) >> 5] |= 1u << ((g0 + b) & 31u);
    g0 += t.nblk;
    al |= reinterpret_cast<uintptr_t>(t.src) | t.src_stride | reinterpret_cast<uintptr_t>(t.inter) | t.inter_stride;
    if (held && tx->relay) { /* (held repair rows are copied too) */
      const ing_rx &rr = tx->from[r.g]->r;
      al |= reinterpret_cast<uintptr_t>(rr.rep) | rr.rep_stride;
    }
  }
  *mode = sys_emit_path(al, hdr, ctx->tune.tx_dword ? 1u : 0u);
  *rdyp = rdy;
  return 0;
}

/* The list route once its arguments are checked: txset_prepare, the call over n packets with its arrays carved out of the set's
 * scratch, and the three bucketing passes over the tags, enqueued.  The emit kernel is the caller's. */
static int txset_call_of(nrq_txset *set, const char *who, const uint32_t *d_keys, const uint32_t *d_tags, uint32_t n, void *d_pkts,
                         size_t pkt_stride, uint32_t hdr, bool held, int32_t *d_results, txs_ready *rdyp, txs_call *cp, int *mode) {
  nrq_ctx *ctx = set->ctx;
  const uint32_t nb = set->nblk, nbins = nb + 1u;
  const size_t o_seg = rx_al((size_t)nbins * 4u), o_order = o_seg + rx_al((size_t)n * 4u), need = o_order + rx_al((size_t)n * 4u);
  const int rc = txset_prepare(set, who, need, d_pkts, pkt_stride, hdr, held, rdyp, mode);
  if (rc) return rc;
  uint8_t *p = (uint8_t *)set->scratch.p;
  uint32_t *cnt = (uint32_t *)p;
  txs_call c{};
  c.pkts = (uint8_t *)d_pkts;
  c.pkt_stride = pkt_stride;
  c.n = n;
  c.hdr = hdr;
  c.T = set->T;
  c.keys = d_keys;
  c.tags = d_tags;
  c.seg = (uint32_t *)(p + o_seg);
  c.order = (uint32_t *)(p + o_order);
  c.results = d_results;
  *cp = c;
  const txs_tab *t = (const txs_tab *)set->tab;
  hipStream_t st = ctx->stream;
  const uint32_t tiles = (n + TX_BIN_TILE - 1u) / TX_BIN_TILE;
  HIPCHK(ctx, hipMemsetAsync(cnt, 0, (size_t)nbins * 4u, st));
  hipLaunchKernelGGL(nrq_txs_hist_kernel, dim3(tiles), dim3(256), 0, st, t, c, cnt);
  hipLaunchKernelGGL(nrq_ings_lists_scan_kernel, dim3(1), dim3(256), 0, st, nbins, cnt);
  hipLaunchKernelGGL(nrq_txs_place_kernel, dim3(tiles), dim3(256), 0, st, t, c, cnt);
  return 0;
}

static_assert(NRQ_TXSET_MAX_SEGS == TXS_MAX_SEGS && NRQ_TXSET_MAX_BLOCKS == TXS_MAX_BLOCKS, "the header's caps are the table's");

extern "C" {

int nrq_txset_create(nrq_ctx *ctx, uint32_t T, nrq_txset **out) {
  if (!ctx) return -1;
  if (!out) return fail(ctx, -1, "nrq_txset_create: out is NULL");
  *out = nullptr;
  if (T == 0) return fail(ctx, -1, "nrq_txset_create: T is 0");
  nrq_txset *set = new (std::nothrow) nrq_txset();
  if (!set) return fail(ctx, -1, "nrq_txset_create: out of host memory");
  set->ctx = ctx;
  set->T = T;
  const int rc = nrq_dev_alloc(ctx, sizeof(txs_tab), &set->tab);
  if (rc) {
    delete set;
    return rc;
  }
  *out = set;
  return 0;
}

void nrq_txset_destroy(nrq_txset *set) {
  if (!set) return;
  nrq_ctx *ctx = set->ctx;
  for (const txset_member &m : set->mem) m.tx->set = nullptr;
  (void)hipStreamSynchronize(ctx->stream); /* (the pool hands freed blocks out again at once) */
  if (set->tab) nrq_dev_free(ctx, set->tab);
  set->scratch.release(ctx);
  delete set;
}

int nrq_txset_attach(nrq_txset *set, uint32_t key, nrq_tx *tx) {
  if (!set) return -1;
  if (!tx) return fail(set->ctx, -1, "nrq_txset_attach: the transmission is NULL");
  return txset_attach(set, "nrq_txset_attach", key, tx, false);
}

int nrq_txset_attach_obj(nrq_txset *set, uint32_t key, nrq_otx *tx) {
  if (!set) return -1;
  if (!tx) return fail(set->ctx, -1, "nrq_txset_attach_obj: the object sender is NULL");
  return txset_attach(set, "nrq_txset_attach_obj", key, tx, true);
}

int nrq_txset_detach(nrq_txset *set, uint32_t key) {
  if (!set) return -1;
  std::vector<txset_member> mem;
  for (const txset_member &m : set->mem)
    if (m.key != key) mem.push_back(m);
  if (mem.size() == set->mem.size()) return fail(set->ctx, -1, "nrq_txset_detach: no member under key %u", key);
  return txset_commit(set, mem);
}

int nrq_txset_blocks(nrq_txset *set, uint32_t *h_keys, uint32_t *h_sbn, uint32_t cap, uint32_t *h_n) {
  if (!set) return -1;
  if (!h_n) return fail(set->ctx, -1, "nrq_txset_blocks: h_n is NULL");
  *h_n = set->nblk;
  if (!h_keys && !h_sbn) return 0;
  if (cap < set->nblk) return fail(set->ctx, -1, "nrq_txset_blocks: the set has %u blocks, the arrays have room for %u", set->nblk, cap);
  uint32_t j = 0;
  for (const txset_seg &r : set->segs) {
    const tx_blk &t = r.tx->s.seg[r.g];
    const uint32_t key = txset_key_of(set, r.tx);
    for (uint32_t b = 0; b < t.nblk; b++, j++) {
      if (h_keys) h_keys[j] = key;
      if (h_sbn) h_sbn[j] = t.sbn0 + b;
    }
  }
  return 0;
}

int nrq_txset_emit(nrq_txset *set, const uint32_t *d_keys, const uint32_t *d_tags, uint32_t n, void *d_pkts, size_t pkt_stride, uint32_t flags,
                   int32_t *d_results) {
  using set_fn = void (*)(const txs_tab *, txs_ready, txs_call);
  static const set_fn kern[2][5] = { /* [held][mode] */
      {nrq_emit_set_kernel<TX_V16, false>, nrq_emit_set_kernel<TX_V16_SHIFT, false>, nrq_emit_set_kernel<TX_DWORD, false>,
       nrq_emit_set_kernel<TX_BYTE, false>, nrq_emit_set_kernel<TXS_V16_KEY, false>},
      {nrq_emit_set_kernel<TX_V16, true>, nrq_emit_set_kernel<TX_V16_SHIFT, true>, nrq_emit_set_kernel<TX_DWORD, true>,
       nrq_emit_set_kernel<TX_BYTE, true>, nrq_emit_set_kernel<TXS_V16_KEY, true>}};
  if (!set) return -1;
  nrq_ctx *ctx = set->ctx;
  const bool inl = (flags & NRQ_TX_TAG_INLINE) != 0, kinl = (flags & NRQ_TX_KEY_INLINE) != 0, held = (flags & NRQ_TX_HELD) != 0;
  if (flags & ~(uint32_t)(NRQ_TX_TAG_INLINE | NRQ_TX_HELD | NRQ_TX_KEY_INLINE)) return fail(ctx, -1, "nrq_txset_emit: unknown flags 0x%x", flags);
  if (kinl && !inl) return fail(ctx, -1, "nrq_txset_emit: NRQ_TX_KEY_INLINE needs NRQ_TX_TAG_INLINE");
  if (n == 0 || set->mem.empty()) return 0;
  if (!d_pkts) return fail(ctx, -1, "nrq_txset_emit: d_pkts is NULL");
  if (!d_tags || n > 0x7FFFFFFFu) return fail(ctx, -1, "nrq_txset_emit: bad tags (n=%u)", n);
  const uint32_t hdr = kinl ? 8u : inl ? 4u : 0u;
  if (pkt_stride < (size_t)set->T + hdr) return fail(ctx, -1, "nrq_txset_emit: pkt_stride %zu shorter than a packet", pkt_stride);
  txs_ready rdy;
  txs_call c;
  int mode;
  const int rc = txset_call_of(set, "nrq_txset_emit", d_keys, d_tags, n, d_pkts, pkt_stride, hdr, held, d_results, &rdy, &c, &mode);
  if (rc) return rc;
  const dim3 grid((n + TX_WAVES * TX_WAVE_PKTS - 1u) / (TX_WAVES * TX_WAVE_PKTS)), wg(64u * TX_WAVES);
  hipLaunchKernelGGL(kern[held][mode], grid, wg, 0, ctx->stream, (const txs_tab *)set->tab, rdy, c);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

} /* extern "C" */

/* ================================================ sets: packets of several symbols (nrq_*set_*_syms, syms_set_body.h) ==== */
/* The two layers above put together, in kernels of their own: every kernel of the sets and of the single several-symbol forms is
 * compiled from the code it always was.
 *
 * Ingest: the chain of nrq_rxset_add over n * G slots.  Passes 2 and 4 are per global block and are nrq_rxset_add's kernels, the
 * copy is nrq_rx_add_syms'; passes 1, 3, 5, 7 are these, with the geometry of the nrq_ings_* kernels, and ask syms_set_body.h what
 * a slot is.  Pass 1 decodes and searches once per SLOT: the slots of a packet may lie in two waves, and the search reads LDS. */
__global__ __launch_bounds__(256) void nrq_ings_first_syms_kernel(const ings_tab *__restrict__ t, ings_call s, sy_rx y) {
  __shared__ uint32_t skey[INGS_MAX_MEMBERS], ssbn0[INGS_MAX_MEMBERS], scnt[INGS_MAX_MEMBERS], sobjZ[INGS_MAX_MEMBERS];
  const uint32_t nmem = min(t->nmem, INGS_MAX_MEMBERS), i = threadIdx.x;
  if (i < nmem) { skey[i] = t->key[i]; ssbn0[i] = t->sbn0[i]; scnt[i] = t->cnt[i]; sobjZ[i] = t->objZ[i]; }
  __syncthreads();
  const uint32_t sl = blockIdx.x * 256u + threadIdx.x;
  if (sl >= s.c.n) return;
  uint32_t key, tag;
  ings_decode(&s, sl / y.G, &key, &tag);
  sys_first(t, &s, &y, sl, tag, ings_find(skey, ssbn0, scnt, sobjZ, nmem, key, tag >> 24));
}

/* dynamic LDS: t->nblk counters */
__global__ __launch_bounds__(256) void nrq_ings_hist_syms_kernel(const ings_tab *__restrict__ t, ings_call s, sy_rx y) {
  extern __shared__ uint32_t ings_h[];
  const uint32_t i = threadIdx.x, sl = blockIdx.x * ING_TILE + i, nb = t->nblk;
  for (uint32_t g = i; g < nb; g += 256u) ings_h[g] = 0;
  __syncthreads();
  if (sl < s.c.n) {
    const uint32_t g = sys_cand(t, &s, &y, sl);
    if (g != ING_NONE) atomicAdd(&ings_h[g], 1u);
  }
  __syncthreads();
  for (uint32_t g = i; g < nb; g += 256u) s.c.base[(size_t)g * s.c.ntiles + blockIdx.x] = ings_h[g];
}

/* dynamic LDS: 4 * t->nblk counters (nrq_ings_classify_kernel over slots: the same ranking, in slot order) */
__global__ __launch_bounds__(256) void nrq_ings_classify_syms_kernel(const ings_tab *__restrict__ t, ings_call s, sy_rx y) {
  extern __shared__ uint32_t ings_wc[];
  const uint32_t i = threadIdx.x, sl = blockIdx.x * ING_TILE + i, nb = t->nblk;
  for (uint32_t j = i; j < 4u * nb; j += 256u) ings_wc[j] = 0;
  __syncthreads();
  const uint32_t g = sl < s.c.n ? sys_cand(t, &s, &y, sl) : ING_NONE;
  const uint32_t row = ing_rank_wg(ings_wc, nb, g, s.c.base, s.c.ntiles);
  if (sl < s.c.n) sys_classify(t, &s, &y, sl, row);
}

__global__ __launch_bounds__(256) void nrq_ings_fold_syms_kernel(const ings_tab *__restrict__ t, ings_call s, sy_rx y) {
  const uint32_t sl = blockIdx.x * 256u + threadIdx.x;
  if (sl < s.c.n) sys_fold(t, &s, &y, sl);
}

/* Emit.  The wave shape of nrq_emit_syms_kernel over the segment table of nrq_emit_set_kernel: a wave takes 64 / G packets of the
 * work order (block-major over the set's global blocks: nrq_txs_hist_kernel, the scan and nrq_txs_place_kernel over the first
 * tags), lane l the slot (l / G, l % G).  Each lane admits its packet (sys_tx_admit: per packet, so every lane of a packet decides
 * alike) and builds its slot's column list into LDS from its segment's parameters, read through the table pointer; then the wave
 * writes the admitted packets one after the other, each as ONE run of c_k * T bytes (txs_payload over a tx_run; a packet of one
 * symbol takes the one-symbol walk), the segment index made wave-uniform as in nrq_emit_set_kernel. */
template <int MODE>
__global__ __launch_bounds__(256) void nrq_emit_set_syms_kernel(const txs_tab *__restrict__ t, txs_ready rdy, txs_call c, sy_tx y) {
  __shared__ uint32_t s_cols[TX_WAVES][TX_WAVE_PKTS][TX_COLS];
  __shared__ uint32_t s_n[TX_WAVES][TX_WAVE_PKTS], s_tag[TX_WAVES][TX_WAVE_PKTS], s_k[TX_WAVES][TX_WAVE_PKTS];
  __shared__ uint32_t s_seg[TX_WAVES][TX_WAVE_PKTS], s_key[TX_WAVES][TX_WAVE_PKTS];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint32_t G = y.G, per = 64u / G, p = lane / G, i = lane - p * G;
  const uint64_t w0 = ((uint64_t)blockIdx.x * TX_WAVES + wv) * per; /* the wave's first packet in the work order */
  {
    uint32_t n = 0, cnt = 0, tag0 = 0, k = 0, sg = TXS_NONE, key = 0;
    if (p < per && w0 + p < c.n) {
      k = c.order[w0 + p];
      if (k < c.n) { /* (always: the work order is a permutation) */
        tag0 = c.tags[k];
        key = txs_key_of(&c, k);
        sg = c.seg[k];
        int32_t code;
        if (sys_tx_admit(t, &rdy, &y, k, tag0, sg, &code, &cnt) && i < cnt) n = tx_rows(&t->seg[sg].b, tag0 + i, s_cols[wv][lane]);
        if (i == 0u && c.results) c.results[k] = code;
      }
    }
    s_n[wv][lane] = n | (cnt << 8); /* (cnt = 0: the packet stays untouched) */
    s_tag[wv][lane] = tag0;
    s_k[wv][lane] = k;
    s_seg[wv][lane] = sg;
    s_key[wv][lane] = key;
  }
  __syncthreads();
  const uint32_t T = c.T;
  for (uint32_t q = 0; q < per && w0 + q < c.n; q++) { /* (wave-uniform) */
    const uint32_t l0 = q * G;
    const uint32_t nk = __builtin_amdgcn_readfirstlane(s_n[wv][l0]), cnt = nk >> 8;
    if (!cnt) continue; /* no member, a block that is not ready, a refused range */
    const uint32_t tag = __builtin_amdgcn_readfirstlane(s_tag[wv][l0]);
    const uint32_t k = __builtin_amdgcn_readfirstlane(s_k[wv][l0]);
    const uint32_t key = __builtin_amdgcn_readfirstlane(s_key[wv][l0]);
    const txs_seg *S = &t->seg[__builtin_amdgcn_readfirstlane(s_seg[wv][l0])];
    const uint8_t *base = tx_base(&S->b, tag); /* (a sender's packet never runs from source into repair ESIs: sy_tx_count) */
    uint8_t *P = c.pkts + (uint64_t)k * c.pkt_stride;
    if (cnt == 1u) txs_payload<MODE>(base, T, tx_one{s_cols[wv][l0], nk & 0xFFu}, key, tag, P, c.hdr, lane);
    else txs_payload<MODE>(base, T, tx_run{&s_cols[wv][l0], &s_n[wv][l0], cnt}, key, tag, P, c.hdr, lane);
  }
}

/* The emit with held symbols (NRQ_TX_HELD): the wave shape of nrq_emit_set_syms_kernel with the admission of
 * nrq_emit_held_syms_kernel, a kernel of its own so that both are compiled from the code they always were.  Admission (hss_packet,
 * runs_set_body.h): a ready block's packet goes the usual way; one of a block that is not ready is written iff the reception behind
 * its segment holds EVERY one of its symbols -- each lane asks for its slot's seen bit in the segment's books, read through the
 * table pointer, and a ballot over the packet's lanes decides, so a packet is written whole or not at all.  Held source symbols
 * are source rows e .. e+c-1; the rows of held repair symbols are found per packet by the wave that writes it, in one walk over the
 * block's repair list in trips of 64 into the LDS slot heads, and the packet is then one run over single-row lists from the base
 * of the block's repair rows. */
template <int MODE>
__global__ __launch_bounds__(256) void nrq_emit_set_held_syms_kernel(const txs_tab *__restrict__ t, txs_ready rdy, txs_call c, sy_tx y) {
  __shared__ uint32_t s_cols[TX_WAVES][TX_WAVE_PKTS][TX_COLS];
  __shared__ uint32_t s_n[TX_WAVES][TX_WAVE_PKTS], s_tag[TX_WAVES][TX_WAVE_PKTS], s_k[TX_WAVES][TX_WAVE_PKTS];
  __shared__ uint32_t s_seg[TX_WAVES][TX_WAVE_PKTS], s_key[TX_WAVES][TX_WAVE_PKTS];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint32_t G = y.G, per = 64u / G, p = lane / G, i = lane - p * G;
  const uint64_t w0 = ((uint64_t)blockIdx.x * TX_WAVES + wv) * per; /* the wave's first packet in the work order */
  {
    uint32_t n = 0, cnt = 0, tag0 = 0, k = 0, sg = TXS_NONE, key = 0, ready = 0, kind = TX_READY;
    int32_t code = TX_FOREIGN;
    bool mine = p < per && w0 + p < c.n;
    if (mine) {
      k = c.order[w0 + p];
      mine = k < c.n; /* (always: the work order is a permutation) */
      if (mine) {
        tag0 = c.tags[k];
        key = txs_key_of(&c, k);
        sg = hss_packet(t, &rdy, &y, k, tag0, c.seg[k], &code, &cnt, &ready);
      }
    }
    const uint32_t e = tag0 & SY_ESI_MAX;
    /* all or nothing: every slot of a packet of a block that is not ready must be held (every lane of the wave takes the ballot) */
    bool ok = true;
    if (sg < TXS_MAX_SEGS && !ready && i < cnt) ok = hss_slot_held(t, sg, tag0, e + i);
    const uint64_t held = __ballot(ok), pmask = (cnt >= 64u ? ~0ull : (1ull << cnt) - 1ull) << (p * G);
    if (sg < TXS_MAX_SEGS && !ready) {
      if ((held & pmask) != pmask) { code = TX_NOT_READY; cnt = 0u; sg = TXS_NONE; }
      else kind = hss_kind(t, sg, tag0);
    }
    if (sg < TXS_MAX_SEGS && i < cnt) {
      if (kind == TX_HELD_REP) { s_cols[wv][lane][0] = TX_NONE; n = 1u; } /* (the row index: found below) */
      else n = tx_rows(&t->seg[sg].b, tag0 + i, s_cols[wv][lane]);        /* (a held source symbol: row e + i, as a ready one) */
    }
    if (mine && i == 0u && c.results && kind != TX_HELD_REP) c.results[k] = code; /* (held repair symbols: once the rows are found) */
    s_n[wv][lane] = n | (cnt << 8) | (kind << 16); /* (cnt = 0: the packet stays untouched) */
    s_tag[wv][lane] = tag0;
    s_k[wv][lane] = k;
    s_seg[wv][lane] = sg;
    s_key[wv][lane] = key;
  }
  __syncthreads();
  const uint32_t T = c.T;
  for (uint32_t q = 0; q < per && w0 + q < c.n; q++) { /* (wave-uniform) */
    const uint32_t l0 = q * G;
    const uint32_t nk = __builtin_amdgcn_readfirstlane(s_n[wv][l0]), cnt = (nk >> 8) & 0xFFu;
    if (!cnt) continue; /* no member, a refused range, a block that is not ready with a symbol that is not held */
    const uint32_t tag = __builtin_amdgcn_readfirstlane(s_tag[wv][l0]);
    const uint32_t k = __builtin_amdgcn_readfirstlane(s_k[wv][l0]);
    const uint32_t key = __builtin_amdgcn_readfirstlane(s_key[wv][l0]);
    const txs_seg *S = &t->seg[__builtin_amdgcn_readfirstlane(s_seg[wv][l0])];
    const uint8_t *base;
    if ((nk >> 16) == TX_HELD_REP) {
      const tx_held_seg *hs = &S->h;
      const uint32_t b = (tag >> 24) - S->b.sbn0;
      const uint32_t nrep = tx_held_nrep(hs, b), e = tag & SY_ESI_MAX;
      for (uint32_t q0 = 0; q0 < nrep; q0 += 64u) {
        const uint32_t x = q0 + lane < nrep ? hs->rep_esi[(uint64_t)b * hs->rep_cap + q0 + lane] - e : TX_NONE;
        if (x < cnt) s_cols[wv][l0 + x][0] = q0 + lane;
      }
      /* the wave reads what its other lanes wrote: LDS operations of one wave complete in order; the fence keeps the compiler from
       * moving the reads above the writes */
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      const bool found = lane >= cnt || s_cols[wv][l0 + lane][0] != TX_NONE;
      const bool all = __ballot(!found) == 0ull;
      if (c.results && lane == 0) c.results[k] = all ? 0 : TX_NOT_READY;
      if (!all) continue; /* (the books say otherwise: a marked repair ESI has its row) */
      base = tx_held_rep_base(hs, b);
    } else {
      base = tx_base(&S->b, tag);
    }
    uint8_t *P = c.pkts + (uint64_t)k * c.pkt_stride;
    if (cnt == 1u) txs_payload<MODE>(base, T, tx_one{s_cols[wv][l0], nk & 0xFFu}, key, tag, P, c.hdr, lane);
    else txs_payload<MODE>(base, T, tx_run{&s_cols[wv][l0], &s_n[wv][l0], cnt}, key, tag, P, c.hdr, lane);
  }
}

extern "C" {

int nrq_rxset_add_syms(nrq_rxset *set, const void *d_pkts, size_t pkt_stride, const uint32_t *d_keys, const uint32_t *d_tags, uint32_t n,
                       uint32_t G, const uint8_t *d_nsym, uint32_t flags, int32_t *d_results) {
  if (!set) return -1;
  nrq_ctx *ctx = set->ctx;
  const char *who = "nrq_rxset_add_syms";
  const bool inl = (flags & NRQ_RX_TAG_INLINE) != 0, kinl = (flags & NRQ_RX_KEY_INLINE) != 0;
  if (flags & ~(uint32_t)(NRQ_RX_TAG_INLINE | NRQ_RX_KEY_INLINE)) return fail(ctx, -1, "%s: unknown flags 0x%x", who, flags);
  if (kinl && !inl) return fail(ctx, -1, "%s: NRQ_RX_KEY_INLINE needs NRQ_RX_TAG_INLINE", who);
  if (kinl && d_keys) return fail(ctx, -1, "%s: give either d_keys or NRQ_RX_KEY_INLINE", who);
  if (G == 0 || G > NRQ_PKT_SYMS_MAX) return fail(ctx, -1, "%s: G=%u outside 1..%u", who, G, NRQ_PKT_SYMS_MAX);
  if (n == 0 || set->mem.empty()) return 0;
  const uint32_t T = set->T, poff = kinl ? 8u : inl ? 4u : 0u;
  const size_t pkt_len = (uint64_t)G * T > 0xFFFFFFFFu ? SIZE_MAX : (size_t)G * T + poff;
  ings_call s{};
  ing_call &c = s.c;
  sy_rx y{};
  y.G = G; y.nsym = d_nsym;
  uint8_t *tail; /* the packets' members (a word per packet), then the slots' kinds (a byte per slot) */
  const int rc = ing_call_of(ctx, set->scratch, who, d_pkts, pkt_stride, d_tags, n, G, pkt_len, inl, set->nblk, d_results,
                             rx_al((size_t)n * 4u) + (size_t)n * G, &c, &tail);
  if (rc) return rc;
  s.keys = d_keys;
  s.key_inline = kinl ? 1u : 0u;
  s.mem = (uint32_t *)tail;
  y.kind = tail + rx_al((size_t)n * 4u);
  uintptr_t al = reinterpret_cast<uintptr_t>(d_pkts) | pkt_stride | poff | T;
  for (const rxset_member &m : set->mem) {
    const ing_rx &r = m.rx->r;
    al |= reinterpret_cast<uintptr_t>(r.src) | r.src_stride | reinterpret_cast<uintptr_t>(r.rep) | r.rep_stride;
  }
  const uint32_t word = sy_copy_word(al);
  const ings_tab *t = (const ings_tab *)set->tab;
  hipStream_t st = ctx->stream;
  const uint32_t g = (c.n + 255u) / 256u, nb = set->nblk;
  hipLaunchKernelGGL(nrq_ings_first_syms_kernel, dim3(g), dim3(256), 0, st, t, s, y);
  hipLaunchKernelGGL(nrq_ings_done_kernel, dim3(nb), dim3(256), 0, st, t);
  hipLaunchKernelGGL(nrq_ings_hist_syms_kernel, dim3(c.ntiles), dim3(256), nb * 4u, st, t, s, y);
  hipLaunchKernelGGL(nrq_ings_scan_kernel, dim3(nb), dim3(256), 0, st, t, s);
  hipLaunchKernelGGL(nrq_ings_classify_syms_kernel, dim3(c.ntiles), dim3(256), nb * 16u, st, t, s, y);
  const dim3 cg((n + 3u) / 4u);
  if (word == 16u)
    hipLaunchKernelGGL(nrq_ing_copy_syms_kernel<uint4>, cg, dim3(256), 0, st, c.pkts, c.pkt_stride, (const uint64_t *)c.dst, n, G, T, poff);
  else if (word == 4u)
    hipLaunchKernelGGL(nrq_ing_copy_syms_kernel<uint32_t>, cg, dim3(256), 0, st, c.pkts, c.pkt_stride, (const uint64_t *)c.dst, n, G, T, poff);
  else
    hipLaunchKernelGGL(nrq_ing_copy_syms_kernel<uint8_t>, cg, dim3(256), 0, st, c.pkts, c.pkt_stride, (const uint64_t *)c.dst, n, G, T, poff);
  hipLaunchKernelGGL(nrq_ings_fold_syms_kernel, dim3(g), dim3(256), 0, st, t, s, y);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

int nrq_txset_emit_syms(nrq_txset *set, const uint32_t *d_keys, const uint32_t *d_tags, uint32_t n, uint32_t G, const uint8_t *d_nsym,
                        void *d_pkts, size_t pkt_stride, uint32_t flags, int32_t *d_results) {
  using set_fn = void (*)(const txs_tab *, txs_ready, txs_call, sy_tx);
  static const set_fn kern[5] = {nrq_emit_set_syms_kernel<TX_V16>, nrq_emit_set_syms_kernel<TX_V16_SHIFT>, nrq_emit_set_syms_kernel<TX_DWORD>,
                                 nrq_emit_set_syms_kernel<TX_BYTE>, nrq_emit_set_syms_kernel<TXS_V16_KEY>}; /* [mode] */
  static const set_fn hkern[5] = {nrq_emit_set_held_syms_kernel<TX_V16>, nrq_emit_set_held_syms_kernel<TX_V16_SHIFT>,
                                  nrq_emit_set_held_syms_kernel<TX_DWORD>, nrq_emit_set_held_syms_kernel<TX_BYTE>,
                                  nrq_emit_set_held_syms_kernel<TXS_V16_KEY>}; /* [mode] */
  if (!set) return -1;
  nrq_ctx *ctx = set->ctx;
  const char *who = "nrq_txset_emit_syms";
  const bool inl = (flags & NRQ_TX_TAG_INLINE) != 0, kinl = (flags & NRQ_TX_KEY_INLINE) != 0, held = (flags & NRQ_TX_HELD) != 0;
  if (held) { /* (as nrq_tx_emit_syms on a sender: where no member reads a reception the flag could do nothing; an empty set and
               * n = 0 included -- the refusal comes before their early return) */
    bool relay = false;
    for (const txset_member &m : set->mem) relay = relay || m.tx->relay;
    if (!relay) return fail(ctx, -1, "%s: NRQ_TX_HELD needs a relay among the members (a sender holds no reception)", who);
  }
  if (flags & ~(uint32_t)(NRQ_TX_TAG_INLINE | NRQ_TX_HELD | NRQ_TX_KEY_INLINE)) return fail(ctx, -1, "%s: unknown flags 0x%x", who, flags);
  if (kinl && !inl) return fail(ctx, -1, "%s: NRQ_TX_KEY_INLINE needs NRQ_TX_TAG_INLINE", who);
  if (G == 0 || G > NRQ_PKT_SYMS_MAX) return fail(ctx, -1, "%s: G=%u outside 1..%u", who, G, NRQ_PKT_SYMS_MAX);
  if (n == 0 || set->mem.empty()) return 0;
  if (!d_pkts) return fail(ctx, -1, "%s: d_pkts is NULL", who);
  if (!d_tags || (uint64_t)n * G > 0x7FFFFFFFu) return fail(ctx, -1, "%s: bad tags (n=%u, G=%u)", who, n, G);
  const uint32_t hdr = kinl ? 8u : inl ? 4u : 0u;
  if ((uint64_t)G * set->T > 0xFFFFFFFFu || pkt_stride < (size_t)G * set->T + hdr)
    return fail(ctx, -1, "%s: pkt_stride %zu shorter than a packet of %u symbols", who, pkt_stride, G);
  txs_ready rdy;
  txs_call c;
  int mode;
  const int rc = txset_call_of(set, who, d_keys, d_tags, n, d_pkts, pkt_stride, hdr, held, d_results, &rdy, &c, &mode);
  if (rc) return rc;
  sy_tx y{};
  y.G = G; y.nsym = d_nsym;
  const uint32_t per = 64u / G, waves = (n + per - 1u) / per;
  hipLaunchKernelGGL((held ? hkern : kern)[mode], dim3((waves + TX_WAVES - 1u) / TX_WAVES), dim3(64u * TX_WAVES), 0, ctx->stream, (const txs_tab *)set->tab, rdy,
                     c, y);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

} /* extern "C" */

/* ================================================ sender sets: the range mode (nrq_txset_emit_all*, emit_set_range_body.h) ==== */
/* The packets of "the next symbols of every block of every member" with no list from the host: ONE pass computes the packet map
 * (emit_set_range_body.h states it) into the (keys, tags, nsym) lists, the packets' segments and the work order, in the set's
 * scratch or in the caller's out arrays; behind it run the list route's payload kernels (nrq_emit_set_kernel,
 * nrq_emit_set_syms_kernel) on those arrays, by the list route's path rule.  One thread per work item in block-major order; the
 * per-segment words are staged in LDS (at most 64 entries: every lane of a block's run reads the same one, as in
 * nrq_txs_hist_kernel), each thread walks them once for its segment and once for its packet index. */
__global__ __launch_bounds__(256) void nrq_txs_range_kernel(const txs_tab *__restrict__ t, txr_call c) {
  __shared__ txr_stage_t s;
  const uint32_t nseg = min(t->nseg, TXS_MAX_SEGS), i = threadIdx.x;
  if (i < nseg) txr_stage(t, &c, i, &s);
  __syncthreads();
  if (i <= nseg) txr_stage_prefix(nseg, i, &s);
  __syncthreads();
  const uint32_t w = blockIdx.x * 256u + i;
  if (w < c.n && w < s.pre[nseg]) txr_map(&s, nseg, &c, w);
}

/* the packets of a range call from the host's copy of the table: *total, and per block in block order h_cnt (nullable).  The
 * checks nrq_txset_count_all and the emits share: G, source, the ESI bound, the totals. */
static int txset_range_count(nrq_txset *set, const char *who, uint32_t source, uint32_t rep0, uint32_t nrep, uint32_t G, uint32_t *h_cnt,
                             uint32_t *total) {
  nrq_ctx *ctx = set->ctx;
  if (G == 0 || G > NRQ_PKT_SYMS_MAX) return fail(ctx, -1, "%s: G=%u outside 1..%u", who, G, NRQ_PKT_SYMS_MAX);
  if (source > 1u) return fail(ctx, -1, "%s: source %u is neither 0 nor 1", who, source);
  uint32_t kmax = 0;
  for (const txset_seg &r : set->segs) kmax = std::max(kmax, r.tx->s.seg[r.g].K);
  if (nrep && (uint64_t)kmax + rep0 + nrep - 1u > 0xFFFFFFu)
    return fail(ctx, -1, "%s: repair ESIs up to %llu reach past 2^24 - 1", who, (unsigned long long)((uint64_t)kmax + rep0 + nrep - 1u));
  uint64_t n = 0;
  for (const txset_seg &r : set->segs) {
    const tx_blk &t = r.tx->s.seg[r.g];
    n += (uint64_t)t.nblk * txr_len(t.K, source, nrep, G);
  }
  if (n > 0x7FFFFFFFu || n * G > 0x7FFFFFFFu)
    return fail(ctx, -1, "%s: %llu packets of %u symbols are more than one call takes", who, (unsigned long long)n, G);
  *total = (uint32_t)n;
  if (h_cnt) {
    uint32_t g = 0;
    for (const txset_seg &r : set->segs) {
      const tx_blk &t = r.tx->s.seg[r.g];
      for (uint32_t b = 0; b < t.nblk; b++) h_cnt[g++] = txr_len(t.K, source, nrep, G);
    }
  }
  return 0;
}

/* The one function behind nrq_txset_emit_all and nrq_txset_emit_all_syms (syms: the several-symbol payload kernels and the
 * counts; else G = 1 and the one-symbol kernels).  Checks first; then txset_prepare as the list route; the map pass; the emit. */
static int txset_range(nrq_txset *set, const char *who, bool syms, uint32_t source, uint32_t rep0, uint32_t nrep, uint32_t G, int order,
                       void *d_pkts, size_t pkt_stride, uint32_t flags, uint32_t *d_keys_out, uint32_t *d_tags_out, uint8_t *d_nsym_out,
                       uint32_t *h_npkt) {
  using set_fn = void (*)(const txs_tab *, txs_ready, txs_call);
  using syms_fn = void (*)(const txs_tab *, txs_ready, txs_call, sy_tx);
  static const set_fn kern[5] = {nrq_emit_set_kernel<TX_V16, false>, nrq_emit_set_kernel<TX_V16_SHIFT, false>, nrq_emit_set_kernel<TX_DWORD, false>,
                                 nrq_emit_set_kernel<TX_BYTE, false>, nrq_emit_set_kernel<TXS_V16_KEY, false>}; /* [mode] */
  static const syms_fn skern[5] = {nrq_emit_set_syms_kernel<TX_V16>, nrq_emit_set_syms_kernel<TX_V16_SHIFT>, nrq_emit_set_syms_kernel<TX_DWORD>,
                                   nrq_emit_set_syms_kernel<TX_BYTE>, nrq_emit_set_syms_kernel<TXS_V16_KEY>}; /* [mode] */
  if (!set) return -1;
  nrq_ctx *ctx = set->ctx;
  const bool inl = (flags & NRQ_TX_TAG_INLINE) != 0, kinl = (flags & NRQ_TX_KEY_INLINE) != 0;
  if (flags & ~(uint32_t)(NRQ_TX_TAG_INLINE | NRQ_TX_HELD | NRQ_TX_KEY_INLINE)) return fail(ctx, -1, "%s: unknown flags 0x%x", who, flags);
  if (flags & NRQ_TX_HELD) return fail(ctx, -1, "%s: NRQ_TX_HELD goes with a tag list (the range forms map packets to every block)", who);
  if (kinl && !inl) return fail(ctx, -1, "%s: NRQ_TX_KEY_INLINE needs NRQ_TX_TAG_INLINE", who);
  if (order != 0 && order != 1) return fail(ctx, -1, "%s: order %d is neither 0 (block-major) nor 1 (interleaved)", who, order);
  uint32_t n = 0;
  int rc = txset_range_count(set, who, source, rep0, nrep, G, nullptr, &n);
  if (rc) return rc;
  if (n == 0) { /* an empty set; neither source nor repair symbols */
    if (h_npkt) *h_npkt = 0;
    return 0;
  }
  if (!d_pkts) return fail(ctx, -1, "%s: d_pkts is NULL", who);
  const uint32_t hdr = kinl ? 8u : inl ? 4u : 0u;
  if ((uint64_t)G * set->T > 0xFFFFFFFFu || pkt_stride < (size_t)G * set->T + hdr)
    return fail(ctx, -1, "%s: pkt_stride %zu shorter than a packet of %u symbols", who, pkt_stride, G);
  /* every block is in the map, so every block must be ready (as nrq_tx_emit_range on a relay) */
  for (const txset_seg &r : set->segs) {
    const tx_sender *tx = r.tx;
    if (!tx->relay || tx->detached) continue; /* (a detached relay: txset_prepare says so) */
    const tx_blk &t = tx->s.seg[r.g];
    for (uint32_t b = 0; b < t.nblk; b++)
      if (!tx_is_ready(tx, t.sbn0 + b - tx->s.sbn0))
        return fail(ctx, -1, "%s: a block of the relay under key %u is not ready: SBN %u", who, txset_key_of(set, tx), t.sbn0 + b);
  }
  /* the per-packet arrays: segments and work order always in the scratch, the lists there unless the caller takes them */
  const size_t words = rx_al((size_t)n * 4u);
  size_t need = 2u * words;
  const size_t o_keys = need;
  if (!d_keys_out) need += words;
  const size_t o_tags = need;
  if (!d_tags_out) need += words;
  const size_t o_nsym = need;
  if (syms && !d_nsym_out) need += rx_al((size_t)n);
  txs_ready rdy;
  int mode;
  if ((rc = txset_prepare(set, who, need, d_pkts, pkt_stride, hdr, false, &rdy, &mode))) return rc;
  uint8_t *p = (uint8_t *)set->scratch.p;
  txr_call r{};
  r.source = source; r.rep0 = rep0; r.nrep = nrep; r.G = G;
  r.order = (uint32_t)order;
  r.n = n;
  r.seg = (uint32_t *)p;
  r.worder = (uint32_t *)(p + words);
  r.keys = d_keys_out ? d_keys_out : (uint32_t *)(p + o_keys);
  r.tags = d_tags_out ? d_tags_out : (uint32_t *)(p + o_tags);
  r.nsym = !syms ? nullptr : d_nsym_out ? d_nsym_out : p + o_nsym;
  txs_call c{};
  c.pkts = (uint8_t *)d_pkts;
  c.pkt_stride = pkt_stride;
  c.n = n;
  c.hdr = hdr;
  c.T = set->T;
  c.keys = r.keys;
  c.tags = r.tags;
  c.seg = r.seg;
  c.order = r.worder;
  const txs_tab *t = (const txs_tab *)set->tab;
  hipStream_t st = ctx->stream;
  hipLaunchKernelGGL(nrq_txs_range_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, t, r);
  HIPCHK(ctx, hipGetLastError());
  if (syms) {
    sy_tx y{};
    y.G = G; y.nsym = r.nsym;
    const uint32_t per = 64u / G, waves = (n + per - 1u) / per;
    hipLaunchKernelGGL(skern[mode], dim3((waves + TX_WAVES - 1u) / TX_WAVES), dim3(64u * TX_WAVES), 0, st, t, rdy, c, y);
  } else {
    hipLaunchKernelGGL(kern[mode], dim3((n + TX_WAVES * TX_WAVE_PKTS - 1u) / (TX_WAVES * TX_WAVE_PKTS)), dim3(64u * TX_WAVES), 0, st, t, rdy, c);
  }
  HIPCHK(ctx, hipGetLastError());
  if (h_npkt) *h_npkt = n;
  return 0;
}

extern "C" {

int nrq_txset_count_all(nrq_txset *set, uint32_t source, uint32_t nrep, uint32_t G, uint32_t *h_cnt, uint32_t *h_npkt) {
  if (!set) return -1;
  uint32_t n = 0;
  const int rc = txset_range_count(set, "nrq_txset_count_all", source, 0, nrep, G, h_cnt, &n);
  if (rc) return rc;
  if (h_npkt) *h_npkt = n;
  return 0;
}

int nrq_txset_emit_all(nrq_txset *set, uint32_t source, uint32_t rep0, uint32_t nrep, int order, void *d_pkts, size_t pkt_stride, uint32_t flags,
                       uint32_t *d_keys_out, uint32_t *d_tags_out, uint32_t *h_npkt) {
  return txset_range(set, "nrq_txset_emit_all", false, source, rep0, nrep, 1u, order, d_pkts, pkt_stride, flags, d_keys_out, d_tags_out, nullptr,
                     h_npkt);
}

int nrq_txset_emit_all_syms(nrq_txset *set, uint32_t source, uint32_t rep0, uint32_t nrep, uint32_t G, int order, void *d_pkts, size_t pkt_stride,
                            uint32_t flags, uint32_t *d_keys_out, uint32_t *d_tags_out, uint8_t *d_nsym_out, uint32_t *h_npkt) {
  return txset_range(set, "nrq_txset_emit_all_syms", true, source, rep0, nrep, G, order, d_pkts, pkt_stride, flags, d_keys_out, d_tags_out,
                     d_nsym_out, h_npkt);
}

} /* extern "C" */
