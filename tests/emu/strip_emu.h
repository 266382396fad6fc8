/*
 * strip_emu.h -- one strip of the solve, from the staging buffer to the output staging buffer, on the CPU (TEST SUPPORT ONLY).
 *
 * The phase functions of nanorq_amd/csrc/solve_body.h with the workgroup's barriers turned into loop boundaries: the threads of
 * a phase run one after the other.  Shared by solve_emu.cpp (one work slot, arrays of the caller's) and launch_emu.cpp (the
 * whole launch as nrq_solve_kernel deals it out, on fenced memory).  Included behind solve_body.h.  An emulation that included
 * wave_emu.h in front of solve_body.h gets ph_store's fast form with wave-wide ballots.
 *
 * G > 1 (wide strips): thread t is lane t % G of virtual thread t / G, c[lane] carries the lane's column of the image and the
 * phases run on the NT / G virtual threads, as in the kernel.
 */
#ifndef NRQ_STRIP_EMU_H
#define NRQ_STRIP_EMU_H

#include <vector>

#include "../../nanorq_amd/csrc/solve_roles.h" /* SolveRoles: which compiled form of a phase the workgroup runs */

/* The forward passes in the order the kernel's wave 0 issues them (plan.h): step q applies row q-NRQ_PIPE,
 * then reads the sources of row q -- so a plan that puts dependent rows closer than NRQ_PIPE rows apart
 * produces wrong symbols here, exactly as it would on the GPU. */
template <int WB, int G> static bool emu_forward(const StripCtx<WB, G> *c) {
  const uint32_t *ops = c[0].template arr<uint32_t>(c[0].h->off_ops);
  const uint32_t nrows = c[0].h->nrows, P = NRQ_PIPE;
  if (c[0].h->pipe != NRQ_PIPE) return false;
  std::vector<SV<WB>> v((size_t)(P + 1) * NRQ_ROW * G);
  for (uint32_t q = 0; q < nrows + P; q++) {
    if (q >= P) {
      const SV<WB> *vr = &v[(size_t)((q - P) % (P + 1)) * NRQ_ROW * G];
      for (uint32_t l = 0; l < NRQ_ROW; l++)
        for (uint32_t s = 0; s < (uint32_t)G; s++) lds_xor<WB, G>(c[s].lds, ops[NRQ_OP_INDEX(q - P, l)] & 0xFFFFu, vr[l * G + s]);
    }
    if (q < nrows) {
      SV<WB> *vr = &v[(size_t)(q % (P + 1)) * NRQ_ROW * G];
      for (uint32_t l = 0; l < NRQ_ROW; l++)
        for (uint32_t s = 0; s < (uint32_t)G; s++) vr[l * G + s] = lds_get<WB, G>(c[s].lds, ops[NRQ_OP_INDEX(q, l)] >> 16);
    }
  }
  return true;
}

/* One strip: the image from `stage` (this strip's input staging buffer), every phase, the results into `ostage` (this strip's
 * output staging buffer).  c[0 .. G): the context of every lane; NT threads; f: the phases' forms (HNT and the five below it); raw: the split solve, which stops after the dense
 * stage (ph_store_raw).  1, or -7 for a plan of another pipeline depth. */
template <int WB, int G>
static int strip_phases(const StripCtx<WB, G> *c, uint32_t NT, const SolveRoles &f, const uint8_t *stage, uint8_t *ostage, bool raw) {
  const uint32_t VNT = NT / G;
  auto each = [&](uint32_t n, auto fn) {
    for (uint32_t t = 0; t < n; t++) fn(c[t % G], t / G, (uint32_t)(t % G));
  };
  typedef const StripCtx<WB, G> &CX;
  each(NT, [&](CX x, uint32_t vt, uint32_t sub) {
    if (f.commit_pb == 8) pf_commit<WB, G, 8>(x, stage + sub * WB, 0u, vt, VNT);
    else pf_commit<WB, G, 4>(x, stage + sub * WB, 0u, vt, VNT);
  });
  each(NT, [&](CX x, uint32_t vt, uint32_t) { ph_clear<WB, G>(x, vt, VNT); });
  if (!emu_forward<WB, G>(c)) return -7;
  each(f.HNT, [&](CX x, uint32_t vt, uint32_t) {
    if constexpr (G == 1) {
      if (f.hdpc_regs) { ph_hdpc<WB, G, true>(x, vt, f.HNT / G); return; }
    }
    ph_hdpc<WB, G, false>(x, vt, f.HNT / G);
  });
  each(NT, [&](CX x, uint32_t vt, uint32_t) { ph_hdpc_reduce<WB, G>(x, vt, VNT); });
  const uint32_t lpr = c[0].h->lpr;
  for (uint32_t w0 = 0; w0 < lpr; w0 += low_table_words<WB, G>(c[0])) {
    each(NT, [&](CX x, uint32_t vt, uint32_t) { ph_low_tables<WB, G>(x, w0, vt, VNT); });
    each(NT, [&](CX x, uint32_t vt, uint32_t) {
      uint32_t cb[NRQ_COMBINE_WU];
      ph_combine_fetch<WB, G>(x, w0, vt, VNT, cb);
      ph_combine<WB, G>(x, w0, vt, VNT, cb);
    });
  }
  if (lpr) each(NT, [&](CX x, uint32_t vt, uint32_t) { ph_clear_x<WB, G>(x, vt, VNT); });
  each(NT, [&](CX x, uint32_t vt, uint32_t) {
    if (f.fold_batch) ph_dense_fold<WB, G, 8>(x, vt, VNT);
    else ph_dense_fold<WB, G, 0>(x, vt, VNT);
  });
  if (dense_fold_shared(VNT) || G > 1) each(NT, [&](CX x, uint32_t vt, uint32_t) { ph_hdpc_reduce<WB, G>(x, vt, VNT); });
  each(NT, [&](CX x, uint32_t vt, uint32_t) {
    if (f.batch) ph_dense_free<WB, G, true>(x, vt, VNT);
    else ph_dense_free<WB, G, false>(x, vt, VNT);
  });
  each(NT, [&](CX x, uint32_t vt, uint32_t) {
    if (f.batch) ph_dense_cu<WB, G, true>(x, vt, VNT);
    else ph_dense_cu<WB, G, false>(x, vt, VNT);
  });
  if (raw) { /* the split solve: slot image and C_u staged, nrq_backsub_kernel / nrq_collect_kernel finish */
    each(NT, [&](CX x, uint32_t vt, uint32_t sub) { ph_store_raw<WB, G>(x, ostage + sub * WB, vt, VNT); });
    return 1;
  }
  each(NT, [&](CX x, uint32_t vt, uint32_t) { ph_tables<WB, G>(x, vt, VNT); });
  each(NT, [&](CX x, uint32_t vt, uint32_t) {
    if (f.fast) ph_backsub<WB, G, true>(x, vt, VNT);
    else ph_backsub<WB, G, false>(x, vt, VNT);
  });
  each(NT, [&](CX x, uint32_t vt, uint32_t) { ph_park<WB, G>(x, vt, VNT); });
#ifdef NRQ_WAVE_EMU_H
  if (f.fast) { /* the fast form loops under wave-wide ballots: a wave's 64 lanes in step (wave_emu.h), as on the device */
    for (uint32_t t0 = 0; t0 < NT; t0 += 64u)
      wave_in_step(NT - t0 < 64u ? NT - t0 : 64u, [&](unsigned l) { const uint32_t t = t0 + l; ph_store<WB, G, true>(c[t % G], ostage + (t % G) * WB, t / G, VNT); });
    return 1;
  }
#endif
  each(NT, [&](CX x, uint32_t vt, uint32_t sub) {
    if (f.fast) ph_store<WB, G, true>(x, ostage + sub * WB, vt, VNT);
    else ph_store<WB, G, false>(x, ostage + sub * WB, vt, VNT);
  });
  return 1;
}

/* ---- the second half of a split solve (split_body.h) ---- */

/* nrq_backsub_kernel<SB> on grid (gridx, nchunks) for one block: Y = its work buffer.  Workgroups run one after the other,
 * the last first (they share nothing but the rows they read: any order gives the same buffer), each with tables of its own in
 * garbage-filled "LDS".  -2: a workgroup was given a strip the row does not have. */
template <int SB> static int run_backsub(const uint8_t *plan, uint8_t *Y, uint32_t T, uint32_t gridx, uint32_t nchunks) {
  const nrq_plan_hdr *h = reinterpret_cast<const nrq_plan_hdr *>(plan);
  std::vector<uint8_t> lds((size_t)h->wpr * 8u * 16u * SB + 64, 0xA5);
  uint8_t *tbl = reinterpret_cast<uint8_t *>((reinterpret_cast<uintptr_t>(lds.data()) + 15) & ~(uintptr_t)15);
  for (uint32_t chunk = nchunks; chunk-- > 0;)
    for (uint32_t wg = gridx; wg-- > 0;) {
      SplitCtx<SB> c;
      const uint32_t strip = sp_strip_of<SB>(wg, gridx);
      if (!sp_ctx<SB>(c, plan, Y, T, strip)) return 0;
      if ((uint64_t)strip * SB >= T) return -2;
      memset(tbl, 0xA5, (size_t)h->wpr * 8u * 16u * SB);
      for (uint32_t t = 0; t < SP_NT; t++) sp_tables<SB>(c, tbl, t);
      for (uint32_t t = 0; t < SP_NT; t++) sp_backsub<SB>(c, tbl, chunk, nchunks, t);
    }
  return 1;
}

/* nrq_collect_kernel on grid x = grid_e for one block: F = the final slot image */
static int run_collect(const nrq_job *job, uint32_t T, const uint8_t *F, uint32_t grid_e) {
  const uint8_t *plan = reinterpret_cast<const uint8_t *>(job->plan);
  const nrq_plan_hdr *h = reinterpret_cast<const nrq_plan_hdr *>(plan);
  if (h->status) return 0;
  for (uint32_t e = 0; e < grid_e; e++) {
    if (e >= sc_elems(job, h)) continue;
    uint32_t rows[RQ_MAX_LT_COLS + 1], nrows = 0xA5A5A5A5u;
    for (uint32_t k = 0; k <= RQ_MAX_LT_COLS; k++) rows[k] = 0xA5A5A5A5u;
    uint8_t *dst[SP_NT];
    for (uint32_t t = 0; t < SP_NT; t++) dst[t] = sc_fetch(job, plan, e, T, t, rows, &nrows);
    for (uint32_t t = 0; t < SP_NT; t++) sc_sum(F, dst[t], T, rows, nrows, t);
  }
  return 1;
}

#endif /* NRQ_STRIP_EMU_H */
