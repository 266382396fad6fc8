/*
 * split_body.h -- the bodies of the second half of a split solve (narrow strips, WB <= 4; nrq_device.hip "split solve of big
 * blocks"): the back-substitution on SB-byte strips of the full-width rows of a block's work buffer, and the collection of the
 * results from the final slot image, as per-thread phase functions.
 *
 * nrq_backsub_kernel<SB> and nrq_collect_kernel (nrq_device.hip) run them with a workgroup barrier between the phases;
 * tests/emu/solve_emu.cpp runs the 256 threads of a phase in a loop on the CPU.  The LDS arrays are the caller's.
 *
 * Work buffer of a block: rows [0, M) the slot image (Y at the pivots' slots), rows [M, M + u) C_u, T bytes each.
 *   sp_strip_of     the strip a workgroup of the back-substitution grid takes
 *   sp_tables       phase 1: 16-entry XOR tables over groups of 4 inactive columns, for the workgroup's strip
 *   sp_backsub      phase 2: the inactive columns to their slots (chunk 0), then Y(slot) ^= W_k * C_u for the chunk's pivots
 *   sc_fetch        collect, phase 1: the rows an output row is the sum of
 *   sc_sum          collect, phase 2: the sum, 16 bytes or one byte per thread and trip
 */
#ifndef NRQ_SPLIT_BODY_H
#define NRQ_SPLIT_BODY_H

#include <stdint.h>

#include "plan.h"
#include "rq_math.h"
#include "solve_body.h"

#define SP_NT 256u  /* threads of both workgroups */
#define SP_WCH 20u  /* W words of a pivot asked for in one batch */

/* Workgroup i runs on XCD i % 8 (round-robin dispatch).  The strips that share a 128-byte line of every row -- 128 / SB
 * neighbours -- are given to workgroups i, i + 8, i + 16 ... : same XCD, dispatched together, walking the pivots in step, so
 * a line fetched for one of them is in that XCD's L2 for the others (with strip = i the neighbours sat on different XCDs and
 * every one of them fetched the line from HBM: the kernel is bound by its scattered 32-byte row accesses).  A permutation of
 * [0, gridx): whole groups of PER = 8 * 128 / SB workgroups are permuted among themselves, the rest keep their index. */
template <int SB> SB_HD uint32_t sp_strip_of(uint32_t i, uint32_t gridx) {
  constexpr uint32_t NB_ = 128u / SB, PER = 8u * NB_;
  const uint32_t full = (gridx / PER) * PER;
  if (i >= full) return i;
  const uint32_t r = i % PER, g = (i / PER) * 8u + (r & 7u), j = r >> 3;
  return g * NB_ + j;
}

/* pivots [k0, k1) of chunk `chunk` of `nchunks` */
SB_HD void sp_chunk_bounds(uint32_t npiv, uint32_t chunk, uint32_t nchunks, uint32_t *k0, uint32_t *k1) {
  *k0 = (uint32_t)(((uint64_t)npiv * chunk) / nchunks);
  *k1 = (uint32_t)(((uint64_t)npiv * (chunk + 1u)) / nchunks);
}

/* one workgroup's view: a block's plan and work buffer, and the strip's columns */
template <int SB> struct SplitCtx {
  const NRQ_GAS uint16_t *pivslot, *uslot;
  const NRQ_GAS uint32_t *wt; /* W transposed by word: word w of pivot k at [w * stride + k] */
  NRQ_GAS uint8_t *Y;
  const NRQ_GAS uint8_t *Cu;
  uint32_t T, u, wpr, npiv, stride, col0, valid;
};

/* false: the block has no plan to run (status != 0) */
template <int SB> SB_HD bool sp_ctx(SplitCtx<SB> &c, const uint8_t *plan, NRQ_GAS uint8_t *Y, uint32_t T, uint32_t strip) {
  const nrq_plan_hdr *h = reinterpret_cast<const nrq_plan_hdr *>(plan);
  if (h->status) return false;
  c.u = h->u; c.wpr = h->wpr; c.npiv = h->npiv; c.stride = h->npiv_pad;
  c.pivslot = gptr<uint16_t>(plan + h->off_pivslot);
  c.uslot = gptr<uint16_t>(plan + h->off_uslot);
  c.wt = gptr<uint32_t>(plan + h->off_wt);
  c.Y = Y;
  c.Cu = Y + (size_t)h->M * T;
  c.T = T;
  c.col0 = strip * SB;
  const uint32_t rem = T - c.col0;
  c.valid = rem < (uint32_t)SB ? rem : (uint32_t)SB;
  return true;
}

/* the strip's `valid` bytes of a row, as SB / 16 quarters of 16 bytes (bytes beyond `valid`: zero, not written) */
template <int SB> SB_HD void sp_load(const NRQ_GAS uint8_t *p, uint32_t valid, SV<16> (&v)[SB / 16]) {
#pragma unroll
  for (int q = 0; q < SB / 16; q++) {
    const uint32_t o = (uint32_t)q * 16u;
    v[q] = o < valid ? g_get<16>(p + o, valid - o < 16u ? valid - o : 16u) : sv_zero<16>();
  }
}
template <int SB> SB_HD void sp_store(NRQ_GAS uint8_t *p, uint32_t valid, const SV<16> (&v)[SB / 16]) {
#pragma unroll
  for (int q = 0; q < SB / 16; q++) {
    const uint32_t o = (uint32_t)q * 16u;
    if (o < valid) g_put<16>(p + o, valid - o < 16u ? valid - o : 16u, v[q]);
  }
}

/* tables (wpr * 8 * 16 entries of SB bytes): entry (grp, nib) = XOR of C_u[4 grp + b] over the bits b of nib */
template <int SB> SB_HD void sp_tables(const SplitCtx<SB> &c, uint8_t *tbl, uint32_t tid) {
  constexpr int NQ = SB / 16;
  const uint32_t ngroups = c.wpr * 8u;
  for (uint32_t e = tid; e < ngroups * 16u; e += SP_NT) {
    const uint32_t grp = e >> 4, nib = e & 15u;
    SV<16> acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) acc[q] = sv_zero<16>();
#pragma unroll
    for (uint32_t b = 0; b < 4; b++) {
      const uint32_t x = grp * 4u + b;
      if (((nib >> b) & 1u) && x < c.u) {
        SV<16> t[NQ];
        sp_load<SB>(c.Cu + (size_t)x * c.T + c.col0, c.valid, t);
#pragma unroll
        for (int q = 0; q < NQ; q++) sv_xor<16>(acc[q], t[q]);
      }
    }
#pragma unroll
    for (int q = 0; q < NQ; q++) lds_put<16>(tbl, e * NQ + q, acc[q]);
  }
}

/* the first SP_WCH words of W from word w0 on, of pivot k (all loads unconditional: a word beyond wpr re-reads the last one
 * and is not used) */
template <int SB> SB_HD void sp_words(const SplitCtx<SB> &c, uint32_t k, uint32_t w0, uint32_t (&b)[SP_WCH]) {
#pragma unroll
  for (uint32_t j = 0; j < SP_WCH; j++) b[j] = c.wt[(size_t)(w0 + j < c.wpr ? w0 + j : c.wpr - 1u) * c.stride + k];
}

template <int SB> SB_HD void sp_backsub(const SplitCtx<SB> &c, const uint8_t *tbl, uint32_t chunk, uint32_t nchunks, uint32_t tid) {
  constexpr int NQ = SB / 16;
  constexpr uint32_t WCH = SP_WCH;
  const uint32_t wpr = c.wpr, T = c.T, col0 = c.col0, valid = c.valid;
  if (chunk == 0) /* park the inactive columns in the slots the plan reserved for them (rows that are no pivots) */
    for (uint32_t x = tid; x < c.u; x += SP_NT) {
      SV<16> t[NQ];
      sp_load<SB>(c.Cu + (size_t)x * T + col0, valid, t);
      sp_store<SB>(c.Y + (size_t)c.uslot[x] * T + col0, valid, t);
    }
  uint32_t k0, k1;
  sp_chunk_bounds(c.npiv, chunk, nchunks, &k0, &k1);
  /* A pivot per thread and trip: Y(slot) ^= W_k * C_u through the tables.  Everything a pivot needs from memory -- its slot, its
   * row, its first WCH words of W -- is asked for while the pivot BEFORE it does its lookups: before, a pivot was a chain of seven
   * trips (slot, row, five groups of four W words: 12 us per pivot at K'=56403, 1.8 ms per launch, 3.3 ms at K=27000 T=65504). */
  uint32_t k = k0 + tid;
  if (k >= k1) return;
  uint32_t bits_n[WCH];
  SV<16> acc_n[NQ];
  NRQ_GAS uint8_t *row_n = c.Y + (size_t)c.pivslot[k] * T + col0;
  sp_load<SB>(row_n, valid, acc_n);
  sp_words<SB>(c, k, 0u, bits_n);
  for (; k < k1; k += SP_NT) {
    SV<16> acc[NQ];
    uint32_t bits[WCH];
    NRQ_GAS uint8_t *row = row_n;
#pragma unroll
    for (int z = 0; z < NQ; z++) acc[z] = acc_n[z];
#pragma unroll
    for (uint32_t j = 0; j < WCH; j++) bits[j] = bits_n[j];
    const uint32_t kn = k + SP_NT;
    if (kn < k1) {
      row_n = c.Y + (size_t)c.pivslot[kn] * T + col0;
      sp_load<SB>(row_n, valid, acc_n);
      sp_words<SB>(c, kn, 0u, bits_n);
    }
    for (uint32_t w0 = 0;;) {
#pragma unroll
      for (uint32_t j = 0; j < WCH; j++) {
        if (w0 + j >= wpr) break;
#pragma unroll
        for (uint32_t q = 0; q < 8; q++) {
          const uint32_t e = ((w0 + j) * 8u + q) * 16u + ((bits[j] >> (4u * q)) & 15u);
#pragma unroll
          for (int z = 0; z < NQ; z++) sv_xor<16>(acc[z], lds_get<16>(tbl, e * NQ + z));
        }
      }
      w0 += WCH;
      if (w0 >= wpr) break;
      sp_words<SB>(c, k, w0, bits); /* (more than WCH words: u > 640) */
    }
    sp_store<SB>(row, valid, acc);
  }
}

/* ---- results: output row e of a block -- intermediate symbol e = row colslot[e] (if the job wants them), or generated symbol
 * q = e - ni = XOR of the rows its list names (plan slots of its LT neighbours), to the row of `out` the job assigns ---- */

/* rows of the block a collect grid has work for */
SB_HD uint32_t sc_elems(const nrq_job *j, const nrq_plan_hdr *h) { return (j->inter ? h->L : 0u) + j->nout; }

/* phase 1: the list into rows[RQ_MAX_LT_COLS + 1] / *nrows (shared by the workgroup); returns the destination row */
SB_HD NRQ_GAS uint8_t *sc_fetch(const nrq_job *j, const uint8_t *plan, uint32_t e, uint32_t T, uint32_t tid, uint32_t *rows, uint32_t *nrows) {
  const nrq_plan_hdr *h = reinterpret_cast<const nrq_plan_hdr *>(plan);
  const uint32_t ni = j->inter ? h->L : 0u;
  if (e < ni) {
    if (tid == 0) { rows[0] = gptr<uint16_t>(plan + h->off_colslot)[e]; *nrows = 1u; }
    return gptr_w<uint8_t>(j->inter) + (size_t)e * T;
  }
  const uint32_t q = e - ni;
  const NRQ_GAS uint32_t *cptr = gptr<uint32_t>(j->out_cptr);
  const NRQ_GAS uint16_t *osl = gptr<uint16_t>(j->out_slots);
  const uint32_t a = cptr[q], n = cptr[q + 1] - a;
  if (tid < n && tid <= RQ_MAX_LT_COLS) rows[tid] = osl[a + tid];
  if (tid == 0) *nrows = n <= RQ_MAX_LT_COLS ? n : RQ_MAX_LT_COLS;
  return gptr_w<uint8_t>(j->out) + (size_t)gptr<uint32_t>(j->out_row)[q] * T;
}

/* phase 2: dst = XOR of rows[0 .. n) of the final slot image F */
SB_HD void sc_sum(const NRQ_GAS uint8_t *F, NRQ_GAS uint8_t *dst, uint32_t T, const uint32_t *rows, uint32_t n, uint32_t tid) {
  const bool vec = (T & 15u) == 0 && ((reinterpret_cast<uintptr_t>(F) | reinterpret_cast<uintptr_t>(dst)) & 15u) == 0;
  if (vec) {
    for (uint32_t off = tid * 16u; off < T; off += SP_NT * 16u) {
      SV<16> acc = sv_zero<16>();
      for (uint32_t k = 0; k < n; k++) sv_xor<16>(acc, g_get_stream<16>(F + (size_t)rows[k] * T + off, 16u));
      g_put<16>(dst + off, 16u, acc);
    }
  } else {
    for (uint32_t off = tid; off < T; off += SP_NT) {
      uint8_t acc = 0;
      for (uint32_t k = 0; k < n; k++) acc ^= F[(size_t)rows[k] * T + off];
      dst[off] = acc;
    }
  }
}

#endif /* NRQ_SPLIT_BODY_H */
