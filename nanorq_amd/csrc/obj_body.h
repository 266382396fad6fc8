/*
 * obj_body.h -- the bodies of the device-resident object layer (nrq_otx_* / nrq_orx_*, include/nanorq_hip.h): an object of F
 * bytes in its RFC 6330 section 4.4.1.2 layout on one side, the row images of its Z source blocks on the other.
 *
 * Layout.  Block b (K_b = KL for b < ZL, else KS) starts at object byte boff(b) = sum of K_c * T over the blocks before it.  Its
 * sub-block j (NL of TL bytes, then NS of TS bytes; col_j = the sum of the widths before it) is the stretch of K_b * T_j bytes at
 * boff(b) + K_b * col_j, row e of it at + e * T_j.  The row image of block b is K_b rows of T bytes, row e = the concatenation of
 * row e of every sub-block, i.e. object byte boff(b) + K_b * col_j + e * T_j + c is row byte e * T + col_j + c.  Every coding
 * operation acts on each byte column on its own, so coding the row image gives exactly the per-sub-block results of the RFC.
 * The row images of all blocks lie back to back, block b's at rows + boff(b) (the same size as its stretch of the object).
 * Object -> rows: bytes at object offset >= F read as zero.  Rows -> object: bytes at object offset >= F are never written.
 *
 * Work.  One workgroup row (blockIdx.y) per block; a work item takes 16-byte windows of the object at 16-byte boundaries
 * (relative to the object's start) that overlap the block, and moves each window as 16 / V pieces of V bytes, V the widest of
 * 16, 8, 4, 2, 1 dividing T, TL and TS: a piece then never straddles a sub-block row, and its row-side address is V-aligned.
 * A window that a block boundary or F cuts goes a byte at a time on the object side, only the block's own bytes.
 * nrq_device.hip instantiates these bodies in nrq_obj_layout_kernel; tests/emu/obj_emu.cpp runs them on the CPU.
 */
#ifndef NRQ_OBJ_BODY_H
#define NRQ_OBJ_BODY_H

#include <stdint.h>

#include "emit_body.h" /* (TX_HD) */

#define OBJ_WIN 16u       /* bytes per object window */
#define OBJ_UNROLL 4u     /* windows per work item (all loaded before any is stored) */
#define OBJ_WG 256u       /* work items per workgroup */

struct obj_lay {
  uint8_t *obj;           /* the object, F bytes */
  uint8_t *rows;          /* block b's row image at rows + boff(b) */
  uint64_t F;
  uint32_t T, Z, ZL, KL, KS;
  uint32_t NL, TL, NS, TS;
  uint32_t to_obj;        /* 0: object -> rows, 1: rows -> object */
  uint32_t obj_vec;       /* 1: the object side may use 16-byte accesses (obj is 16-byte aligned) */
  uint32_t mask[8];       /* rows -> object: a bit per block to write */
};

TX_HD uint32_t obj_K(const struct obj_lay *l, uint32_t b) { return b < l->ZL ? l->KL : l->KS; }

TX_HD uint64_t obj_boff(const struct obj_lay *l, uint32_t b) {
  return b < l->ZL ? (uint64_t)b * l->KL * l->T : ((uint64_t)l->ZL * l->KL + (uint64_t)(b - l->ZL) * l->KS) * l->T;
}

/* the piece width V: the widest of 16, 8, 4, 2, 1 that divides T, TL, TS and the rows' address */
TX_HD uint32_t obj_width(const struct obj_lay *l) {
  const uint64_t a = (uint64_t)(uintptr_t)l->rows | l->T | l->TL | l->TS;
  uint32_t V = 16u;
  while (a & (V - 1u)) V >>= 1;
  return V;
}

/* windows of 16 bytes that overlap block b */
TX_HD uint32_t obj_windows(const struct obj_lay *l, uint32_t b) {
  const uint64_t o0 = obj_boff(l, b), o1 = o0 + (uint64_t)obj_K(l, b) * l->T;
  return (uint32_t)((o1 + OBJ_WIN - 1u) / OBJ_WIN - o0 / OBJ_WIN);
}

/* row-image offset of in-block object offset r (block of K symbols); *rem = bytes left in that sub-block row */
TX_HD uint32_t obj_locate(const struct obj_lay *l, uint32_t K, uint32_t r, uint32_t *rem) {
  const uint32_t sL = K * l->TL, aL = l->NL * sL;
  uint32_t j, s, col, Tj;
  if (r < aL) {
    j = r / sL; s = r - j * sL; col = j * l->TL; Tj = l->TL;
  } else {
    const uint32_t sS = K * l->TS, r2 = r - aL;
    j = r2 / sS; s = r2 - j * sS; col = l->NL * l->TL + j * l->TS; Tj = l->TS;
  }
  const uint32_t e = s / Tj, c = s - e * Tj;
  *rem = Tj - c;
  return e * l->T + col + c;
}

/* 16 bytes as V-byte pieces */
template <typename W>
struct alignas(16) obj_chunk {
  W w[OBJ_WIN / sizeof(W)];
};

/* The row-side offsets (from the block's row image) of the pieces of window q of block b, and which pieces belong to the block.
 * Returns the window's object offset; *full = 1 when the whole window lies inside the block and before F. */
template <typename W>
TX_HD uint64_t obj_window_map(const struct obj_lay *l, uint32_t b, uint32_t q, uint32_t *roff, uint32_t *own, uint32_t *full) {
  constexpr uint32_t V = sizeof(W), P = OBJ_WIN / V;
  const uint32_t K = obj_K(l, b);
  const uint64_t o0 = obj_boff(l, b), o1 = o0 + (uint64_t)K * l->T;
  const uint64_t ws = (o0 / OBJ_WIN + q) * OBJ_WIN;
  *own = 0;
  *full = ws >= o0 && ws + OBJ_WIN <= o1 && ws + OBJ_WIN <= l->F;
  uint32_t rem = 0, ro = 0;
#pragma unroll
  for (uint32_t p = 0; p < P; p++) {
    const uint64_t o = ws + (uint64_t)p * V;
    roff[p] = 0;
    if (o < o0 || o >= o1) continue;
    if (rem >= 2u * V) { ro += V; rem -= V; }
    else ro = obj_locate(l, K, (uint32_t)(o - o0), &rem);
    roff[p] = ro;
    *own |= 1u << p;
  }
  return ws;
}

/* object bytes [ws, ws + 16) as 16 / V pieces (zero at offsets >= F; the object side 16 bytes wide when it may be) */
template <typename W>
TX_HD obj_chunk<W> obj_load_window(const struct obj_lay *l, uint64_t ws, uint32_t full) {
  obj_chunk<W> v;
  if (full && l->obj_vec) return *reinterpret_cast<const obj_chunk<W> *>(l->obj + ws);
  uint8_t *bytes = reinterpret_cast<uint8_t *>(v.w);
#pragma unroll
  for (uint32_t i = 0; i < OBJ_WIN; i++) bytes[i] = ws + i < l->F ? l->obj[ws + i] : (uint8_t)0;
  return v;
}

/* pieces `own` of v to the object (bytes at offsets >= F skipped) */
template <typename W>
TX_HD void obj_store_window(const struct obj_lay *l, uint64_t ws, uint32_t full, uint32_t own, const obj_chunk<W> &v) {
  constexpr uint32_t V = sizeof(W);
  if (full && l->obj_vec) {
    *reinterpret_cast<obj_chunk<W> *>(l->obj + ws) = v;
    return;
  }
  const uint8_t *bytes = reinterpret_cast<const uint8_t *>(v.w);
#pragma unroll
  for (uint32_t i = 0; i < OBJ_WIN; i++)
    if (((own >> (i / V)) & 1u) && ws + i < l->F) l->obj[ws + i] = bytes[i];
}

/* windows q0, q0 + stride, ... (OBJ_UNROLL of them) of block b: every load before any store */
template <typename W>
TX_HD void obj_move(const struct obj_lay *l, uint32_t b, uint32_t q0, uint32_t stride) {
  constexpr uint32_t P = OBJ_WIN / sizeof(W);
  const uint32_t nw = obj_windows(l, b);
  uint8_t *R = l->rows + obj_boff(l, b);
  obj_chunk<W> v[OBJ_UNROLL];
  uint32_t roff[OBJ_UNROLL][P], own[OBJ_UNROLL], full[OBJ_UNROLL];
  uint64_t ws[OBJ_UNROLL];
#pragma unroll
  for (uint32_t u = 0; u < OBJ_UNROLL; u++) {
    const uint32_t q = q0 + u * stride;
    own[u] = 0;
    if (q >= nw) continue;
    ws[u] = obj_window_map<W>(l, b, q, roff[u], &own[u], &full[u]);
    if (!l->to_obj) {
      v[u] = obj_load_window<W>(l, ws[u], full[u]);
    } else {
      for (uint32_t p = 0; p < P; p++) v[u].w[p] = ((own[u] >> p) & 1u) ? *reinterpret_cast<const W *>(R + roff[u][p]) : W();
    }
  }
#pragma unroll
  for (uint32_t u = 0; u < OBJ_UNROLL; u++) {
    if (!own[u]) continue;
    if (!l->to_obj) {
      for (uint32_t p = 0; p < P; p++)
        if ((own[u] >> p) & 1u) *reinterpret_cast<W *>(R + roff[u][p]) = v[u].w[p];
    } else {
      obj_store_window<W>(l, ws[u], full[u], own[u], v[u]);
    }
  }
}

#endif /* NRQ_OBJ_BODY_H */
