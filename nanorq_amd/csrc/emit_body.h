/*
 * emit_body.h -- the per-packet bodies of the device-resident emit (nrq_tx_* and nrq_otx_*, include/nanorq_hip.h): packets -- an
 * optional 4-byte RFC 6330 FEC Payload ID and a payload at a packet stride -- written straight into device memory from the
 * intermediate symbols of blocks that are already in device memory.
 *
 * The source of an emit is a table (tx_src) of up to TX_SEGS segments: consecutive SBN ranges of equal (K, K', T) and uniform
 * row strides (tx_blk), which together cover the span of Z blocks from SBN sbn0, the first ZL of them of the larger class.  A
 * transmission (nrq_tx) is one segment with Z = ZL = nblk; an object (nrq_otx) has class L, class S and a last block staged
 * apart (N = 1, F < Kt * T).
 *
 * Payload of (block b, ESI e), bit-exact with nanorq_encode (nanorq_api.c):
 *   e <  K   source row e of block b (the caller's rows)
 *   e >= K   LT(C_b, e + K' - K): the XOR of the intermediate symbols rq_lt_columns names
 * nrq_device.hip instantiates these bodies in its emit kernels; emit_emu.cpp runs them sequentially on the CPU.
 *
 * Work order.  A packet's repair gathers hit its block's L x T bytes of intermediate symbols; the kernel walks packets BLOCK-MAJOR
 * (work item w -> packet tx_packet_of(w)) so that a block's packets run together and its rows are served from the caches, in
 * whatever order the packets lie in the output.  Range mode maps analytically; a tag list is first bucketed by block (tx_bin:
 * one bucket per block of the span, one more for SBNs outside it) into c->order.
 *
 * Ready mask.  A relay (a sender over a reception's rows) may hold blocks whose intermediate symbols are not written yet:
 * tx_src::ready has a bit per block of the span, and a packet of a block whose bit is clear is left untouched with the result
 * TX_NOT_READY (tx_admit).  Senders pass all ones.
 *
 * Held symbols.  With NRQ_TX_HELD a relay's tag-list emit carries a second table (tx_held: per segment the books and repair rows of
 * the reception the segment reads) and admits packets through tx_admit_held: a block that is not ready still gives the symbols
 * the reception holds, as copies of their rows.  nrq_emit_held_kernel is the kernel of that form; held_emu.cpp emulates it.
 */
#ifndef NRQ_EMIT_BODY_H
#define NRQ_EMIT_BODY_H

#include <stdint.h>

#include "rq_math.h"

#if defined(__HIPCC__)
#define TX_HD __host__ __device__ __forceinline__
#else
#define TX_HD static inline
#endif

#define TX_NONE 0xFFFFFFFFu
#define TX_COLS 33u   /* room per packet for a column list: rq_lt_columns gives at most RQ_LT_COLS_MAX_REAL (odd: a lane's list
                       * in LDS starts on its own bank) */
#define TX_WAVE_PKTS 64u /* work items one wave takes: one per lane for the column lists, then one after the other for the payload */

#define TX_SEGS 3u /* segments of an emit source: block class L, class S, and a last block staged apart */

#define TX_FOREIGN (-1)   /* list mode result: SBN outside the span */
#define TX_NOT_READY (-2) /* list mode result: a block of the span that is not ready (relays only) */

/* one segment: nblk blocks of equal (K, K', T), SBNs sbn0 .. sbn0+nblk-1 (device addresses; the emulation passes host arrays) */
struct tx_blk {
  rq_params p;            /* of K' (p.K = K) */
  uint32_t K, T, nblk, sbn0;
  const uint8_t *src;     /* block b's source row e at src + b*src_stride + e*T */
  uint64_t src_stride;
  const uint8_t *inter;   /* block b's intermediate symbol i at inter + b*inter_stride + i*T */
  uint64_t inter_stride;
};

/* the emit source: segments seg[0 .. nseg) over the span of Z blocks from SBN sbn0, the first ZL of them of the larger class */
struct tx_src {
  struct tx_blk seg[TX_SEGS];
  uint32_t nseg;
  uint32_t sbn0, Z, ZL;
  uint32_t ready[8];      /* a bit per block of the span (Z <= 256): its packets may be emitted.  All ones for a sender; a relay
                           * (nrq_rx_relay) clears the blocks whose intermediate symbols are not there yet */
};

/* one emit call */
struct tx_call {
  uint8_t *pkts;          /* packet k at pkts + k*pkt_stride */
  uint64_t pkt_stride;
  uint32_t n;             /* packets (work items) */
  uint32_t inl;           /* 1: FEC Payload ID at +0, payload at +4 */
  const uint32_t *tags;   /* list mode: tag of packet k (nanorq_tag form); NULL: range mode */
  const uint32_t *order;  /* list mode: packet of work item w (bucketed by block) */
  int32_t *results;       /* list mode, nullable: 0 written, TX_FOREIGN SBN outside the span, TX_NOT_READY */
  uint32_t esi0, nL, nS;  /* range mode: ESIs esi0 .. esi0+nL-1 of each of the first ZL blocks, esi0 .. esi0+nS-1 of the rest */
  uint32_t interleave;    /* range mode: 0 block-major, 1 sorted by (ESI, SBN) */
  uint32_t *tags_out;     /* range mode, nullable: the tag of each packet */
};

TX_HD uint32_t tx_tag(uint32_t sbn, uint32_t esi) { return (sbn << 24) | esi; }

/* block of a tag inside SBNs sbn0 .. sbn0+nblk-1, or TX_NONE */
TX_HD uint32_t tx_index(uint32_t sbn0, uint32_t nblk, uint32_t tag) {
  const uint32_t sbn = tag >> 24;
  return (sbn >= sbn0 && sbn - sbn0 < nblk) ? sbn - sbn0 : TX_NONE;
}
TX_HD uint32_t tx_block(const struct tx_blk *t, uint32_t tag) { return tx_index(t->sbn0, t->nblk, tag); }

/* list mode bucket: the block in the span, or nblk for an SBN outside it */
TX_HD uint32_t tx_bin(uint32_t sbn0, uint32_t nblk, uint32_t tag) {
  const uint32_t b = tx_index(sbn0, nblk, tag);
  return b == TX_NONE ? nblk : b;
}

/* the segment holding the SBN of `tag`, or TX_SEGS (outside the span); MULTI = false: a one-segment table */
template <bool MULTI>
TX_HD uint32_t tx_seg(const struct tx_src *s, uint32_t tag) {
  const uint32_t nseg = MULTI ? s->nseg : 1u;
  for (uint32_t g = 0; g < nseg; g++)
    if (tx_block(&s->seg[g], tag) != TX_NONE) return g;
  return TX_SEGS;
}

/* the ready bit of the block of `tag` (a tag of the span); the mask word is picked by value (no dynamic index into the kernel
 * arguments) */
TX_HD uint32_t tx_ready(const struct tx_src *s, uint32_t tag) {
  const uint32_t b = (tag >> 24) - s->sbn0;
  uint32_t w = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (uint32_t i = 0; i < 8u; i++) w = i == (b >> 5) ? s->ready[i] : w;
  return (w >> (b & 31u)) & 1u;
}

/* what a packet of `tag` gets: its segment, or TX_SEGS when it stays untouched -- *code says why (0: it is written) */
template <bool MULTI>
TX_HD uint32_t tx_admit(const struct tx_src *s, uint32_t tag, int32_t *code) {
  const uint32_t g = tx_seg<MULTI>(s, tag);
  if (g == TX_SEGS) { *code = TX_FOREIGN; return TX_SEGS; }
  if (!tx_ready(s, tag)) { *code = TX_NOT_READY; return TX_SEGS; }
  *code = 0;
  return g;
}

/* segment g, selected by value (no dynamic index into the kernel arguments) */
TX_HD struct tx_blk tx_pick(const struct tx_src *s, uint32_t g) {
  struct tx_blk t = s->seg[0];
  if (g == 1u) t = s->seg[1];
  else if (g == 2u) t = s->seg[2];
  return t;
}

/* Held symbols (NRQ_TX_HELD, relays only).  Beside the source table lies, per segment, the index of the reception whose rows the
 * segment reads (ing_rx's books): a packet of a block that is NOT ready is then still written when the reception holds that very
 * symbol -- a copy of source row ESI (its seen bit is set), or of the repair row q with rep_esi[b][q] == ESI, q < nrep[b] (a
 * repair symbol's seen bit is set when it took a row, and only then: FULL ones are not marked).  Ready blocks go the usual way. */
struct tx_held_seg {
  const uint32_t *seen;    /* [nblk][bm_words] */
  const uint32_t *rep_esi; /* [nblk][rep_cap]: ESI of repair row q, arrival order */
  const uint32_t *nrep;    /* [nblk]: repair rows used */
  const uint8_t *rep;      /* block b's repair row q at rep + b*rep_stride + q*T */
  uint64_t rep_stride;
  uint32_t bm_words, rep_cap;
};
struct tx_held {
  struct tx_held_seg seg[TX_SEGS];
};

#define TX_READY 0u    /* kinds of an admitted packet: built from the block's rows as ever */
#define TX_HELD_SRC 1u /* a copy of the held source row ESI */
#define TX_HELD_REP 2u /* a copy of the held repair row tx_held_find gives */

/* the seen bit of ESI `esi` of block b (an ESI beyond the bitmap, i.e. above max_esi, is not seen: nothing is read) */
TX_HD uint32_t tx_held_seen(const struct tx_held_seg *h, uint32_t b, uint32_t esi) {
  if ((esi >> 5) >= h->bm_words) return 0u;
  return (h->seen[(uint64_t)b * h->bm_words + (esi >> 5)] >> (esi & 31u)) & 1u;
}

/* held segment g, selected by value (as tx_pick) */
TX_HD struct tx_held_seg tx_held_pick(const struct tx_held *h, uint32_t g) {
  struct tx_held_seg t = h->seg[0];
  if (g == 1u) t = h->seg[1];
  else if (g == 2u) t = h->seg[2];
  return t;
}

/* tx_admit with held symbols: the segment and *kind (TX_READY / TX_HELD_SRC / TX_HELD_REP), or TX_SEGS when the packet stays
 * untouched.  (A TX_HELD_REP packet's row is still to be found: tx_held_find.) */
template <bool MULTI>
TX_HD uint32_t tx_admit_held(const struct tx_src *s, const struct tx_held *h, uint32_t tag, int32_t *code, uint32_t *kind) {
  const uint32_t g = tx_seg<MULTI>(s, tag);
  *kind = TX_READY;
  if (g == TX_SEGS) { *code = TX_FOREIGN; return TX_SEGS; }
  *code = 0;
  if (tx_ready(s, tag)) return g;
  const struct tx_blk t = tx_pick(s, MULTI ? g : 0u);
  const struct tx_held_seg hs = tx_held_pick(h, MULTI ? g : 0u);
  const uint32_t esi = tag & 0xFFFFFFu;
  if (!tx_held_seen(&hs, tx_block(&t, tag), esi)) { *code = TX_NOT_READY; return TX_SEGS; }
  *kind = esi < t.K ? TX_HELD_SRC : TX_HELD_REP;
  return g;
}

/* one probe of the ESI -> repair row lookup: is repair row q of block b the one of `esi`?  (The kernel probes 64 rows per trip, a
 * lane each, and takes a ballot; tx_held_find is the same walk one row at a time.) */
TX_HD bool tx_held_hit(const struct tx_held_seg *h, uint32_t b, uint32_t q, uint32_t nrep, uint32_t esi) {
  return q < nrep && h->rep_esi[(uint64_t)b * h->rep_cap + q] == esi;
}
TX_HD uint32_t tx_held_nrep(const struct tx_held_seg *h, uint32_t b) {
  const uint32_t n = h->nrep[b];
  return n < h->rep_cap ? n : h->rep_cap;
}
TX_HD uint32_t tx_held_find(const struct tx_held_seg *h, uint32_t b, uint32_t esi) {
  const uint32_t nrep = tx_held_nrep(h, b);
  for (uint32_t q = 0; q < nrep; q++)
    if (tx_held_hit(h, b, q, nrep, esi)) return q;
  return TX_NONE;
}

/* the rows of a TX_HELD_REP packet: the block's repair rows */
TX_HD const uint8_t *tx_held_rep_base(const struct tx_held_seg *h, uint32_t b) { return h->rep + (uint64_t)b * h->rep_stride; }

/* Range mode.  Block-major: block b's packets (nL or nS of them) one after the other.  Interleaved: round i holds ESI esi0 + i of
 * every block while i < nlo, later rounds only the first ZL blocks' (nL >= nS).  MULTI = false: a one-segment table, i.e. one
 * block class, where every block has nL packets (the launcher passes nL = nS) and the maps reduce to (w / nL, w % nL) and
 * (k % Z, k / Z). */
TX_HD uint32_t tx_nlo(const struct tx_src *s, const struct tx_call *c) { return s->Z - s->ZL ? c->nS : c->nL; }

/* block-major position w -> (block, i) */
template <bool MULTI>
TX_HD void tx_bm(const struct tx_src *s, const struct tx_call *c, uint32_t w, uint32_t *b, uint32_t *i) {
  const uint32_t aL = s->ZL * c->nL;
  if (!MULTI || w < aL) { *b = w / c->nL; *i = w - *b * c->nL; }
  else { const uint32_t w2 = w - aL, q = w2 / c->nS; *b = s->ZL + q; *i = w2 - q * c->nS; }
}

/* interleaved packet index of (block, i), and back */
template <bool MULTI>
TX_HD uint32_t tx_il_index(const struct tx_src *s, const struct tx_call *c, uint32_t b, uint32_t i) {
  const uint32_t nlo = tx_nlo(s, c);
  return !MULTI || i < nlo ? i * s->Z + b : nlo * s->Z + (i - nlo) * s->ZL + b;
}
template <bool MULTI>
TX_HD void tx_il_pair(const struct tx_src *s, const struct tx_call *c, uint32_t k, uint32_t *b, uint32_t *i) {
  const uint32_t nlo = tx_nlo(s, c), a = nlo * s->Z;
  if (!MULTI || k < a) { *i = k / s->Z; *b = k - *i * s->Z; }
  else { const uint32_t k2 = k - a, r = k2 / s->ZL; *i = nlo + r; *b = k2 - r * s->ZL; }
}

/* packet index of work item w (work in block-major order) */
template <bool MULTI>
TX_HD uint32_t tx_packet_of(const struct tx_src *s, const struct tx_call *c, uint32_t w) {
  if (c->tags) return c->order[w];
  if (!c->interleave) return w;
  uint32_t b, i;
  tx_bm<MULTI>(s, c, w, &b, &i);
  return tx_il_index<MULTI>(s, c, b, i);
}

/* tag of packet k */
template <bool MULTI>
TX_HD uint32_t tx_tag_of(const struct tx_src *s, const struct tx_call *c, uint32_t k) {
  if (c->tags) return c->tags[k];
  uint32_t b, i;
  if (c->interleave) tx_il_pair<MULTI>(s, c, k, &b, &i);
  else tx_bm<MULTI>(s, c, k, &b, &i);
  return tx_tag(s->sbn0 + b, c->esi0 + i);
}

/* the rows a packet of `tag` (inside the segment) is made of: the block's source rows or its intermediate symbols */
TX_HD const uint8_t *tx_base(const struct tx_blk *t, uint32_t tag) {
  const uint32_t b = tx_block(t, tag);
  return (tag & 0xFFFFFFu) < t->K ? t->src + (uint64_t)b * t->src_stride : t->inter + (uint64_t)b * t->inter_stride;
}

/* The rows whose XOR is the payload of `tag`, as indices (times T) from tx_base into cols[TX_COLS]; returns their count, 0 for
 * an SBN outside the segment. */
TX_HD uint32_t tx_rows(const struct tx_blk *t, uint32_t tag, uint32_t *cols) {
  const uint32_t esi = tag & 0xFFFFFFu;
  if (tx_block(t, tag) == TX_NONE) return 0;
  if (esi < t->K) {
    cols[0] = esi;
    return 1;
  }
  return rq_lt_columns(&t->p, esi + (t->p.Kp - t->K), cols);
}

/* the FEC Payload ID as it lies in memory (network byte order), read as a little-endian word */
TX_HD uint32_t tx_header_word(uint32_t tag) {
  return (tag >> 24) | ((tag >> 8) & 0xFF00u) | ((tag << 8) & 0xFF0000u) | (tag << 24);
}

/* XOR of the W-wide words at byte `off` of rows cols[0..n) (four loads in flight before they are combined) */
template <typename W>
TX_HD W tx_gather(const uint8_t *base, uint64_t T, const uint32_t *cols, uint32_t n, uint64_t off) {
  W acc = W();
  uint32_t i = 0;
  for (; i + 4u <= n; i += 4u) {
    const W a = *reinterpret_cast<const W *>(base + (uint64_t)cols[i] * T + off);
    const W b = *reinterpret_cast<const W *>(base + (uint64_t)cols[i + 1u] * T + off);
    const W c = *reinterpret_cast<const W *>(base + (uint64_t)cols[i + 2u] * T + off);
    const W d = *reinterpret_cast<const W *>(base + (uint64_t)cols[i + 3u] * T + off);
    acc = acc ^ a ^ b ^ c ^ d;
  }
  for (; i < n; i++) acc = acc ^ *reinterpret_cast<const W *>(base + (uint64_t)cols[i] * T + off);
  return acc;
}

/* 16 bytes as a value type both compilers treat alike */
struct alignas(16) tx_u128 {
  uint32_t x, y, z, w;
};
TX_HD tx_u128 operator^(tx_u128 a, tx_u128 b) { return tx_u128{a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w}; }

/* payload paths of the emit kernels, chosen per call from the alignment of the rows, the packets and T */
enum : int {
  TX_V16 = 0,       /* 16-byte loads and stores (payload at +0) */
  TX_V16_SHIFT = 1, /* 16-byte loads and stores under an inline header: the payload moves up one dword across the lanes */
  TX_DWORD = 2,     /* 4-byte loads and stores */
  TX_BYTE = 3
};

/* what decides the path: the OR of the packet buffer's address and stride, T and every row table's address and stride (h: the
 * held table of an NRQ_TX_HELD call, whose repair rows are copied too; else NULL) */
TX_HD uint64_t tx_align(const struct tx_src *s, const struct tx_call *c, const struct tx_held *h) {
  uint64_t al = (uint64_t)(uintptr_t)c->pkts | c->pkt_stride | s->seg[0].T;
  for (uint32_t g = 0; g < s->nseg; g++) {
    const struct tx_blk *t = &s->seg[g];
    al |= (uint64_t)(uintptr_t)t->src | t->src_stride | (uint64_t)(uintptr_t)t->inter | t->inter_stride;
    if (h) al |= (uint64_t)(uintptr_t)h->seg[g].rep | h->seg[g].rep_stride;
  }
  return al;
}

/* the path: the widest word every address of the call allows (force_dword: the tuning knob that keeps a call off the 16-byte paths) */
TX_HD int tx_emit_path(uint64_t al, uint32_t inl, uint32_t force_dword) {
  if ((al & 15u) == 0 && !force_dword) return inl ? TX_V16_SHIFT : TX_V16;
  return (al & 3u) == 0 ? TX_DWORD : TX_BYTE;
}

/* one whole packet, a byte at a time (the emulation; the kernels' byte path does the same with a lane per byte) */
TX_HD void tx_emit_bytes(const struct tx_blk *t, const struct tx_call *c, uint32_t k, uint32_t tag, const uint32_t *cols, uint32_t n) {
  const uint8_t *base = tx_base(t, tag);
  uint8_t *P = c->pkts + (uint64_t)k * c->pkt_stride;
  if (c->inl) {
    const uint32_t h = tx_header_word(tag);
    for (uint32_t j = 0; j < 4u; j++) P[j] = (uint8_t)(h >> (8u * j));
    P += 4;
  }
  for (uint32_t j = 0; j < t->T; j++) P[j] = tx_gather<uint8_t>(base, t->T, cols, n, j);
}

#endif /* NRQ_EMIT_BODY_H */
