/*
 * ingest_body.h -- the per-thread bodies of the device-resident receiver (nrq_rx_*, include/nanorq_hip.h): packets already in
 * device memory are classified with the rules of nanorq_decoder_add_symbol (nanorq_api.c), placed into their rows and booked
 * into a device-resident reception -- a batch of nblk blocks of equal (K, K', T), SBNs sbn0 .. sbn0+nblk-1.
 *
 * nrq_device.hip instantiates them in a chain of short kernels on one stream (no cross-workgroup handshake); tests/emu/ingest_emu.cpp
 * runs the same functions sequentially on the CPU.  One call over packets 0 .. n-1:
 *   1. first   (per packet)  decode the tag, first arrival of every (block, ESI) of this call: atomicMin of the packet index
 *   2. done    (per block)   the packet index at which the block's source set becomes complete: a max over its missing source ESIs
 *   3. hist    (per tile)    repair packets that may be added (first arrival, not seen, block not complete yet), per block
 *   4. scan    (per block)   exclusive scan of (3) over the tiles: the row of the tile's first such packet
 *   5. classify (per tile)   result code; the row of an added repair packet = (4) + its rank in the tile, in packet order
 *   6. copy    (per packet)  the payload of an added packet to its row
 *   7. fold    (per packet)  duplicates of a repair packet that found the rows full are full too; seen bits; reset of (1)
 * Every decision depends on packet order only, never on the order waves run in: the repair list is the arrival order.
 */
#ifndef NRQ_INGEST_BODY_H
#define NRQ_INGEST_BODY_H

#include <stdint.h>

#if defined(__HIPCC__)
#define ING_HD __host__ __device__ __forceinline__
#define ING_ATOMIC_MIN(p, v) atomicMin((p), (v))
#define ING_ATOMIC_OR(p, v) atomicOr((p), (v))
#else
#define ING_HD static inline
#define ING_ATOMIC_MIN(p, v) (*(p) = *(p) < (v) ? *(p) : (v))
#define ING_ATOMIC_OR(p, v) (*(p) |= (v))
#endif

/* result codes (NANORQ_SYM_* of include/nanorq.h, plus one) */
#define ING_ERR (-1)
#define ING_ADDED 0
#define ING_IGN 1
#define ING_DUP 2
#define ING_FULL 3 /* NRQ_RX_FULL: a repair symbol that found the block's rep_cap repair rows used; not marked as seen */

#define ING_TILE 256u     /* packets per tile (passes 3 and 5: one workgroup) */
#define ING_NONE 0xFFFFFFFFu

/* the reception's device state (all arrays in device memory; the emulation passes host arrays) */
struct ing_rx {
  uint32_t K, T, nblk, sbn0, max_esi, rep_cap;
  uint32_t m1;        /* max_esi + 1: entries of a block's first-arrival table */
  uint32_t bm_words;  /* 32-bit words of a block's seen bitmap (max_esi / 32 + 1) */
  uint8_t *src;       /* block b's source row e at src + b*src_stride + e*T */
  uint64_t src_stride;
  uint8_t *rep;       /* block b's repair row q at rep + b*rep_stride + q*T */
  uint64_t rep_stride;
  uint32_t *first;    /* [nblk][m1]: packet index of the first arrival in the running call, ING_NONE between calls */
  uint32_t *seen;     /* [nblk][bm_words]: ESIs booked by earlier calls (and the source rows a decode recovered) */
  uint32_t *gaps;     /* [nblk]: source ESIs not seen */
  uint32_t *nrep;     /* [nblk]: repair rows used */
  uint32_t *rep_esi;  /* [nblk][rep_cap]: ESI of repair row q, in arrival order */
  uint32_t *live;     /* [nblk]: packets of the running call with index >= live[b] find the block complete (IGN) */
};

/* one call's packets and per-packet scratch */
struct ing_call {
  const uint8_t *pkts; /* packet k at pkts + k*pkt_stride */
  uint64_t pkt_stride;
  const uint32_t *tags; /* nanorq_tag() form, or NULL: each packet starts with the RFC 6330 section 3.2 FEC Payload ID */
  uint32_t n, ntiles;
  uint32_t *tagv;    /* [n] the decoded tags */
  int32_t *codes;    /* [n] result codes (the caller's array or scratch) */
  uint32_t *fidx;    /* [n] first arrival of the packet's (block, ESI) (pass 5 -> 7) */
  uint64_t *dst;     /* [n] destination row of the payload, 0 = none (pass 5 -> 6) */
  uint32_t *base;    /* [nblk][ntiles] repair candidates per tile (pass 3), then the row of the tile's first one (pass 4) */
};

ING_HD uint32_t ing_payload_off(const struct ing_call *c) { return c->tags ? 0u : 4u; }

/* block of a tag inside the reception, or ING_NONE */
ING_HD uint32_t ing_block(const struct ing_rx *r, uint32_t tag) {
  const uint32_t sbn = tag >> 24;
  return (sbn >= r->sbn0 && sbn - r->sbn0 < r->nblk) ? sbn - r->sbn0 : ING_NONE;
}

ING_HD bool ing_seen(const struct ing_rx *r, uint32_t b, uint32_t esi) {
  return (r->seen[(uint64_t)b * r->bm_words + (esi >> 5)] >> (esi & 31u)) & 1u;
}

/* 32-bit words of a block's seen bitmap that cover its source ESIs */
ING_HD uint32_t ing_src_words(const struct ing_rx *r) { return (r->K + 31u) / 32u; }

/* the bits of word w (below ing_src_words) that are source ESIs: the last word is masked at K.  A decode that recovers a block
 * sets exactly these in every word (nanorq_repair_block); the listings read no others as source symbols. */
ING_HD uint32_t ing_src_mask(const struct ing_rx *r, uint32_t w) {
  const uint32_t nb = r->K - w * 32u < 32u ? r->K - w * 32u : 32u;
  return nb == 32u ? 0xFFFFFFFFu : ((1u << nb) - 1u);
}

/* set bits of v; the number of its lowest set bit (v != 0) */
ING_HD uint32_t ing_popc(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__popc(v);
#else
  return (uint32_t)__builtin_popcount(v);
#endif
}
ING_HD uint32_t ing_lowbit(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__ffs(v) - 1u;
#else
  return (uint32_t)__builtin_ctz(v);
#endif
}

/* pass 1 */
ING_HD void ing_first(const struct ing_rx *r, const struct ing_call *c, uint32_t k) {
  uint32_t tag;
  if (c->tags) {
    tag = c->tags[k];
  } else { /* SBN (8 bits) and ESI (24 bits), network byte order */
    const uint8_t *p = c->pkts + (uint64_t)k * c->pkt_stride;
    tag = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
  }
  c->tagv[k] = tag;
  const uint32_t b = ing_block(r, tag), esi = tag & 0xFFFFFFu;
  if (b != ING_NONE && esi <= r->max_esi) ING_ATOMIC_MIN(&r->first[(uint64_t)b * r->m1 + esi], k);
}

/* pass 2, the part of one source ESI: folds it into (mx, cnt) = (latest first arrival of a missing ESI, missing ESIs that arrived) */
ING_HD void ing_done_part(const struct ing_rx *r, uint32_t b, uint32_t e, uint32_t *mx, uint32_t *cnt) {
  if (ing_seen(r, b, e)) return;
  const uint32_t f = r->first[(uint64_t)b * r->m1 + e];
  if (f > *mx) *mx = f;
  if (f != ING_NONE) (*cnt)++;
}
/* pass 2, per block after the reduction.  A block with gaps at the start of the call is complete once every missing ESI has
 * arrived; the packet that completes it is added, the ones after it are IGN. */
ING_HD void ing_done_finish(const struct ing_rx *r, uint32_t b, uint32_t mx, uint32_t cnt) {
  if (r->gaps[b] == 0) {
    r->live[b] = 0;
  } else {
    r->live[b] = mx == ING_NONE ? ING_NONE : mx + 1u;
    r->gaps[b] -= cnt;
  }
}

/* a repair packet that is the first arrival of its ESI in this call, not seen before, before its block completes: it takes the
 * next repair row if there is one (passes 3 and 5).  Returns its block or ING_NONE. */
ING_HD uint32_t ing_cand(const struct ing_rx *r, const struct ing_call *c, uint32_t k) {
  const uint32_t tag = c->tagv[k], b = ing_block(r, tag), esi = tag & 0xFFFFFFu;
  if (b == ING_NONE || esi > r->max_esi || esi < r->K || k >= r->live[b] || ing_seen(r, b, esi)) return ING_NONE;
  return r->first[(uint64_t)b * r->m1 + esi] == k ? b : ING_NONE;
}

/* pass 5: the result of packet k.  `row` = the repair row it would take if it is a candidate (ing_cand). */
ING_HD void ing_classify(const struct ing_rx *r, const struct ing_call *c, uint32_t k, uint32_t row) {
  const uint32_t tag = c->tagv[k], b = ing_block(r, tag), esi = tag & 0xFFFFFFu;
  if (b == ING_NONE) { /* another reception's packet: its result untouched, nothing copied */
    c->dst[k] = 0;
    return;
  }
  int32_t code;
  uint64_t dst = 0;
  uint32_t f = k;
  if (esi > r->max_esi) {
    code = ING_ERR;
  } else if (k >= r->live[b]) {
    code = ING_IGN;
  } else if (ing_seen(r, b, esi)) {
    code = ING_DUP;
  } else if ((f = r->first[(uint64_t)b * r->m1 + esi]) != k) {
    code = ING_DUP; /* an earlier packet of this call carried the ESI; pass 7 makes it FULL if that one found the rows full */
  } else if (esi < r->K) {
    code = ING_ADDED;
    dst = (uint64_t)(uintptr_t)(r->src + b * r->src_stride + (uint64_t)esi * r->T);
  } else if (row < r->rep_cap) {
    code = ING_ADDED;
    dst = (uint64_t)(uintptr_t)(r->rep + b * r->rep_stride + (uint64_t)row * r->T);
    r->rep_esi[(uint64_t)b * r->rep_cap + row] = esi;
  } else {
    code = ING_FULL;
  }
  c->codes[k] = code;
  c->fidx[k] = f;
  c->dst[k] = dst;
}

/* pass 7 */
ING_HD void ing_fold(const struct ing_rx *r, const struct ing_call *c, uint32_t k) {
  const uint32_t tag = c->tagv[k], b = ing_block(r, tag), esi = tag & 0xFFFFFFu;
  if (b == ING_NONE || esi > r->max_esi) return;
  const int32_t code = c->codes[k];
  if (code == ING_DUP && c->fidx[k] != k && c->codes[c->fidx[k]] == ING_FULL) c->codes[k] = ING_FULL;
  if (code == ING_ADDED) ING_ATOMIC_OR(&r->seen[(uint64_t)b * r->bm_words + (esi >> 5)], 1u << (esi & 31u));
  r->first[(uint64_t)b * r->m1 + esi] = ING_NONE;
}

#endif /* NRQ_INGEST_BODY_H */
