/*
 * held_body.h -- the bodies of the listing of what a reception holds (nrq_rx_held / nrq_orx_held, include/nanorq_hip.h): the tags
 * (nanorq_tag() form) of every symbol whose bytes lie in the reception's rows, block-major, within a block the seen source ESIs
 * ascending, then the repair ESIs in arrival order.  It is the list a held emit (NRQ_TX_HELD, emit_body.h) answers in full.
 *
 * nrq_device.hip runs them in three short kernels on the reception's stream -- count (per block: a popcount over the seen words
 * below K, plus the repair rows used), an exclusive scan over the blocks, compaction (per block: a scan over its words' counts
 * places each word's tags) -- and held_emu.cpp sequentially on the CPU.  They only read the reception's books (ingest_body.h).
 */
#ifndef NRQ_HELD_BODY_H
#define NRQ_HELD_BODY_H

#include <stdint.h>

#include "ingest_body.h"

/* 32-bit words of a block's seen bitmap that cover its source ESIs */
ING_HD uint32_t hl_words(const struct ing_rx *r) { return (r->K + 31u) / 32u; }

/* the seen source ESIs of word w of block b (bits at or above K masked off) */
ING_HD uint32_t hl_have(const struct ing_rx *r, uint32_t b, uint32_t w) {
  const uint32_t nb = r->K - w * 32u < 32u ? r->K - w * 32u : 32u;
  return r->seen[(uint64_t)b * r->bm_words + w] & (nb == 32u ? 0xFFFFFFFFu : ((1u << nb) - 1u));
}

ING_HD uint32_t hl_popc(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__popc(v);
#else
  return (uint32_t)__builtin_popcount(v);
#endif
}

/* repair rows of block b in use */
ING_HD uint32_t hl_nrep(const struct ing_rx *r, uint32_t b) { return r->nrep[b] < r->rep_cap ? r->nrep[b] : r->rep_cap; }

/* the tags of word w's seen source ESIs (`have` = hl_have), ascending, to out[0 ..]; returns their count */
ING_HD uint32_t hl_put(const struct ing_rx *r, uint32_t b, uint32_t w, uint32_t have, uint32_t *out) {
  uint32_t n = 0;
  while (have) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t i = (uint32_t)__ffs(have) - 1u;
#else
    const uint32_t i = (uint32_t)__builtin_ctz(have);
#endif
    out[n++] = ((r->sbn0 + b) << 24) | (w * 32u + i);
    have &= have - 1u;
  }
  return n;
}

/* the tag of repair row q of block b */
ING_HD uint32_t hl_rep_tag(const struct ing_rx *r, uint32_t b, uint32_t q) {
  return ((r->sbn0 + b) << 24) | r->rep_esi[(uint64_t)b * r->rep_cap + q];
}

#endif /* NRQ_HELD_BODY_H */
