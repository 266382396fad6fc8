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

/* the seen source ESIs of word w (below ing_src_words) of block b */
ING_HD uint32_t hl_have(const struct ing_rx *r, uint32_t b, uint32_t w) {
  return r->seen[(uint64_t)b * r->bm_words + w] & ing_src_mask(r, w);
}

/* repair rows of block b in use */
ING_HD uint32_t hl_nrep(const struct ing_rx *r, uint32_t b) { return r->nrep[b] < r->rep_cap ? r->nrep[b] : r->rep_cap; }

/* the tags of word w's seen source ESIs (`have` = hl_have), ascending, to out[0 ..]; returns their count */
ING_HD uint32_t hl_put(const struct ing_rx *r, uint32_t b, uint32_t w, uint32_t have, uint32_t *out) {
  uint32_t n = 0;
  while (have) {
    out[n++] = ((r->sbn0 + b) << 24) | (w * 32u + ing_lowbit(have));
    have &= have - 1u;
  }
  return n;
}

/* the tag of repair row q of block b */
ING_HD uint32_t hl_rep_tag(const struct ing_rx *r, uint32_t b, uint32_t q) {
  return ((r->sbn0 + b) << 24) | r->rep_esi[(uint64_t)b * r->rep_cap + q];
}

#endif /* NRQ_HELD_BODY_H */
