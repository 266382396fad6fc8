/*
 * lists_set_body.h -- the bodies of a reception set's listing passes (nrq_rxset_counts / _lists / _decode, include/nanorq_hip.h):
 * what nrq_rx_counts and nrq_rx_lists give for one reception, for every block of every member in one pass over the member table
 * (struct ings_tab, ingest_set_body.h).  Blocks are in the table's order: global block g = blk0[m] + b.
 *
 * The compact lists are made the way the held / want listings are: a count per block, exclusive offsets by ONE scan over the
 * counts, a fill per block.  (The single form, nrq_ing_lists_kernel, sums the counts of all earlier blocks in one lane of every
 * workgroup; at 1024 blocks read through the table that is 1024 dependent loads per workgroup.)  The list buffer of a set of nb
 * blocks:
 *   [0, nb)        gaps of block g
 *   [nb, 2nb]      offset of block g's list in words (nb + 1 entries: the last is the total); nrep = off[g+1] - off[g] - gaps[g]
 *   [2nb + 1, ...) block by block its repair ESIs in arrival order, then its missing source ESIs ascending
 *
 * nrq_device.hip runs the bodies in kernels; rxset_lists_emu.cpp runs them on the CPU in the kernels' rounds.  They only read
 * the members' books.
 */
#ifndef NRQ_LISTS_SET_BODY_H
#define NRQ_LISTS_SET_BODY_H

#include "ingest_set_body.h"

#define LSS_ROUND 256u /* seen words a fill workgroup places per round */

/* the member of global block g and the block's number in it */
ING_HD const struct ing_rx *lss_block(const struct ings_tab *t, uint32_t g, uint32_t *b) {
  const uint32_t m = ings_member_of_block(t->blk0, t->nmem, g);
  *b = g - t->blk0[m];
  return &t->r[m];
}

/* the counts pass: gaps and nrep of global block g */
ING_HD void lss_counts(const struct ings_tab *t, uint32_t g, uint32_t *gaps, uint32_t *nrep) {
  uint32_t b;
  const struct ing_rx *r = lss_block(t, g, &b);
  *gaps = r->gaps[b];
  *nrep = r->nrep[b];
}

/* the count pass of the lists: buf[g] = gaps, buf[nb + g] = words of block g's list (the scan turns them into offsets) */
ING_HD void lss_list_count(const struct ings_tab *t, uint32_t g, uint32_t *buf) {
  uint32_t ng, nr;
  lss_counts(t, g, &ng, &nr);
  buf[g] = ng;
  buf[t->nblk + g] = ng + nr;
  if (g == 0) buf[2u * t->nblk] = 0;
}

/* the missing source ESIs of word w of block b (w beyond the words of the source ESIs: none) */
ING_HD uint32_t lss_miss(const struct ing_rx *r, uint32_t b, uint32_t w) {
  if (w >= ing_src_words(r)) return 0u;
  return ~r->seen[(uint64_t)b * r->bm_words + w] & ing_src_mask(r, w);
}

/* the ESIs of word w's missing bits, ascending, to out[0 ..] */
ING_HD void lss_put(uint32_t w, uint32_t miss, uint32_t *out) {
  while (miss) {
    *out++ = w * 32u + ing_lowbit(miss);
    miss &= miss - 1u;
  }
}

#endif /* NRQ_LISTS_SET_BODY_H */
