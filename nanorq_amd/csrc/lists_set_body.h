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

/* 32-bit words of a block's seen bitmap that cover its source ESIs */
ING_HD uint32_t lss_words(const struct ing_rx *r) { return (r->K + 31u) / 32u; }

/* the missing source ESIs of word w of block b (the last word masked at K; w beyond the words: none) */
ING_HD uint32_t lss_miss(const struct ing_rx *r, uint32_t b, uint32_t w) {
  if (w >= lss_words(r)) return 0u;
  const uint32_t nb = r->K - w * 32u < 32u ? r->K - w * 32u : 32u;
  return ~r->seen[(uint64_t)b * r->bm_words + w] & (nb == 32u ? 0xFFFFFFFFu : ((1u << nb) - 1u));
}

ING_HD uint32_t lss_popc(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__popc(v);
#else
  return (uint32_t)__builtin_popcount(v);
#endif
}

/* the ESIs of word w's missing bits, ascending, to out[0 ..] */
ING_HD void lss_put(uint32_t w, uint32_t miss, uint32_t *out) {
  while (miss) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t i = (uint32_t)__ffs(miss) - 1u;
#else
    const uint32_t i = (uint32_t)__builtin_ctz(miss);
#endif
    *out++ = w * 32u + i;
    miss &= miss - 1u;
  }
}

#endif /* NRQ_LISTS_SET_BODY_H */
