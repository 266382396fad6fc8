/*
 * want_set_body.h -- the bodies of a reception set's want and held listings (nrq_rxset_want / nrq_rxset_held, include/nanorq_hip.h):
 * what nrq_rx_want and nrq_rx_held give for one reception, for every block of every member in one pass over the member table
 * (struct ings_tab, ingest_set_body.h), WITH the key of each tag's member beside it -- the (keys, tags) form nrq_txset_emit takes.
 * Blocks are in the table's order: global block g = blk0[m] + b (lss_block, lists_set_body.h).
 *
 * Three passes, as the single listings: a count per global block, exclusive offsets by one scan over the nb + 1 counts, a fill
 * per global block.  Per block everything is the single form's body (wn_need / wn_bits / wn_put of want_body.h, hl_have / hl_put /
 * hl_rep_tag of held_body.h) on the member the block belongs to; what this header adds is the query of a MEMBER -- every member
 * has its own K, max_esi and rep_cap, so the ESI range that is walked (struct wn_q) is formed per block from the call's three
 * words -- and the block's keys.
 *
 * nrq_device.hip runs the bodies in kernels; rxset_want_emu.cpp runs them on the CPU in the kernels' rounds.  They only read the
 * members' books.
 */
#ifndef NRQ_WANT_SET_BODY_H
#define NRQ_WANT_SET_BODY_H

#include "lists_set_body.h"
#include "want_body.h"

/* one want call over a set: the caller's arguments as they are (wn_check has passed them) */
struct wns_call {
  uint32_t flags, extra, esi_from;
};

/* the member of global block g, the block's number in it and the member's key */
ING_HD const struct ing_rx *wns_block(const struct ings_tab *t, uint32_t g, uint32_t *b, uint32_t *key) {
  const uint32_t m = ings_member_of_block(t->blk0, t->nmem, g);
  *b = g - t->blk0[m];
  *key = t->key[m];
  return &t->r[m];
}

/* the call as member r sees it */
ING_HD struct wn_q wns_query(const struct ing_rx *r, const struct wns_call *c) { return wn_query(r, c->flags, c->extra, c->esi_from); }

/* the counts' last entry: nothing, so that the scan leaves the total there */
ING_HD void wns_count_end(const struct ings_tab *t, uint32_t g, uint32_t *cnt) {
  if (g == 0) cnt[t->nblk] = 0;
}

/* the keys of a block's tags, keys[lo .. hi): entries lo + i, lo + i + step, ... (thread i of `step`: neighbours store neighbours) */
ING_HD void wns_put_keys(uint32_t *keys, uint32_t lo, uint32_t hi, uint32_t key, uint32_t i, uint32_t step) {
  for (uint32_t j = lo + i; j < hi; j += step) keys[j] = key;
}

#endif /* NRQ_WANT_SET_BODY_H */
