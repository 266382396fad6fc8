/*
 * runs_set_body.h -- the request side of packets of several symbols for reception sets and sender sets: what runs_body.h is for
 * one reception, over the member table of want_set_body.h and the segment table of syms_set_body.h.
 *
 * The listings (nrq_rxset_want_syms / nrq_rxset_held_syms, include/nanorq_hip.h) need no body of their own: a global block finds
 * its member and key (lss_block / wns_block), forms that member's query (wns_query) and walks as the single form does (rn_walk_want
 * / rn_walk_held, rn_word_pkts, the row walk); the block's key goes over its packet range (wns_put_keys).  The list is the
 * members' own lists one behind the other in block order, each packetised with its own K.
 *
 * The held emit (NRQ_TX_HELD in nrq_txset_emit_syms).  hss_packet is the packet-level part of the admission on the segment the
 * bucketing pass stored for the packet, in hs_packet's order -- no member, then the range, then the ready bit: an inadmissible
 * range is TX_BAD_RANGE whether or not the block is ready -- and hss_slot_held the per-symbol part: a packet of a block that is
 * not ready is written iff the reception behind its segment holds EVERY symbol e .. e+c-1, else TX_NOT_READY and untouched.  A
 * sender's blocks are always ready (txs_ready), so its packets get what they get without the flag.
 *
 * nrq_device.hip runs the bodies in kernels, rxset_runs_emu.cpp on the CPU.
 */
#ifndef NRQ_RUNS_SET_BODY_H
#define NRQ_RUNS_SET_BODY_H

#include <stdint.h>

#include "runs_body.h"
#include "syms_set_body.h"
#include "want_set_body.h"

/* The packet-level part of the admission of packet k (first tag `tag`, segment sg = c->seg[k]): its segment, or TXS_NONE when it
 * stays untouched for what *code says (TX_FOREIGN, TX_BAD_RANGE).  *cnt = its symbols, *ready = its block's ready bit. */
TX_HD uint32_t hss_packet(const struct txs_tab *t, const struct txs_ready *r, const struct sy_tx *y, uint32_t k, uint32_t tag, uint32_t sg,
                          int32_t *code, uint32_t *cnt, uint32_t *ready) {
  *cnt = 0u;
  *ready = 0u;
  if (sg >= TXS_MAX_SEGS) { *code = TX_FOREIGN; return TXS_NONE; }
  const struct txs_seg *S = &t->seg[sg];
  *cnt = sy_tx_count(S->b.K, tag & SY_ESI_MAX, y->G, y->nsym, k);
  if (*cnt == 0u) { *code = TX_BAD_RANGE; return TXS_NONE; }
  *ready = txs_is_ready(r, S->blk0 + tx_block(&S->b, tag));
  *code = 0;
  return sg;
}

/* does the reception behind segment sg hold ESI `esi` of the block of `tag` */
TX_HD bool hss_slot_held(const struct txs_tab *t, uint32_t sg, uint32_t tag, uint32_t esi) {
  const struct txs_seg *S = &t->seg[sg];
  return hs_slot_held(&S->h, tx_block(&S->b, tag), esi);
}

/* the kind of an admitted packet of a block that is not ready: copies of source rows, or of repair rows still to be found */
TX_HD uint32_t hss_kind(const struct txs_tab *t, uint32_t sg, uint32_t tag) {
  return (tag & SY_ESI_MAX) < t->seg[sg].b.K ? TX_HELD_SRC : TX_HELD_REP;
}

#endif /* NRQ_RUNS_SET_BODY_H */
