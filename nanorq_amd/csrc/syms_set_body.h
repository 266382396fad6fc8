/*
 * syms_set_body.h -- packets of several symbols (RFC 6330 section 4.4.2) for reception sets and sender sets: the bodies of
 * nrq_rxset_add_syms and nrq_txset_emit_syms (include/nanorq_hip.h).  The slot layer of syms_body.h over the member table of
 * ingest_set_body.h and the segment table of emit_set_body.h.
 *
 * Packets and slots are those of syms_body.h: packet k carries c_k <= G symbols of ONE block with consecutive ESIs behind one
 * header (hdr = 0, 4, or 8 with the key in front of the FEC Payload ID), symbol i at hdr + i * T; slot (k, i) has index k * G + i.
 *
 * Ingest.  The seven passes run over the n * G slots, counting per GLOBAL block as a set does.  Pass 1 (sys_first) decodes the
 * packet's key and first tag (ings_decode), finds its member (ings_find) and gives every slot its kind and tag by sy_first's rule
 * with the member's K and max_esi.  The member is a property of the PACKET -- the SBN never changes inside one -- so it is stored
 * once per packet (n words, not n * G; s->mem[k], written by the packet's slot 0); per slot there is the kind byte.  The later
 * passes run the ingest_body.h bodies on the slot's member for live slots only (what ings_cand / ings_classify / ings_fold do for
 * a packet, with the member looked up under the packet's index and the books under the slot's).  A packet of an attached
 * object's key with an SBN >= Z (INGS_FOREIGN) gets nrq_orx_add_syms' answer slot by slot, decided in pass 1 from the object's
 * max_esi: SY_BAD (ERR) or SYS_IGN.
 *
 * Emit.  Admission is per packet (sys_tx_admit, in sy_tx_admit's order: no member, not ready, range) on the segment the
 * bucketing pass stored in c.seg[k]; the count rule takes the segment's K.
 *
 * nrq_device.hip instantiates the bodies in kernels; syms_set_emu.cpp runs them sequentially on the CPU.
 */
#ifndef NRQ_SYMS_SET_BODY_H
#define NRQ_SYMS_SET_BODY_H

#include <stdint.h>

#include "emit_set_body.h"
#include "ingest_set_body.h"
#include "syms_body.h"

/* a fourth slot kind beside SY_ABSENT / SY_LIVE / SY_BAD: a symbol of an attached object's key whose SBN is not below the
 * object's Z and whose ESI the object would take: IGN and nothing else */
#define SYS_IGN 3u

/* ---- ingest ---- */
/* one call: s->c.n counts SLOTS (tagv, codes, fidx, dst per slot), s->mem has an entry per PACKET; y as in syms_body.h */

/* the member of slot sl's packet */
ING_HD uint32_t sys_member(const struct ings_call *s, const struct sy_rx *y, uint32_t sl) { return s->mem[sl / y->G]; }

/* pass 1 of slot sl.  m: the member of its packet's (key, SBN), found by the caller from `tag0` (ings_decode, ings_find) */
ING_HD void sys_first(const struct ings_tab *t, const struct ings_call *s, const struct sy_rx *y, uint32_t sl, uint32_t tag0, uint32_t m) {
  const uint32_t k = sl / y->G, i = sl - k * y->G, e = tag0 & SY_ESI_MAX;
  uint32_t kind = SY_ABSENT, tag = tag0;
  if (i == 0u) s->mem[k] = m;
  if (m < INGS_MAX_MEMBERS) {
    const struct ing_rx *r = &t->r[m];
    const uint32_t cnt = sy_rx_count(r->K, e, y->G, y->nsym, k);
    if (cnt == 0u) kind = i == 0u ? SY_BAD : SY_ABSENT;
    else if (i < cnt) {
      if (e + i > SY_ESI_MAX) kind = SY_BAD;
      else { kind = SY_LIVE; tag = tag0 + i; }
    }
    if (kind == SY_LIVE && e + i <= r->max_esi) ING_ATOMIC_MIN(&r->first[(uint64_t)ing_block(r, tag0) * r->m1 + e + i], sl);
  } else if (m != ING_NONE) { /* INGS_FOREIGN: the object has no block of this SBN (nrq_orx_add_syms' rule: a given count or G) */
    const uint32_t cnt = y->nsym ? y->nsym[k] : y->G;
    if (cnt == 0u || cnt > y->G) kind = i == 0u ? SY_BAD : SY_ABSENT;
    else if (i < cnt) kind = e + i > t->r[m & ~INGS_FOREIGN].max_esi ? SY_BAD : SYS_IGN;
  }
  s->c.tagv[sl] = tag;
  y->kind[sl] = (uint8_t)kind;
}

/* passes 3 and 5: the global block of a slot that is a repair candidate, or ING_NONE */
ING_HD uint32_t sys_cand(const struct ings_tab *t, const struct ings_call *s, const struct sy_rx *y, uint32_t sl) {
  if (y->kind[sl] != SY_LIVE) return ING_NONE;
  const uint32_t m = sys_member(s, y, sl), b = ing_cand(&t->r[m], &s->c, sl);
  return b == ING_NONE ? ING_NONE : t->blk0[m] + b;
}

/* pass 5 */
ING_HD void sys_classify(const struct ings_tab *t, const struct ings_call *s, const struct sy_rx *y, uint32_t sl, uint32_t row) {
  const uint32_t kind = y->kind[sl];
  if (kind == SY_LIVE) { ing_classify(&t->r[sys_member(s, y, sl)], &s->c, sl, row); return; }
  s->c.dst[sl] = 0;
  if (kind == SY_BAD) { s->c.codes[sl] = ING_ERR; s->c.fidx[sl] = sl; }
  else if (kind == SYS_IGN) s->c.codes[sl] = ING_IGN;
}

/* pass 7 */
ING_HD void sys_fold(const struct ings_tab *t, const struct ings_call *s, const struct sy_rx *y, uint32_t sl) {
  if (y->kind[sl] == SY_LIVE) ing_fold(&t->r[sys_member(s, y, sl)], &s->c, sl);
}

/* ---- emit ---- */
/* c->n counts PACKETS, c->tags are first tags, c->seg / c->order are per packet (nrq_txs_hist_kernel and nrq_txs_place_kernel over
 * the first tags); y->G and y->nsym as in syms_body.h (list mode only: sets have no range forms) */

/* admission of packet k (first tag `tag`, segment sg = c->seg[k]): true and *cnt = its symbols when it is written; false when it
 * stays untouched, *code says why */
TX_HD bool sys_tx_admit(const struct txs_tab *t, const struct txs_ready *r, const struct sy_tx *y, uint32_t k, uint32_t tag, uint32_t sg,
                        int32_t *code, uint32_t *cnt) {
  *cnt = 0u;
  if (sg >= TXS_MAX_SEGS) { *code = TX_FOREIGN; return false; }
  const struct txs_seg *S = &t->seg[sg];
  if (!txs_is_ready(r, S->blk0 + tx_block(&S->b, tag))) { *code = TX_NOT_READY; return false; }
  *cnt = sy_tx_count(S->b.K, tag & SY_ESI_MAX, y->G, y->nsym, k);
  if (*cnt == 0u) { *code = TX_BAD_RANGE; return false; }
  *code = 0;
  return true;
}

/* the payload path of a set's several-symbol emit (the rule of nrq_txset_emit): al = the OR of the packet buffer's address and
 * stride, T and every row table's address and stride; 4 = the 16-byte walk under the 8-byte header (TXS_V16_KEY) */
TX_HD int sys_emit_path(uint64_t al, uint32_t hdr, uint32_t force_dword) {
  if ((al & 15u) == 0 && !force_dword) return hdr == 8u ? 4 : hdr ? TX_V16_SHIFT : TX_V16;
  return (al & 3u) == 0 ? TX_DWORD : TX_BYTE;
}

/* one whole packet of cnt symbols in any header form, a byte at a time (the emulation; every wider path must give these bytes):
 * symbol 0 with the header as a one-symbol packet, the others behind it */
TX_HD void sys_emit_bytes(const struct txs_seg *S, const struct txs_call *c, uint32_t k, uint32_t key, uint32_t tag, uint32_t cnt) {
  uint32_t cols[TX_COLS];
  for (uint32_t i = 0; i < cnt; i++) {
    const uint32_t n = tx_rows(&S->b, tag + i, cols);
    struct txs_call c1 = *c;
    if (i) { c1.pkts = c->pkts + c->hdr + (uint64_t)i * c->T; c1.hdr = 0u; }
    txs_emit_bytes(tx_base(&S->b, tag + i), &c1, k, key, tag + i, cols, n);
  }
}

#endif /* NRQ_SYMS_SET_BODY_H */
