/*
 * syms_body.h -- packets of several symbols (RFC 6330 section 4.4.2) for the device-resident emit and ingest: the bodies of
 * nrq_tx_emit_syms / nrq_tx_emit_range_syms / nrq_rx_add_syms and their object forms (include/nanorq_hip.h), built over
 * emit_body.h and ingest_body.h.
 *
 * A packet carries up to G symbols (1 <= G <= SY_G_MAX) of ONE source block with consecutive ESIs: packet k has a first tag
 * (SBN, e_k) and a count c_k; its symbol i < c_k has ESI e_k + i -- computed in ESI space, the SBN never changes inside a packet,
 * an ESI above 2^24 - 1 does not exist -- and its payload at hdr + i * T in the packet (hdr = 0, or 4 behind the inline FEC
 * Payload ID of the first tag).  SLOT (k, i) has index k * G + i; the expansion of a packet list is its one-symbol packets in
 * slot order.
 *
 * Ingest.  The seven passes of ingest_body.h run over the n * G slots as if they were packets: pass 1 (sy_first) decodes a slot's
 * tag from its packet's first tag and says what the slot is (SY_LIVE / SY_BAD / SY_ABSENT, kept in a byte per slot); the later
 * passes run their ingest_body.h bodies on live slots only, so that arrival order is slot order and the reception ends in exactly
 * the state nrq_rx_add leaves after the expansion.  Emit.  Admission is per packet (sy_tx_admit: tx_admit of the first tag and the
 * sender's range rule); an admitted packet's slots each get their column list (tx_rows) and the payload is written as one
 * contiguous run.  Range forms cut every block's source run and repair run into packets of G (sy_range_pkt) and reuse the
 * block-major / interleaved maps of emit_body.h with packets per block in place of ESIs per block.
 *
 * What is NOT here, because the one-symbol forms' code serves as it is: the payload path rule (tx_emit_path / tx_align,
 * emit_body.h), the payload walk (the kernels' tx_payload over a run of symbols), the ranking of repair candidates (ing_rank_wg)
 * and the host set-up of a call (bucketing, the ingest call's scratch).  nrq_device.hip instantiates the bodies below in kernels of
 * their own -- entry points only, around those shared bodies; syms_emu.cpp runs them sequentially on the CPU.
 */
#ifndef NRQ_SYMS_BODY_H
#define NRQ_SYMS_BODY_H

#include <stdint.h>

#include "emit_body.h"
#include "ingest_body.h"

#define SY_G_MAX 64u       /* NRQ_PKT_SYMS_MAX: symbols a packet can carry (a wave's lanes) */
#define SY_ESI_MAX 0xFFFFFFu
#define TX_BAD_RANGE (-3)  /* NRQ_TX_BAD_RANGE: a packet whose count or ESI range a sender refuses */

/* what a slot is to the reception (a byte per slot, pass 1 -> 3, 5, 7) */
#define SY_ABSENT 0u /* not a symbol of this reception: behaves as a packet of no reception (result untouched) */
#define SY_LIVE 1u   /* a symbol: goes through the passes as a packet of its own */
#define SY_BAD 2u    /* ERR and nothing else: slot 0 of a packet with a malformed count, or a symbol whose ESI would pass 2^24 - 1 */

/* ---- the count rule ---- */
/* symbols of a packet with first ESI e of a block of K source symbols when no count is given: G, but a packet of source symbols
 * ends with the block's last source symbol */
TX_HD uint32_t sy_rule(uint32_t K, uint32_t e, uint32_t G) { return e < K ? (K - e < G ? K - e : G) : G; }

/* a receiver's count (liberal): a given count 1..G as it is, 0 for a malformed one; none given: the rule */
TX_HD uint32_t sy_rx_count(uint32_t K, uint32_t e, uint32_t G, const uint8_t *nsym, uint32_t k) {
  if (!nsym) return sy_rule(K, e, G);
  const uint32_t c = nsym[k];
  return c >= 1u && c <= G ? c : 0u;
}

/* a sender's count (strict), 0 = TX_BAD_RANGE: a count outside 1..G, a given count that takes a packet of source symbols to K
 * or beyond, a last ESI above 2^24 - 1 */
TX_HD uint32_t sy_tx_count(uint32_t K, uint32_t e, uint32_t G, const uint8_t *nsym, uint32_t k) {
  const uint32_t c = nsym ? nsym[k] : sy_rule(K, e, G);
  if (c == 0u || c > G) return 0u;
  if (e < K && e + c > K) return 0u;
  if (e + c - 1u > SY_ESI_MAX) return 0u;
  return c;
}

/* ---- the range packetisation ---- */
/* ESIs esi0 .. esi0+n-1 of a block of K source symbols: the source run [esi0, min(K, esi0+n)) and the repair run
 * [max(K, esi0), esi0+n), each cut into packets of G from its start, the last one short */
TX_HD uint32_t sy_src_pkts(uint32_t K, uint32_t esi0, uint32_t n, uint32_t G) {
  const uint64_t end = (uint64_t)esi0 + n, se = end < K ? end : K;
  return se > esi0 ? (uint32_t)((se - esi0 + G - 1u) / G) : 0u;
}
TX_HD uint32_t sy_rep_pkts(uint32_t K, uint32_t esi0, uint32_t n, uint32_t G) {
  const uint64_t end = (uint64_t)esi0 + n, rs = esi0 > K ? esi0 : K;
  return end > rs ? (uint32_t)((end - rs + G - 1u) / G) : 0u;
}
TX_HD uint32_t sy_pkt_count(uint32_t K, uint32_t esi0, uint32_t n, uint32_t G) {
  return sy_src_pkts(K, esi0, n, G) + sy_rep_pkts(K, esi0, n, G);
}
/* packet j (below sy_pkt_count) of that block: its first ESI and count */
TX_HD void sy_range_pkt(uint32_t K, uint32_t esi0, uint32_t n, uint32_t G, uint32_t j, uint32_t *first, uint32_t *cnt) {
  const uint32_t ps = sy_src_pkts(K, esi0, n, G);
  const uint64_t end = (uint64_t)esi0 + n;
  uint64_t f, e;
  if (j < ps) { f = (uint64_t)esi0 + (uint64_t)j * G; e = end < K ? end : K; }
  else { f = (esi0 > K ? esi0 : K) + (uint64_t)(j - ps) * G; e = end; }
  *first = (uint32_t)f;
  *cnt = (uint32_t)(e - f < G ? e - f : G);
}
/* and back: the packet of that block that carries ESI e (esi0 <= e < esi0 + n) */
TX_HD uint32_t sy_range_index(uint32_t K, uint32_t esi0, uint32_t n, uint32_t G, uint32_t e) {
  if (e < K) return (e - esi0) / G;
  return sy_src_pkts(K, esi0, n, G) + (e - (esi0 > K ? esi0 : K)) / G;
}

/* ---- emit ---- */
/* what an emit call carries beside its tx_call (whose n, nL, nS count PACKETS: packets in the list, packets per block of each
 * class in range mode) */
struct sy_tx {
  uint32_t G;
  const uint8_t *nsym;  /* list mode, nullable: count of packet k; NULL: the rule */
  uint8_t *nsym_out;    /* range mode, nullable: the count of each packet */
  uint32_t eL, eS;      /* range mode: ESIs per block of the larger / the smaller class (esi0 .. esi0+eL-1) */
};

/* slot 0's tag and the count of packet k; list mode: *cnt may be 0 (TX_BAD_RANGE once the block is known) */
template <bool MULTI>
TX_HD uint32_t sy_tx_packet(const struct tx_src *s, const struct tx_call *c, const struct sy_tx *y, uint32_t k, uint32_t *cnt, bool *ranged) {
  *ranged = !c->tags;
  if (c->tags) { *cnt = 0u; return c->tags[k]; }
  uint32_t b, j, first;
  if (c->interleave) tx_il_pair<MULTI>(s, c, k, &b, &j);
  else tx_bm<MULTI>(s, c, k, &b, &j);
  const uint32_t tag = tx_tag(s->sbn0 + b, 0u), g = tx_seg<MULTI>(s, tag);
  const struct tx_blk t = tx_pick(s, MULTI && g < TX_SEGS ? g : 0u);
  sy_range_pkt(t.K, c->esi0, MULTI && b >= s->ZL ? y->eS : y->eL, y->G, j, &first, cnt);
  return tag | first;
}

/* admission of packet k (first tag `tag`): its segment, or TX_SEGS when the packet stays untouched; *cnt = its symbols */
template <bool MULTI>
TX_HD uint32_t sy_tx_admit(const struct tx_src *s, const struct sy_tx *y, uint32_t tag, uint32_t k, bool ranged, int32_t *code, uint32_t *cnt) {
  const uint32_t g = tx_admit<MULTI>(s, tag, code);
  if (g == TX_SEGS) { *cnt = 0u; return TX_SEGS; }
  if (!ranged) {
    const struct tx_blk t = tx_pick(s, MULTI ? g : 0u);
    *cnt = sy_tx_count(t.K, tag & SY_ESI_MAX, y->G, y->nsym, k);
  }
  if (*cnt == 0u) { *code = TX_BAD_RANGE; return TX_SEGS; }
  return g;
}

/* ---- ingest ---- */
struct sy_rx {
  uint32_t G;
  const uint8_t *nsym; /* nullable: count of packet k; NULL: the rule */
  uint8_t *kind;       /* a byte per slot: SY_ABSENT / SY_LIVE / SY_BAD */
};

/* the first tag of packet k (c->pkts / c->tags as in ing_call; c->n counts slots) */
ING_HD uint32_t sy_first_tag(const struct ing_call *c, uint32_t k) {
  if (c->tags) return c->tags[k];
  const uint8_t *p = c->pkts + (uint64_t)k * c->pkt_stride; /* SBN (8 bits) and ESI (24 bits), network byte order */
  return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
}

/* pass 1 of slot s: its tag, what it is, and the first arrival of its (block, ESI) by slot index */
ING_HD void sy_first(const struct ing_rx *r, const struct ing_call *c, const struct sy_rx *y, uint32_t s) {
  const uint32_t k = s / y->G, i = s - k * y->G;
  const uint32_t tag0 = sy_first_tag(c, k), e = tag0 & SY_ESI_MAX, b = ing_block(r, tag0);
  uint32_t kind = SY_ABSENT, tag = tag0;
  if (b != ING_NONE) {
    const uint32_t cnt = sy_rx_count(r->K, e, y->G, y->nsym, k);
    if (cnt == 0u) kind = i == 0u ? SY_BAD : SY_ABSENT;
    else if (i < cnt) {
      if (e + i > SY_ESI_MAX) kind = SY_BAD;
      else { kind = SY_LIVE; tag = tag0 + i; }
    }
  }
  c->tagv[s] = tag;
  y->kind[s] = (uint8_t)kind;
  if (kind == SY_LIVE && e + i <= r->max_esi) ING_ATOMIC_MIN(&r->first[(uint64_t)b * r->m1 + e + i], s);
}

/* passes 3 and 5: a slot's repair candidacy */
ING_HD uint32_t sy_cand(const struct ing_rx *r, const struct ing_call *c, const struct sy_rx *y, uint32_t s) {
  return y->kind[s] == SY_LIVE ? ing_cand(r, c, s) : ING_NONE;
}

/* pass 5 */
ING_HD void sy_classify(const struct ing_rx *r, const struct ing_call *c, const struct sy_rx *y, uint32_t s, uint32_t row) {
  const uint32_t kind = y->kind[s];
  if (kind == SY_LIVE) { ing_classify(r, c, s, row); return; }
  c->dst[s] = 0;
  if (kind == SY_BAD) { c->codes[s] = ING_ERR; c->fidx[s] = s; }
}

/* pass 7 */
ING_HD void sy_fold(const struct ing_rx *r, const struct ing_call *c, const struct sy_rx *y, uint32_t s) {
  if (y->kind[s] == SY_LIVE) ing_fold(r, c, s);
}

/* the copy's word: the widest every address of the call allows (al: the OR of the packet buffer's address and stride, the payload
 * offset, T and both row tables' addresses and strides); 16, 4 or 1 bytes */
ING_HD uint32_t sy_copy_word(uint64_t al) { return (al & 15u) == 0 ? 16u : (al & 3u) == 0 ? 4u : 1u; }

#endif /* NRQ_SYMS_BODY_H */
