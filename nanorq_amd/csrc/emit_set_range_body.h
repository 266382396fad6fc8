/*
 * emit_set_range_body.h -- the range mode of a sender set (nrq_txset_emit_all / nrq_txset_emit_all_syms, include/nanorq_hip.h):
 * the packet map of "the next symbols of every block of every member", computed on the device into the (keys, tags, nsym)
 * lists, the packets' segments and the work order the set's emit kernels (emit_set_body.h, syms_set_body.h) take.  The payload
 * kernels are the list route's, unchanged: a range packet is the list emit's packet because the same code writes it.
 *
 * THE MAP.  The set's blocks are numbered g = 0 .. nb-1 in the set's block order (nrq_txset_blocks: members sorted by (key, first
 * SBN), a member's blocks in SBN order -- the table's own order, blk0[seg] + b); block g has the K of its segment.  A call names
 *   source (0 / 1): whether the block's K source symbols are sent;
 *   rep0, nrep:     the repair ESIs K + rep0 .. K + rep0 + nrep - 1 of every block, each block with its own K;
 *   G:              symbols per packet (1 in the one-symbol call).
 * Block g's packet list is the source run [0, K) cut into packets of G from its start, the last one short (only with source),
 * then the repair run [K + rep0, K + rep0 + nrep) cut the same way:
 *   len_g = (source ? ceil(K / G) : 0) + ceil(nrep / G).
 * With source = 1 and rep0 = 0 this is the list of nrq_otx_emit_all_syms / nrq_tx_emit_range_syms(0, K + nrep), and
 * len_g = nrq_pkt_count(K, 0, K + nrep, G).  Packet j of block g has first tag (SBN_g << 24) | e, count c and key key_g.
 *   order 0, block-major:  packet (g, j) has index  sum_{g' < g} len_g' + j;
 *   order 1, interleaved:  round j holds packet j of every block with len_g > j, in block order (the rule of
 *                          nrq_otx_emit_all_syms over the set's block order; a block with fewer packets drops out of the later
 *                          rounds):  index of (g, j) = sum_{g'} min(len_g', j) + #{g' < g : len_g' > j}.
 * The map is piecewise linear over the table's segments (blocks of one segment have one K, hence one length): both sums are
 * walks over at most TXS_MAX_SEGS staged entries.
 *
 * THE PASS.  One work item per packet, w = 0 .. n-1 in BLOCK-MAJOR order whatever the packet order: item w finds its segment in
 * the prefix of cnt * len, its (b, j) in it, the packet index k by the rule above, and writes order[w] = k, seg[k], tags[k],
 * keys[k] and (several-symbol form) nsym[k].  The work order is block-major by construction, so this one pass stands for the
 * histogram, scan and place passes of the list route.
 *
 * nrq_device.hip runs txr_stage / txr_map in nrq_txs_range_kernel; txset_range_emu.cpp runs them sequentially on the CPU.
 */
#ifndef NRQ_EMIT_SET_RANGE_BODY_H
#define NRQ_EMIT_SET_RANGE_BODY_H

#include "emit_set_body.h"

/* one range call (by value in the kernel arguments) */
struct txr_call {
  uint32_t source;   /* 0 / 1 */
  uint32_t rep0, nrep;
  uint32_t G;
  uint32_t order;    /* 0 block-major, 1 interleaved */
  uint32_t n;        /* packets = work items */
  uint32_t *keys;    /* [n] out: key of packet k */
  uint32_t *tags;    /* [n] out: first tag of packet k */
  uint8_t *nsym;     /* [n] out, nullable: symbols of packet k */
  uint32_t *seg;     /* [n] out: segment of packet k */
  uint32_t *worder;  /* [n] out: packet of work item w */
};

/* the per-segment words a workgroup stages (LDS on the device, plain arrays in the emulation) */
struct txr_stage_t {
  uint32_t cnt[TXS_MAX_SEGS], K[TXS_MAX_SEGS], blk0[TXS_MAX_SEGS], key[TXS_MAX_SEGS], sbn0[TXS_MAX_SEGS];
  uint32_t len[TXS_MAX_SEGS];       /* packets per block of the segment */
  uint32_t pre[TXS_MAX_SEGS + 1u];  /* work items in front of the segment: the prefix of cnt * len; pre[nseg] = n */
};

/* packets of the source run and of the repair run of a block of K source symbols */
TX_HD uint32_t txr_src_pkts(uint32_t K, uint32_t source, uint32_t G) { return source ? (K + G - 1u) / G : 0u; }
TX_HD uint32_t txr_rep_pkts(uint32_t nrep, uint32_t G) { return nrep / G + (nrep % G ? 1u : 0u); }
TX_HD uint32_t txr_len(uint32_t K, uint32_t source, uint32_t nrep, uint32_t G) { return txr_src_pkts(K, source, G) + txr_rep_pkts(nrep, G); }

/* packet j (below txr_len) of a block of K source symbols: its first ESI and its count */
TX_HD void txr_pkt(uint32_t K, const struct txr_call *c, uint32_t j, uint32_t *first, uint32_t *cnt) {
  const uint32_t ps = txr_src_pkts(K, c->source, c->G);
  if (j < ps) {
    const uint32_t e = j * c->G;
    *first = e;
    *cnt = K - e < c->G ? K - e : c->G;
  } else {
    const uint32_t q = (j - ps) * c->G; /* (below nrep) */
    *first = K + c->rep0 + q;
    *cnt = c->nrep - q < c->G ? c->nrep - q : c->G;
  }
}

/* staging, part 1: entry i < nseg from the table */
TX_HD void txr_stage(const struct txs_tab *t, const struct txr_call *c, uint32_t i, struct txr_stage_t *s) {
  s->cnt[i] = t->cnt[i];
  s->K[i] = t->seg[i].b.K;
  s->blk0[i] = t->blk0[i];
  s->key[i] = t->key[i];
  s->sbn0[i] = t->sbn0[i];
  s->len[i] = txr_len(t->seg[i].b.K, c->source, c->nrep, c->G);
}
/* staging, part 2 (once part 1 is complete for every entry): pre[i] for i <= nseg */
TX_HD void txr_stage_prefix(uint32_t nseg, uint32_t i, struct txr_stage_t *s) {
  uint32_t p = 0;
  for (uint32_t q = 0; q < i && q < nseg; q++) p += s->cnt[q] * s->len[q];
  s->pre[i] = p;
}

/* work item w < pre[nseg] */
TX_HD void txr_map(const struct txr_stage_t *s, uint32_t nseg, const struct txr_call *c, uint32_t w) {
  uint32_t sg = 0;
  while (sg + 1u < nseg && w >= s->pre[sg + 1u]) sg++;
  const uint32_t len = s->len[sg], r = w - s->pre[sg], b = r / len, j = r - b * len;
  uint32_t k = w;
  if (c->order) {
    /* the rounds in front: min(len', j) packets of every block; then the live blocks in front of this one in round j (the
     * blocks of this segment in front of b are live: they have this block's length) */
    k = b;
    for (uint32_t q = 0; q < nseg; q++) {
      const uint32_t lq = s->len[q];
      k += s->cnt[q] * (lq < j ? lq : j);
      if (q < sg && lq > j) k += s->cnt[q];
    }
  }
  uint32_t e, cnt;
  txr_pkt(s->K[sg], c, j, &e, &cnt);
  c->worder[w] = k;
  if (k >= c->n) return; /* (never: n is pre[nseg], the host's count over the same table) */
  c->seg[k] = sg;
  c->tags[k] = tx_tag(s->sbn0[sg] + b, e);
  c->keys[k] = s->key[sg];
  if (c->nsym) c->nsym[k] = (uint8_t)cnt;
}

#endif /* NRQ_EMIT_SET_RANGE_BODY_H */
