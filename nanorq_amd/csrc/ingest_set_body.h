/*
 * ingest_set_body.h -- the per-thread bodies of a reception set's ingest (nrq_rxset_*, include/nanorq_hip.h): the packets of many
 * receptions in one buffer, each with a 32-bit key beside its tag, are booked into their receptions by ONE chain of the seven
 * passes of ingest_body.h over a table of members in device memory.
 *
 * A member is one reception (struct ing_rx) under a key; an object is two members, one per block class, under a key of its own.
 * The table is sorted by (key, sbn0) on the host.  The set numbers the blocks of all members in one row: member m's block b is
 * global block blk0[m] + b.  The per-block passes (done, scan) run once per global block, the per-tile passes (hist, classify)
 * count per global block; everything else is ing_done_part / ing_done_finish / ing_cand / ing_classify / ing_fold of
 * ingest_body.h on the member a packet belongs to, which pass 1 finds once and stores beside the decoded tag.  As there, every
 * decision depends on packet order only: a member ends with the books nrq_rx_add gives it for the packets of its key alone.
 *
 * nrq_device.hip instantiates the bodies in kernels; rxset_emu.cpp runs them sequentially on the CPU.
 */
#ifndef NRQ_INGEST_SET_BODY_H
#define NRQ_INGEST_SET_BODY_H

#include "ingest_body.h"

#define INGS_MAX_MEMBERS 64u  /* NRQ_RXSET_MAX_MEMBERS: pass 1 searches the table linearly from LDS */
#define INGS_MAX_BLOCKS 1024u /* NRQ_RXSET_MAX_BLOCKS: one LDS counter per block in pass 3, four in pass 5 */
/* in ings_call.mem[]: no member holds the packet's SBN, but the key is an object's and the SBN is not below its Z; the low bits
 * name a member of that object (for its max_esi) */
#define INGS_FOREIGN 0x80000000u

/* the member table (device memory; the emulation passes a host copy) */
struct ings_tab {
  uint32_t nmem, nblk;                 /* members; blocks over all members */
  uint32_t key[INGS_MAX_MEMBERS];
  uint32_t sbn0[INGS_MAX_MEMBERS];     /* (copies of r[m].sbn0 and r[m].nblk: what the search of pass 1 stages) */
  uint32_t cnt[INGS_MAX_MEMBERS];
  uint32_t objZ[INGS_MAX_MEMBERS];     /* the member is a block class of an object of Z blocks; 0: a plain reception */
  uint32_t blk0[INGS_MAX_MEMBERS + 1]; /* global number of the member's first block; blk0[nmem] = nblk */
  uint32_t pad_;
  struct ing_rx r[INGS_MAX_MEMBERS];
};

/* one call: struct ing_call with c.base = [tab.nblk][ntiles], c.tags NULL = the tag is in the packet */
struct ings_call {
  struct ing_call c;
  const uint32_t *keys; /* [n], or NULL: the key is in the packet (key_inline) or 0 */
  uint32_t key_inline;  /* packet = key (32 bits, network byte order), FEC Payload ID, payload */
  uint32_t *mem;        /* [n] member of the packet (pass 1 -> the rest): an index, INGS_FOREIGN | index, or ING_NONE */
};

ING_HD uint32_t ings_payload_off(const struct ings_call *s) { return s->c.tags ? 0u : s->key_inline ? 8u : 4u; }

ING_HD uint32_t ings_be32(const uint8_t *p) {
  return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
}

/* the member of (key, sbn).  key / sbn0 / cnt / objZ: the table's arrays or a staged copy of them */
ING_HD uint32_t ings_find(const uint32_t *key, const uint32_t *sbn0, const uint32_t *cnt, const uint32_t *objZ, uint32_t nmem, uint32_t k,
                          uint32_t sbn) {
  uint32_t m = ING_NONE;
  for (uint32_t i = 0; i < nmem; i++) {
    if (key[i] != k) continue;
    if (sbn >= sbn0[i] && sbn - sbn0[i] < cnt[i]) return i;
    if (objZ[i] && sbn >= objZ[i]) m = INGS_FOREIGN | i;
  }
  return m;
}

/* the member that holds global block g (g < blk0[nmem]) */
ING_HD uint32_t ings_member_of_block(const uint32_t *blk0, uint32_t nmem, uint32_t g) {
  uint32_t m = 0;
  while (m + 1u < nmem && blk0[m + 1u] <= g) m++;
  return m;
}

/* pass 1: key and tag of packet k; the caller finds the member m of (key, tag >> 24) (ings_find) and hands it to ings_first */
ING_HD void ings_decode(const struct ings_call *s, uint32_t k, uint32_t *key, uint32_t *tag) {
  const uint8_t *p = s->c.pkts + (uint64_t)k * s->c.pkt_stride;
  *key = s->keys ? s->keys[k] : s->key_inline ? ings_be32(p) : 0u;
  *tag = s->c.tags ? s->c.tags[k] : ings_be32(p + (s->key_inline ? 4u : 0u));
}
ING_HD void ings_first(const struct ings_tab *t, const struct ings_call *s, uint32_t k, uint32_t tag, uint32_t m) {
  s->c.tagv[k] = tag;
  s->mem[k] = m;
  if (m >= INGS_MAX_MEMBERS) return;
  const struct ing_rx *r = &t->r[m];
  const uint32_t b = ing_block(r, tag), esi = tag & 0xFFFFFFu;
  if (esi <= r->max_esi) ING_ATOMIC_MIN(&r->first[(uint64_t)b * r->m1 + esi], k);
}

/* passes 3 and 5: the global block of a repair candidate (ing_cand on the packet's member), or ING_NONE */
ING_HD uint32_t ings_cand(const struct ings_tab *t, const struct ings_call *s, uint32_t k) {
  const uint32_t m = s->mem[k];
  if (m >= INGS_MAX_MEMBERS) return ING_NONE;
  const uint32_t b = ing_cand(&t->r[m], &s->c, k);
  return b == ING_NONE ? ING_NONE : t->blk0[m] + b;
}

/* pass 5: the result of packet k.  `row` = the repair row it would take if it is a candidate.  The SBN >= Z rule of an attached
 * object (nrq_orx_add) is decided here: ERR above max_esi, else IGN. */
ING_HD void ings_classify(const struct ings_tab *t, const struct ings_call *s, uint32_t k, uint32_t row) {
  const uint32_t m = s->mem[k];
  if (m < INGS_MAX_MEMBERS) {
    ing_classify(&t->r[m], &s->c, k, row);
    return;
  }
  s->c.dst[k] = 0;
  if (m != ING_NONE) s->c.codes[k] = (s->c.tagv[k] & 0xFFFFFFu) > t->r[m & ~INGS_FOREIGN].max_esi ? ING_ERR : ING_IGN;
}

/* pass 7 */
ING_HD void ings_fold(const struct ings_tab *t, const struct ings_call *s, uint32_t k) {
  const uint32_t m = s->mem[k];
  if (m < INGS_MAX_MEMBERS) ing_fold(&t->r[m], &s->c, k);
}

#endif /* NRQ_INGEST_SET_BODY_H */
