/*
 * emit_set_body.h -- the per-packet bodies of a sender set's emit (nrq_txset_*, include/nanorq_hip.h): the packets of many
 * transmissions and objects, each named by a 32-bit key beside its tag, written into ONE buffer by one chain of kernels over a
 * table of segments in device memory.  The send-side counterpart of ingest_set_body.h.
 *
 * A segment is one tx_blk of emit_body.h under a key: a transmission is one segment, an object up to TX_SEGS (class L, class S,
 * a staged last block).  The table is sorted by (key, sbn0) on the host.  The set numbers the blocks of all segments in one row:
 * segment g's block b is global block blk0[g] + b.  A packet's segment is found once, by a linear search over the compact key /
 * sbn0 / cnt arrays (txs_find), and stored beside the packet; the work order is block-major over the global blocks (txs_bin: one
 * bucket per global block, one more for packets of no member).
 *
 * Ready state.  Whether a global block may be emitted is NOT in the table: a relay's ready mask is host state that changes
 * without any call on the set, so every emit carries a bit per global block by value (txs_ready, 128 bytes of kernel arguments),
 * gathered from the members' masks as they are at that call.  Held symbols (NRQ_TX_HELD) are answered from the tx_held_seg of
 * the segment -- zeros for a sender, whose blocks are always ready.
 *
 * Packet forms: hdr = 0 (payload only), 4 (FEC Payload ID, payload) or 8 (key in network byte order, FEC Payload ID, payload).
 *
 * nrq_device.hip instantiates these bodies in its kernels; txset_emu.cpp runs them sequentially on the CPU.
 */
#ifndef NRQ_EMIT_SET_BODY_H
#define NRQ_EMIT_SET_BODY_H

#include "emit_body.h"

#define TXS_MAX_SEGS 64u     /* NRQ_TXSET_MAX_SEGS: the search walks the table linearly from LDS */
#define TXS_MAX_BLOCKS 1024u /* NRQ_TXSET_MAX_BLOCKS: one LDS counter per block in the bucketing passes, one ready bit per block */
#define TXS_NONE 0xFFFFFFFFu /* the segment of a packet that belongs to no member */

/* one table segment */
struct txs_seg {
  struct tx_blk b;
  struct tx_held_seg h; /* the books of the reception a relay's segment reads; zeros for a sender */
  uint32_t key;
  uint32_t blk0;        /* global number of the segment's first block */
};

/* the segment table (device memory; the emulation passes a host copy) */
struct txs_tab {
  uint32_t nseg, nblk;            /* segments; blocks over all segments */
  uint32_t key[TXS_MAX_SEGS];     /* (copies of seg[g].key, .b.sbn0, .b.nblk and .blk0: what the search stages) */
  uint32_t sbn0[TXS_MAX_SEGS];
  uint32_t cnt[TXS_MAX_SEGS];
  uint32_t blk0[TXS_MAX_SEGS];
  struct txs_seg seg[TXS_MAX_SEGS];
};

/* a bit per global block: its packets may be emitted (by value in the kernel arguments) */
struct txs_ready {
  uint32_t w[TXS_MAX_BLOCKS / 32u];
};

/* one emit call */
struct txs_call {
  uint8_t *pkts;         /* packet k at pkts + k*pkt_stride */
  uint64_t pkt_stride;
  uint32_t n;            /* packets (work items) */
  uint32_t hdr;          /* bytes in front of the payload: 0, 4 (FEC Payload ID) or 8 (key, FEC Payload ID) */
  uint32_t T;
  uint32_t pad_;
  const uint32_t *keys;  /* [n], or NULL: every key is 0 */
  const uint32_t *tags;  /* [n] */
  uint32_t *seg;         /* [n] segment of packet k (first pass -> the rest): an index or TXS_NONE */
  uint32_t *order;       /* [n] packet of work item w */
  int32_t *results;      /* nullable: 0 written, TX_FOREIGN no member, TX_NOT_READY */
};

TX_HD uint32_t txs_key_of(const struct txs_call *c, uint32_t k) { return c->keys ? c->keys[k] : 0u; }

/* the segment of (key, sbn), or TXS_NONE.  key / sbn0 / cnt: the table's arrays or a staged copy of them */
TX_HD uint32_t txs_find(const uint32_t *key, const uint32_t *sbn0, const uint32_t *cnt, uint32_t nseg, uint32_t k, uint32_t sbn) {
  for (uint32_t i = 0; i < nseg; i++)
    if (key[i] == k && sbn >= sbn0[i] && sbn - sbn0[i] < cnt[i]) return i;
  return TXS_NONE;
}

/* the bucket of a packet of segment sg: its global block, or nblk ("no member") */
TX_HD uint32_t txs_bin(const uint32_t *sbn0, const uint32_t *blk0, uint32_t nblk, uint32_t sg, uint32_t tag) {
  return sg == TXS_NONE ? nblk : blk0[sg] + ((tag >> 24) - sbn0[sg]);
}

/* the ready bit of global block g; the mask word is picked by value (no dynamic index into the kernel arguments) */
TX_HD uint32_t txs_is_ready(const struct txs_ready *r, uint32_t g) {
  uint32_t w = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (uint32_t i = 0; i < TXS_MAX_BLOCKS / 32u; i++) w = i == (g >> 5) ? r->w[i] : w;
  return (w >> (g & 31u)) & 1u;
}

/* What a packet of `tag` in segment S gets: true and *kind (TX_READY / TX_HELD_SRC / TX_HELD_REP) when it is written, false when
 * it stays untouched; *code says why (tx_admit and tx_admit_held of emit_body.h on one segment; held = NRQ_TX_HELD).  (A
 * TX_HELD_REP packet's row is still to be found, and its code is final only then.) */
TX_HD bool txs_admit(const struct txs_seg *S, const struct txs_ready *r, bool held, uint32_t tag, int32_t *code, uint32_t *kind) {
  const uint32_t b = tx_block(&S->b, tag), esi = tag & 0xFFFFFFu;
  *kind = TX_READY;
  *code = 0;
  if (txs_is_ready(r, S->blk0 + b)) return true;
  if (held && tx_held_seen(&S->h, b, esi)) {
    *kind = esi < S->b.K ? TX_HELD_SRC : TX_HELD_REP;
    return true;
  }
  *code = TX_NOT_READY;
  return false;
}

/* the key as it lies in memory (network byte order), read as a little-endian word */
TX_HD uint32_t txs_key_word(uint32_t key) { return tx_header_word(key); }

/* one whole packet of any form from rows cols[0..n) of `base`, a byte at a time (the emulation; the kernels' byte path does the
 * same with a lane per byte, and every wider path must give these bytes) */
TX_HD void txs_emit_bytes(const uint8_t *base, const struct txs_call *c, uint32_t k, uint32_t key, uint32_t tag, const uint32_t *cols,
                          uint32_t n) {
  uint8_t *P = c->pkts + (uint64_t)k * c->pkt_stride;
  if (c->hdr == 8u) {
    const uint32_t h = txs_key_word(key);
    for (uint32_t j = 0; j < 4u; j++) P[j] = (uint8_t)(h >> (8u * j));
    P += 4;
  }
  if (c->hdr) {
    const uint32_t h = tx_header_word(tag);
    for (uint32_t j = 0; j < 4u; j++) P[j] = (uint8_t)(h >> (8u * j));
    P += 4;
  }
  for (uint32_t j = 0; j < c->T; j++) P[j] = tx_gather<uint8_t>(base, c->T, cols, n, j);
}

#endif /* NRQ_EMIT_SET_BODY_H */
