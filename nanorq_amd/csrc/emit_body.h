/*
 * emit_body.h -- the per-packet bodies of the device-resident sender (nrq_tx_*, include/nanorq_hip.h): packets -- an optional
 * 4-byte RFC 6330 FEC Payload ID and a payload at a packet stride -- written straight into device memory for a transmission of
 * nblk blocks of equal (K, K', T), SBNs sbn0 .. sbn0+nblk-1, whose intermediate symbols are already in device memory.
 *
 * Payload of (block b, ESI e), bit-exact with nanorq_encode (nanorq_api.c):
 *   e <  K   source row e of block b (the caller's rows)
 *   e >= K   LT(C_b, e + K' - K): the XOR of the intermediate symbols rq_lt_columns names
 * nrq_device.hip instantiates these bodies in its emit kernels; tests/emu/emit_emu.cpp runs them sequentially on the CPU.
 *
 * Work order.  A packet's repair gathers hit its block's L x T bytes of intermediate symbols; the kernels walk packets BLOCK-MAJOR
 * (work item w -> packet tx_work_packet(w)) so that a block's packets run together and its rows are served from the caches, in
 * whatever order the packets lie in the output.  emit_range maps analytically; a tag list is first bucketed by block
 * (tx_bin: one bucket per block, one more for foreign SBNs) into c->order.
 */
#ifndef NRQ_EMIT_BODY_H
#define NRQ_EMIT_BODY_H

#include <stdint.h>

#include "rq_math.h"

#if defined(__HIPCC__)
#define TX_HD __host__ __device__ __forceinline__
#else
#define TX_HD static inline
#endif

#define TX_NONE 0xFFFFFFFFu
#define TX_COLS 33u   /* room per packet for a column list: rq_lt_columns gives at most RQ_LT_COLS_MAX_REAL (odd: a lane's list
                       * in LDS starts on its own bank) */
#define TX_WAVE_PKTS 64u /* work items one wave takes: one per lane for the column lists, then one after the other for the payload */

/* the transmission (device addresses; the emulation passes host arrays) */
struct tx_blk {
  rq_params p;            /* of K' (p.K = K) */
  uint32_t K, T, nblk, sbn0;
  const uint8_t *src;     /* block b's source row e at src + b*src_stride + e*T */
  uint64_t src_stride;
  const uint8_t *inter;   /* block b's intermediate symbol i at inter + b*inter_stride + i*T */
  uint64_t inter_stride;
};

/* one emit call */
struct tx_call {
  uint8_t *pkts;          /* packet k at pkts + k*pkt_stride */
  uint64_t pkt_stride;
  uint32_t n;             /* packets (work items) */
  uint32_t inl;           /* 1: FEC Payload ID at +0, payload at +4 */
  const uint32_t *tags;   /* list mode: tag of packet k (nanorq_tag form); NULL: range mode */
  const uint32_t *order;  /* list mode: packet of work item w (bucketed by block) */
  int32_t *results;       /* list mode, nullable: 0 written, -1 SBN outside the transmission */
  uint32_t esi0, per_blk, interleave; /* range mode: per_blk ESIs esi0.. of every block; packet k -> (k % nblk, k / nblk) or
                                       * (k / per_blk, k % per_blk) */
  uint32_t *tags_out;     /* range mode, nullable: the tag of each packet */
};

TX_HD uint32_t tx_tag(uint32_t sbn, uint32_t esi) { return (sbn << 24) | esi; }

/* block of a tag inside the transmission, or TX_NONE */
TX_HD uint32_t tx_block(const struct tx_blk *t, uint32_t tag) {
  const uint32_t sbn = tag >> 24;
  return (sbn >= t->sbn0 && sbn - t->sbn0 < t->nblk) ? sbn - t->sbn0 : TX_NONE;
}

/* list mode bucket: the block, or nblk for a foreign SBN */
TX_HD uint32_t tx_bin(const struct tx_blk *t, uint32_t tag) {
  const uint32_t b = tx_block(t, tag);
  return b == TX_NONE ? t->nblk : b;
}

/* packet index of work item w */
TX_HD uint32_t tx_work_packet(const struct tx_blk *t, const struct tx_call *c, uint32_t w) {
  if (c->tags) return c->order[w];
  if (!c->interleave) return w;
  const uint32_t b = w / c->per_blk, i = w - b * c->per_blk;
  return i * t->nblk + b;
}

/* tag of packet k */
TX_HD uint32_t tx_packet_tag(const struct tx_blk *t, const struct tx_call *c, uint32_t k) {
  if (c->tags) return c->tags[k];
  uint32_t b, i;
  if (c->interleave) { i = k / t->nblk; b = k - i * t->nblk; }
  else { b = k / c->per_blk; i = k - b * c->per_blk; }
  return tx_tag(t->sbn0 + b, c->esi0 + i);
}

/* the rows a packet of `tag` (inside the transmission) is made of: the block's source rows or its intermediate symbols */
TX_HD const uint8_t *tx_base(const struct tx_blk *t, uint32_t tag) {
  const uint32_t b = tx_block(t, tag);
  return (tag & 0xFFFFFFu) < t->K ? t->src + (uint64_t)b * t->src_stride : t->inter + (uint64_t)b * t->inter_stride;
}

/* The rows whose XOR is the payload of `tag`, as indices (times T) from tx_base into cols[TX_COLS]; returns their count, 0 for
 * a foreign SBN. */
TX_HD uint32_t tx_rows(const struct tx_blk *t, uint32_t tag, uint32_t *cols) {
  const uint32_t esi = tag & 0xFFFFFFu;
  if (tx_block(t, tag) == TX_NONE) return 0;
  if (esi < t->K) {
    cols[0] = esi;
    return 1;
  }
  return rq_lt_columns(&t->p, esi + (t->p.Kp - t->K), cols);
}

/* the FEC Payload ID as it lies in memory (network byte order), read as a little-endian word */
TX_HD uint32_t tx_header_word(uint32_t tag) {
  return (tag >> 24) | ((tag >> 8) & 0xFF00u) | ((tag << 8) & 0xFF0000u) | (tag << 24);
}

/* XOR of the W-wide words at byte `off` of rows cols[0..n) (four loads in flight before they are combined) */
template <typename W>
TX_HD W tx_gather(const uint8_t *base, uint64_t T, const uint32_t *cols, uint32_t n, uint64_t off) {
  W acc = W();
  uint32_t i = 0;
  for (; i + 4u <= n; i += 4u) {
    const W a = *reinterpret_cast<const W *>(base + (uint64_t)cols[i] * T + off);
    const W b = *reinterpret_cast<const W *>(base + (uint64_t)cols[i + 1u] * T + off);
    const W c = *reinterpret_cast<const W *>(base + (uint64_t)cols[i + 2u] * T + off);
    const W d = *reinterpret_cast<const W *>(base + (uint64_t)cols[i + 3u] * T + off);
    acc = acc ^ a ^ b ^ c ^ d;
  }
  for (; i < n; i++) acc = acc ^ *reinterpret_cast<const W *>(base + (uint64_t)cols[i] * T + off);
  return acc;
}

/* 16 bytes as a value type both compilers treat alike */
struct alignas(16) tx_u128 {
  uint32_t x, y, z, w;
};
TX_HD tx_u128 operator^(tx_u128 a, tx_u128 b) { return tx_u128{a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w}; }

/* one whole packet, a byte at a time (the emulation; the kernels' byte path does the same with a lane per byte) */
TX_HD void tx_emit_bytes(const struct tx_blk *t, const struct tx_call *c, uint32_t k, uint32_t tag, const uint32_t *cols, uint32_t n) {
  const uint8_t *base = tx_base(t, tag);
  uint8_t *P = c->pkts + (uint64_t)k * c->pkt_stride;
  if (c->inl) {
    const uint32_t h = tx_header_word(tag);
    for (uint32_t j = 0; j < 4u; j++) P[j] = (uint8_t)(h >> (8u * j));
    P += 4;
  }
  for (uint32_t j = 0; j < t->T; j++) P[j] = tx_gather<uint8_t>(base, t->T, cols, n, j);
}

#endif /* NRQ_EMIT_BODY_H */
