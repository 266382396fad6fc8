/* CPU emulation of a sender set's emit (emit_set_body.h): the same per-packet bodies the gfx950 kernels run, called in loops in
 * kernel order over a table of host arrays -- the search and the histogram per tile, the scan, the placement, then every work
 * item in block-major order: admit (with and without held symbols), column list, payload.  The payload is written a byte at a
 * time in every header form (none, FEC Payload ID, key + FEC Payload ID): what the kernels' byte path does, and what their
 * wider paths -- the 16-byte form under an 8-byte header among them -- must give.  As in held_emu.cpp the repair row lookup is
 * the sequential tx_held_find, where nrq_emit_set_kernel takes a ballot per wave; that wave-level code is covered by the GPU
 * tests (tests/test_gpu_txset.py).  Test support, not part of the library: build.build_txset_emu() makes
 * tests/emu/libtxset_emu.so of it. */
#include <stdint.h>
#include <string.h>

#include <vector>

#include "emit_set_body.h"

#define EMU_TILE 4096u /* TX_BIN_TILE: packets per workgroup of the bucketing passes */

extern "C" {

/* The set emit over nseg segments sorted by (key, sbn0).
 *   prm [nseg][8] = {K, K', T, nblk, sbn0, key, bm_words, rep_cap}
 *   ptr [nseg][9] = {src, src_stride, inter, inter_stride, seen, rep_esi, nrep, rep, rep_stride} (the last five 0 for a sender)
 *   ready [32]: a bit per global block; keys nullable (every key 0); hdr 0 / 4 / 8; held: NRQ_TX_HELD
 *   order_out nullable [n]: the work order the bucketing made
 * -1: a bad table; -2: the work order is not a permutation of the packets; -3: it is not block-major. */
int emu_txset_emit(uint32_t nseg, const uint32_t *prm, const uint64_t *ptr, const uint32_t *ready, const uint32_t *keys, const uint32_t *tags,
                   uint32_t n, uint32_t hdr, uint32_t held, uint8_t *pkts, uint64_t pkt_stride, int32_t *results, uint32_t *order_out) {
  if (nseg > TXS_MAX_SEGS || (hdr != 0u && hdr != 4u && hdr != 8u)) return -1;
  std::vector<txs_tab> tv(1);
  txs_tab &t = tv[0];
  memset(&t, 0, sizeof(t));
  t.nseg = nseg;
  uint32_t T = 0;
  for (uint32_t g = 0; g < nseg; g++) {
    const uint32_t *q = prm + 8u * g;
    const uint64_t *a = ptr + 9u * g;
    txs_seg &S = t.seg[g];
    tx_blk &b = S.b;
    if (!rq_params_init(q[1], &b.p) || b.p.Kp != q[1] || q[0] == 0 || q[0] > q[1]) return -1;
    b.p.K = q[0];
    b.K = q[0]; b.T = q[2]; b.nblk = q[3]; b.sbn0 = q[4];
    b.src = (const uint8_t *)(uintptr_t)a[0]; b.src_stride = a[1];
    b.inter = (const uint8_t *)(uintptr_t)a[2]; b.inter_stride = a[3];
    S.h.seen = (const uint32_t *)(uintptr_t)a[4]; S.h.rep_esi = (const uint32_t *)(uintptr_t)a[5];
    S.h.nrep = (const uint32_t *)(uintptr_t)a[6]; S.h.rep = (const uint8_t *)(uintptr_t)a[7]; S.h.rep_stride = a[8];
    S.h.bm_words = q[6]; S.h.rep_cap = q[7];
    S.key = q[5]; S.blk0 = t.nblk;
    t.key[g] = S.key; t.sbn0[g] = b.sbn0; t.cnt[g] = b.nblk; t.blk0[g] = S.blk0;
    t.nblk += b.nblk;
    if (g && b.T != T) return -1;
    T = b.T;
  }
  if (t.nblk > TXS_MAX_BLOCKS) return -1;
  txs_ready r;
  memcpy(r.w, ready, sizeof(r.w));
  std::vector<uint32_t> seg(n ? n : 1u), order(n ? n : 1u), cnt(t.nblk + 1u, 0);
  txs_call c;
  memset(&c, 0, sizeof(c));
  c.pkts = pkts; c.pkt_stride = pkt_stride; c.n = n; c.hdr = hdr; c.T = T;
  c.keys = keys; c.tags = tags; c.seg = seg.data(); c.order = order.data(); c.results = results;
  /* pass 1, per tile: the segment of every packet, and the packets per bucket */
  for (uint32_t k0 = 0; k0 < n; k0 += EMU_TILE)
    for (uint32_t k = k0; k < n && k < k0 + EMU_TILE; k++) {
      const uint32_t sg = txs_find(t.key, t.sbn0, t.cnt, t.nseg, txs_key_of(&c, k), tags[k] >> 24);
      c.seg[k] = sg;
      cnt[txs_bin(t.sbn0, t.blk0, t.nblk, sg, tags[k])]++;
    }
  /* pass 2: counts -> exclusive offsets */
  uint32_t run_ = 0;
  for (uint32_t b = 0; b <= t.nblk; b++) { const uint32_t v = cnt[b]; cnt[b] = run_; run_ += v; }
  /* pass 3: placement (the kernels place inside a bucket in any order) */
  for (uint32_t k = 0; k < n; k++) c.order[cnt[txs_bin(t.sbn0, t.blk0, t.nblk, c.seg[k], tags[k])]++] = k;
  if (order_out) memcpy(order_out, c.order, (size_t)n * 4u);
  /* pass 4: every work item in order */
  std::vector<uint8_t> hit(n ? n : 1u, 0);
  uint32_t cols[TX_COLS], last_bin = 0;
  for (uint32_t w = 0; w < n; w++) {
    const uint32_t k = c.order[w];
    if (k >= n || hit[k]++) return -2;
    const uint32_t tag = tags[k], key = txs_key_of(&c, k), sg = c.seg[k];
    const uint32_t bin = txs_bin(t.sbn0, t.blk0, t.nblk, sg, tag);
    if (bin < last_bin) return -3;
    last_bin = bin;
    if (sg == TXS_NONE) {
      if (results) results[k] = TX_FOREIGN;
      continue;
    }
    const txs_seg *S = &t.seg[sg];
    int32_t code;
    uint32_t kind, nc = 0;
    const uint8_t *base = nullptr;
    if (txs_admit(S, &r, held != 0, tag, &code, &kind)) {
      if (kind == TX_HELD_REP) { /* a copy of repair row q: one row from the row found */
        const uint32_t b = tx_block(&S->b, tag), q = tx_held_find(&S->h, b, tag & 0xFFFFFFu);
        code = q == TX_NONE ? TX_NOT_READY : 0;
        if (q != TX_NONE) {
          cols[0] = 0;
          nc = 1;
          base = tx_held_rep_base(&S->h, b) + (uint64_t)q * T;
        }
      } else {
        nc = tx_rows(&S->b, tag, cols);
        base = tx_base(&S->b, tag);
      }
    }
    if (results) results[k] = code;
    if (nc) txs_emit_bytes(base, &c, k, key, tag, cols, nc);
  }
  return 0;
}

} /* extern "C" */
