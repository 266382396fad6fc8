/* CPU emulation of the held-symbol emit (NRQ_TX_HELD: tx_admit_held and the repair row lookup of emit_body.h) and of the listing
 * of what a reception holds (held_body.h), called in loops in the kernels' work order.  The admit step, the payload paths and the
 * listing bodies are the ones the gfx950 kernels run.  The repair row lookup is NOT: here it is the sequential tx_held_find, while
 * nrq_emit_held_kernel does it per wave (each lane probes rep_esi[b][q0 + lane], a ballot and a find-first give the row, the
 * result is written after the trips, n and kind travel packed through a readfirstlane) and picks the row's base itself; that
 * wave-level code is covered by the byte-exact GPU tests only (tests/test_gpu_held.py).  Test support, not part of the library:
 * build.build_held_emu() makes tests/emu/libheld_emu.so of it.  The table set-up and the bucketing are emit_emu.h's, shared with the
 * plain emit's emulation (emit_emu.cpp). */
#include <stdint.h>
#include <string.h>

#include <vector>

#include "emit_emu.h"
#include "held_body.h"

/* every work item in order, as nrq_emit_held_kernel; -2: the work order is not a permutation of the packets */
template <bool MULTI>
static int run_held(const tx_src *s, const tx_held *h, const tx_call *c) {
  std::vector<uint8_t> hit(c->n, 0);
  uint32_t cols[TX_COLS];
  for (uint32_t w = 0; w < c->n; w++) {
    const uint32_t k = tx_packet_of<MULTI>(s, c, w);
    if (k >= c->n || hit[k]++) return -2;
    const uint32_t tag = tx_tag_of<MULTI>(s, c, k);
    int32_t code;
    uint32_t kind;
    const uint32_t g = tx_admit_held<MULTI>(s, h, tag, &code, &kind);
    if (g == TX_SEGS) {
      if (c->results) c->results[k] = code;
      continue;
    }
    tx_blk t = tx_pick(s, g);
    uint32_t n;
    if (kind == TX_HELD_REP) {
      /* a copy of repair row q: one row from the base of the block's repair rows, through the same payload path */
      const tx_held_seg hs = tx_held_pick(h, g);
      const uint32_t b = tx_block(&t, tag), q = tx_held_find(&hs, b, tag & 0xFFFFFFu);
      code = q == TX_NONE ? TX_NOT_READY : 0;
      n = q == TX_NONE ? 0u : 1u;
      cols[0] = 0;
      /* (tx_base picks `inter` for an ESI >= K: point it at the row found, block stride 0) */
      t.inter = tx_held_rep_base(&hs, b) + (uint64_t)q * t.T;
      t.inter_stride = 0;
    } else {
      n = tx_rows(&t, tag, cols);
    }
    if (c->results) c->results[k] = code;
    if (n) tx_emit_bytes(&t, c, k, tag, cols, n);
  }
  return 0;
}

extern "C" {

/* The tag-list emit of a relay with NRQ_TX_HELD.  The source table as emu_emit_table_ready (prm = nseg x {K, K', T, nblk, sbn0},
 * span = {sbn0, Z, ZL}, ready = 8 words); the held table per segment: the reception's seen bitmap ([nblk][bm_words]), repair ESI
 * list ([nblk][rep_cap]), repair rows used ([nblk]) and repair rows (rep, rep_stride).  -1: a bad table. */
int emu_emit_held(const uint32_t *prm, uint32_t nseg, const uint32_t *span, const uint8_t *const *src, const uint64_t *src_stride,
                  const uint8_t *const *inter, const uint64_t *inter_stride, const uint32_t *ready, const uint32_t *const *seen,
                  const uint32_t *bm_words, const uint32_t *const *rep_esi, const uint32_t *const *nrep, const uint32_t *rep_cap,
                  const uint8_t *const *rep, const uint64_t *rep_stride, const uint32_t *tags, uint32_t n, uint32_t inl, uint8_t *pkts,
                  uint64_t pkt_stride, int32_t *results) {
  tx_src s;
  tx_held h;
  memset(&h, 0, sizeof(h));
  if (!tags || !emu_tx_table(&s, prm, nseg, span, src, src_stride, inter, inter_stride, ready)) return -1;
  for (uint32_t g = 0; g < nseg; g++) {
    tx_held_seg &hs = h.seg[g];
    hs.seen = seen[g]; hs.bm_words = bm_words[g]; hs.rep_esi = rep_esi[g]; hs.nrep = nrep[g]; hs.rep_cap = rep_cap[g];
    hs.rep = rep[g]; hs.rep_stride = rep_stride[g];
  }
  tx_call c;
  memset(&c, 0, sizeof(c));
  c.pkts = pkts; c.pkt_stride = pkt_stride; c.inl = inl;
  const std::vector<uint32_t> order = emu_tx_bucket(&s, tags, n);
  c.n = n; c.tags = tags; c.order = order.data(); c.results = results;
  return nseg > 1u ? run_held<true>(&s, &h, &c) : run_held<false>(&s, &h, &c);
}

/* The listing of one reception: prm = {K, nblk, sbn0, max_esi, rep_cap}; the count pass, the scan over the blocks, the fill pass.
 * *n = symbols held; out (nullable) receives the tags when cap >= *n, else -1. */
int emu_rx_held(const uint32_t *prm, const uint32_t *seen, const uint32_t *nrep, const uint32_t *rep_esi, uint32_t *out, uint32_t cap,
                uint32_t *n) {
  ing_rx r;
  memset(&r, 0, sizeof(r));
  r.K = prm[0]; r.nblk = prm[1]; r.sbn0 = prm[2]; r.max_esi = prm[3]; r.rep_cap = prm[4];
  r.m1 = r.max_esi + 1u;
  r.bm_words = r.max_esi / 32u + 1u;
  r.seen = const_cast<uint32_t *>(seen); r.nrep = const_cast<uint32_t *>(nrep); r.rep_esi = const_cast<uint32_t *>(rep_esi);
  std::vector<uint32_t> off(r.nblk + 1u, 0);
  for (uint32_t b = 0; b < r.nblk; b++) { /* count */
    uint32_t c = hl_nrep(&r, b);
    for (uint32_t w = 0; w < ing_src_words(&r); w++) c += ing_popc(hl_have(&r, b, w));
    off[b] = c;
  }
  uint32_t run_ = 0; /* scan */
  for (uint32_t b = 0; b <= r.nblk; b++) { const uint32_t v = off[b]; off[b] = run_; run_ += v; }
  *n = off[r.nblk];
  if (!out) return 0;
  if (cap < *n) return -1;
  for (uint32_t b = 0; b < r.nblk; b++) { /* fill */
    uint32_t o = off[b];
    for (uint32_t w = 0; w < ing_src_words(&r); w++) o += hl_put(&r, b, w, hl_have(&r, b, w), out + o);
    for (uint32_t q = 0; q < hl_nrep(&r, b); q++) out[o + q] = hl_rep_tag(&r, b, q);
  }
  return 0;
}

} /* extern "C" */
