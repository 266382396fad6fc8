/* CPU emulation of the want and held listings as runs (nrq_rx_want_syms / nrq_rx_held_syms) and of the held emit of packets of
 * several symbols (NRQ_TX_HELD in nrq_tx_emit_syms), over runs_body.h.  The listings run in the rounds of the gfx950 kernels:
 * WN_ROUND words (rows) per round, one per "thread", the workgroup's sum-scan and max-scan done in loops, the run start, the symbols
 * found and the packets placed carried from round to round; the per-word and per-row bodies are the ones the kernels run.  The held
 * emit runs the kernel's admission (hs_packet, hs_slot_held; the ballot over a packet's lanes is a loop over its slots) and its walk
 * over the block's repair list in trips of 64 entries, and moves the payload a byte at a time; the wave-level code -- ballots,
 * the row indices handed through LDS, the wider payload paths -- is covered by the byte-exact GPU tests only
 * (tests/test_gpu_runs.py).  Test support, not part of the library: build.build_runs_emu() makes tests/emu/libruns_emu.so of it. */
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "emit_emu.h"
#include "runs_body.h"
#include "runs_emu_walks.h"

static ing_rx books(const uint32_t *prm, const uint32_t *seen, const uint32_t *gaps, const uint32_t *nrep, const uint32_t *rep_esi) {
  ing_rx r;
  memset(&r, 0, sizeof(r));
  r.K = prm[0]; r.nblk = prm[1]; r.sbn0 = prm[2]; r.max_esi = prm[3]; r.rep_cap = prm[4];
  r.m1 = r.max_esi + 1u;
  r.bm_words = r.max_esi / 32u + 1u;
  r.seen = const_cast<uint32_t *>(seen); r.gaps = const_cast<uint32_t *>(gaps); r.nrep = const_cast<uint32_t *>(nrep);
  r.rep_esi = const_cast<uint32_t *>(rep_esi);
  return r;
}

/* what rn_check of nrq_device.hip refuses */
static bool refused(uint32_t G, const uint32_t *tags, const uint8_t *nsym, uint32_t *npkt, uint32_t *nsym_total) {
  if (!npkt) return true;
  *npkt = 0;
  if (nsym_total) *nsym_total = 0;
  return G == 0 || G > SY_G_MAX || !tags != !nsym;
}

/* the held emit, every packet in work order as nrq_emit_held_syms_kernel; -2: the work order is not a permutation of the packets */
template <bool MULTI>
static int run_held_syms(const tx_src *s, const tx_held *h, const tx_call *c, const sy_tx *y) {
  std::vector<uint8_t> hit(c->n, 0);
  uint32_t cols[TX_COLS], rows[SY_G_MAX];
  for (uint32_t w = 0; w < c->n; w++) {
    const uint32_t k = c->order[w];
    if (k >= c->n || hit[k]++) return -2;
    const uint32_t tag = c->tags[k], e = tag & SY_ESI_MAX;
    int32_t code;
    uint32_t cnt, ready;
    uint32_t g = hs_packet<MULTI>(s, y, tag, k, &code, &cnt, &ready);
    uint32_t kind = TX_READY, b = 0;
    tx_blk t = tx_pick(s, g);
    tx_held_seg hs = tx_held_pick(h, g);
    if (g < TX_SEGS && !ready) {
      b = tx_block(&t, tag);
      bool all = true;
      for (uint32_t i = 0; i < cnt; i++) all = all && hs_slot_held(&hs, b, e + i); /* (the ballot over the packet's lanes) */
      if (!all) { code = TX_NOT_READY; g = TX_SEGS; }
      else kind = e < t.K ? TX_HELD_SRC : TX_HELD_REP;
    }
    if (g < TX_SEGS && kind == TX_HELD_REP) { /* the wave's walk over the block's repair list, 64 entries a trip */
      const uint32_t nrep = tx_held_nrep(&hs, b);
      for (uint32_t i = 0; i < cnt; i++) rows[i] = TX_NONE;
      for (uint32_t q0 = 0; q0 < nrep; q0 += 64u)
        for (uint32_t lane = 0; lane < 64u && q0 + lane < nrep; lane++) {
          const uint32_t x = hs.rep_esi[(uint64_t)b * hs.rep_cap + q0 + lane] - e;
          if (x < cnt) rows[x] = q0 + lane;
        }
      for (uint32_t i = 0; i < cnt; i++)
        if (rows[i] == TX_NONE) { code = TX_NOT_READY; g = TX_SEGS; }
    }
    if (c->results) c->results[k] = code;
    if (g == TX_SEGS) continue;
    for (uint32_t i = 0; i < cnt; i++) { /* slot i: symbol 0 with the header as a one-symbol packet, the others behind it */
      tx_blk ti = t;
      uint32_t n;
      if (kind == TX_HELD_REP) { /* (tx_base picks `inter` for an ESI >= K: point it at the row found, block stride 0) */
        ti.inter = tx_held_rep_base(&hs, b) + (uint64_t)rows[i] * t.T;
        ti.inter_stride = 0;
        cols[0] = 0;
        n = 1u;
      } else {
        n = tx_rows(&ti, tag + i, cols);
      }
      tx_call c1 = *c;
      if (i) { c1.pkts = c->pkts + (c->inl ? 4u : 0u) + (uint64_t)i * t.T; c1.inl = 0; }
      tx_emit_bytes(&ti, &c1, k, tag + i, cols, n);
    }
  }
  return 0;
}

extern "C" {

/* The want listing of one reception in packets of up to G symbols: prm = {K, nblk, sbn0, max_esi, rep_cap}; the count pass, the
 * scan over the blocks, the fill pass.  *npkt = packets, *nsym_total (nullable) = symbols; tags and nsym (both, or neither)
 * receive the packets when cap >= *npkt, else -1 and nothing written.  -1 too for what the call refuses. */
int emu_rx_want_syms(const uint32_t *prm, const uint32_t *seen, const uint32_t *gaps, const uint32_t *nrep, uint32_t flags, uint32_t extra,
                     uint32_t esi_from, uint32_t G, uint32_t *tags, uint8_t *nsym, uint32_t cap, uint32_t *npkt, uint32_t *nsym_total) {
  if (refused(G, tags, nsym, npkt, nsym_total)) return -1;
  if (wn_check(flags, extra, esi_from)) return -1;
  const ing_rx r = books(prm, seen, gaps, nrep, nullptr);
  const wn_q q = wn_query(&r, flags, extra, esi_from);
  std::vector<uint32_t> off(r.nblk + 1u, 0);
  uint32_t total = 0;
  for (uint32_t b = 0; b < r.nblk; b++) { /* count */
    const rn_walk k = rn_walk_want(&r, &q, b);
    uint32_t syms;
    off[b] = bits_walk(&r, &k, G, nullptr, nullptr, 0u, &syms);
    total += syms;
  }
  uint32_t run = 0; /* scan */
  for (uint32_t b = 0; b <= r.nblk; b++) { const uint32_t v = off[b]; off[b] = run; run += v; }
  *npkt = off[r.nblk];
  if (nsym_total) *nsym_total = total;
  if (!tags) return 0;
  if (cap < *npkt) return -1;
  for (uint32_t b = 0; b < r.nblk; b++) { /* fill */
    const rn_walk k = rn_walk_want(&r, &q, b);
    if (bits_walk(&r, &k, G, tags, nsym, off[b], nullptr) != off[b + 1u]) return -3; /* (the passes disagree) */
  }
  return 0;
}

/* The held listing of one reception in packets of up to G symbols; as emu_rx_want_syms. */
int emu_rx_held_syms(const uint32_t *prm, const uint32_t *seen, const uint32_t *nrep, const uint32_t *rep_esi, uint32_t G, uint32_t *tags,
                     uint8_t *nsym, uint32_t cap, uint32_t *npkt, uint32_t *nsym_total) {
  if (refused(G, tags, nsym, npkt, nsym_total)) return -1;
  const ing_rx r = books(prm, seen, nullptr, nrep, rep_esi);
  std::vector<uint32_t> off(r.nblk + 1u, 0);
  uint32_t total = 0;
  for (uint32_t b = 0; b < r.nblk; b++) { /* count */
    const rn_walk k = rn_walk_held(&r, b);
    uint32_t syms;
    off[b] = bits_walk(&r, &k, G, nullptr, nullptr, 0u, &syms) + rows_walk(&r, b, G, nullptr, nullptr, 0u);
    total += syms + hl_nrep(&r, b);
  }
  uint32_t run = 0; /* scan */
  for (uint32_t b = 0; b <= r.nblk; b++) { const uint32_t v = off[b]; off[b] = run; run += v; }
  *npkt = off[r.nblk];
  if (nsym_total) *nsym_total = total;
  if (!tags) return 0;
  if (cap < *npkt) return -1;
  for (uint32_t b = 0; b < r.nblk; b++) { /* fill */
    const rn_walk k = rn_walk_held(&r, b);
    const uint32_t at = bits_walk(&r, &k, G, tags, nsym, off[b], nullptr);
    if (at == RN_ALL || rows_walk(&r, b, G, tags, nsym, at) != off[b + 1u]) return -3; /* (the passes disagree) */
  }
  return 0;
}

/* The tag-list emit of packets of up to G symbols of a relay with NRQ_TX_HELD: the tables as emu_emit_held (held_emu.cpp), n first
 * tags, nsym nullable (the sender's rule).  -1: a bad table or G. */
int emu_emit_held_syms(const uint32_t *prm, uint32_t nseg, const uint32_t *span, const uint8_t *const *src, const uint64_t *src_stride,
                       const uint8_t *const *inter, const uint64_t *inter_stride, const uint32_t *ready, const uint32_t *const *seen,
                       const uint32_t *bm_words, const uint32_t *const *rep_esi, const uint32_t *const *nrep, const uint32_t *rep_cap,
                       const uint8_t *const *rep, const uint64_t *rep_stride, const uint32_t *tags, const uint8_t *nsym, uint32_t n, uint32_t G,
                       uint32_t inl, uint8_t *pkts, uint64_t pkt_stride, int32_t *results) {
  tx_src s;
  tx_held h;
  memset(&h, 0, sizeof(h));
  if (G == 0 || G > SY_G_MAX || !tags || !emu_tx_table(&s, prm, nseg, span, src, src_stride, inter, inter_stride, ready)) return -1;
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
  sy_tx y;
  memset(&y, 0, sizeof(y));
  y.G = G; y.nsym = nsym;
  return nseg > 1u ? run_held_syms<true>(&s, &h, &c, &y) : run_held_syms<false>(&s, &h, &c, &y);
}

} /* extern "C" */
