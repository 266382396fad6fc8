/* CPU emulation of the emit and ingest of packets of several symbols (syms_body.h over emit_body.h and ingest_body.h): the same
 * bodies the gfx950 kernels run, called in loops in kernel order.  The payload is moved a byte at a time -- what the kernels' byte
 * paths do; their wider paths must give the same bytes.  Test support, not part of the library: build.build_syms_emu() makes
 * tests/emu/libsyms_emu.so of it.  It also exports the count rule, the range packetisation and the path rules, so that a test
 * asks them and does not restate them. */
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "emit_emu.h"
#include "syms_body.h"

/* every packet in work order; -2: the work order is not a permutation of the packets */
template <bool MULTI>
static int run_emit(const tx_src *s, const tx_call *c, const sy_tx *y) {
  std::vector<uint8_t> hit(c->n, 0);
  uint32_t cols[TX_COLS];
  for (uint32_t w = 0; w < c->n; w++) {
    const uint32_t k = tx_packet_of<MULTI>(s, c, w);
    if (k >= c->n || hit[k]++) return -2;
    uint32_t cnt;
    bool ranged;
    const uint32_t tag = sy_tx_packet<MULTI>(s, c, y, k, &cnt, &ranged);
    int32_t code;
    const uint32_t g = sy_tx_admit<MULTI>(s, y, tag, k, ranged, &code, &cnt);
    if (c->results) c->results[k] = code;
    if (c->tags_out) c->tags_out[k] = tag;
    if (y->nsym_out) y->nsym_out[k] = (uint8_t)cnt;
    if (g == TX_SEGS) continue;
    const tx_blk t = tx_pick(s, g);
    for (uint32_t i = 0; i < cnt; i++) { /* slot i: symbol 0 with the header as a one-symbol packet, the others behind it */
      const uint32_t n = tx_rows(&t, tag + i, cols);
      tx_call c1 = *c;
      if (i) { c1.pkts = c->pkts + (c->inl ? 4u : 0u) + (uint64_t)i * t.T; c1.inl = 0; }
      tx_emit_bytes(&t, &c1, k, tag + i, cols, n);
    }
  }
  return 0;
}

extern "C" {

uint32_t emu_sy_rule(uint32_t K, uint32_t e, uint32_t G) { return sy_rule(K, e, G); }
uint32_t emu_sy_pkt_count(uint32_t K, uint32_t esi0, uint32_t n, uint32_t G) { return sy_pkt_count(K, esi0, n, G); }
void emu_sy_range_pkt(uint32_t K, uint32_t esi0, uint32_t n, uint32_t G, uint32_t j, uint32_t *first, uint32_t *cnt) {
  sy_range_pkt(K, esi0, n, G, j, first, cnt);
}
uint32_t emu_sy_range_index(uint32_t K, uint32_t esi0, uint32_t n, uint32_t G, uint32_t e) { return sy_range_index(K, esi0, n, G, e); }
int emu_sy_emit_path(uint64_t al, uint32_t inl) { return tx_emit_path(al, inl, 0u); }
uint32_t emu_sy_copy_word(uint64_t al) { return sy_copy_word(al); }

/* The emit from a table of nseg segments (as emu_emit_table_ready of emit_emu.cpp): list mode when tags is not NULL (n first
 * tags, nsym nullable, results), else range mode with range = {esi0, eL, eS, interleave} (ESIs per block of each class; tags_out,
 * nsym_out nullable; *npkt_out = packets).  back_out (range mode, nullable): per packet the index found again from its block and
 * first ESI through sy_range_index and the inverse map.  pkts NULL (range mode): the maps only. */
int emu_sy_emit_table(const uint32_t *prm, uint32_t nseg, const uint32_t *span, const uint8_t *const *src, const uint64_t *src_stride,
                      const uint8_t *const *inter, const uint64_t *inter_stride, const uint32_t *tags, const uint8_t *nsym, uint32_t n,
                      uint32_t G, const uint32_t *range, uint32_t inl, uint8_t *pkts, uint64_t pkt_stride, int32_t *results,
                      uint32_t *tags_out, uint8_t *nsym_out, uint32_t *back_out, uint32_t *npkt_out, const uint32_t *ready) {
  tx_src s;
  if (G == 0 || G > SY_G_MAX || !emu_tx_table(&s, prm, nseg, span, src, src_stride, inter, inter_stride, ready)) return -1;
  tx_call c;
  memset(&c, 0, sizeof(c));
  sy_tx y;
  memset(&y, 0, sizeof(y));
  y.G = G;
  c.pkts = pkts; c.pkt_stride = pkt_stride; c.inl = inl;
  std::vector<uint32_t> order;
  if (tags) {
    order = emu_tx_bucket(&s, tags, n);
    c.n = n; c.tags = tags; c.order = order.data(); c.results = results;
    y.nsym = nsym;
  } else {
    /* (what the launcher does: packets per block of each class; a table of one class has its count in both) */
    const uint32_t KL = s.seg[0].K, KS = s.seg[nseg > 1u && s.ZL && s.Z > s.ZL ? 1u : 0u].K;
    uint32_t eL = range[1], eS = range[2];
    if (!s.ZL) eL = eS;
    c.esi0 = range[0]; c.interleave = range[3]; c.tags_out = tags_out;
    c.nL = sy_pkt_count(KL, c.esi0, eL, G);
    c.nS = s.Z > s.ZL ? sy_pkt_count(KS, c.esi0, eS, G) : c.nL;
    if (!s.ZL) c.nL = c.nS;
    c.n = s.ZL * c.nL + (s.Z - s.ZL) * c.nS;
    y.eL = eL; y.eS = eS; y.nsym_out = nsym_out;
    if (npkt_out) *npkt_out = c.n;
    if (back_out)
      for (uint32_t k = 0; k < c.n; k++) {
        uint32_t cnt;
        bool ranged;
        const uint32_t tag = nseg > 1u ? sy_tx_packet<true>(&s, &c, &y, k, &cnt, &ranged) : sy_tx_packet<false>(&s, &c, &y, k, &cnt, &ranged);
        const uint32_t b = (tag >> 24) - s.sbn0, small = nseg > 1u && b >= s.ZL;
        const uint32_t j = sy_range_index(small ? KS : KL, c.esi0, small ? eS : eL, G, tag & SY_ESI_MAX);
        if (c.interleave) back_out[k] = nseg > 1u ? tx_il_index<true>(&s, &c, b, j) : tx_il_index<false>(&s, &c, b, j);
        else back_out[k] = !small ? b * c.nL + j : s.ZL * c.nL + (b - s.ZL) * c.nS + j;
      }
    if (!pkts) {
      for (uint32_t k = 0; k < c.n; k++) {
        uint32_t cnt;
        bool ranged;
        const uint32_t tag = nseg > 1u ? sy_tx_packet<true>(&s, &c, &y, k, &cnt, &ranged) : sy_tx_packet<false>(&s, &c, &y, k, &cnt, &ranged);
        if (tags_out) tags_out[k] = tag;
        if (nsym_out) nsym_out[k] = (uint8_t)cnt;
      }
      return 0;
    }
  }
  return nseg > 1u ? run_emit<true>(&s, &c, &y) : run_emit<false>(&s, &c, &y);
}

/* The ingest of n packets of up to G symbols: prm = {K, T, nblk, sbn0, max_esi, rep_cap}; state arrays as struct ing_rx;
 * results[n * G].  -1: a slot's destination was left unwritten by the classify pass */
int emu_sy_rx_add(const uint32_t *prm, uint8_t *src, uint64_t src_stride, uint8_t *rep, uint64_t rep_stride, uint32_t *first, uint32_t *seen,
                  uint32_t *gaps, uint32_t *nrep, uint32_t *rep_esi, uint32_t *live, const uint8_t *pkts, uint64_t pkt_stride,
                  const uint32_t *tags, const uint8_t *nsym, uint32_t n, uint32_t G, int32_t *results) {
  ing_rx r;
  r.K = prm[0]; r.T = prm[1]; r.nblk = prm[2]; r.sbn0 = prm[3]; r.max_esi = prm[4]; r.rep_cap = prm[5];
  r.m1 = r.max_esi + 1u;
  r.bm_words = r.max_esi / 32u + 1u;
  r.src = src; r.src_stride = src_stride; r.rep = rep; r.rep_stride = rep_stride;
  r.first = first; r.seen = seen; r.gaps = gaps; r.nrep = nrep; r.rep_esi = rep_esi; r.live = live;
  if (n == 0) return 0;
  if (G == 0 || G > SY_G_MAX) return -1;
  const uint32_t ns = n * G;
  ing_call c;
  c.pkts = pkts; c.pkt_stride = pkt_stride; c.tags = tags; c.n = ns;
  c.ntiles = (ns + ING_TILE - 1u) / ING_TILE;
  std::vector<uint32_t> tagv(ns), fidx(ns), base((size_t)r.nblk * c.ntiles, 0), cnt(r.nblk);
  std::vector<uint8_t> kind(ns, 0xEE);
  const uint64_t poison = 0xDEADBEEFDEADBEEFull;
  std::vector<uint64_t> dst(ns, poison);
  c.tagv = tagv.data(); c.codes = results; c.fidx = fidx.data(); c.dst = dst.data(); c.base = base.data();
  sy_rx y;
  y.G = G; y.nsym = nsym; y.kind = kind.data();
  for (uint32_t s = 0; s < ns; s++) sy_first(&r, &c, &y, s); /* 1 */
  for (uint32_t b = 0; b < r.nblk; b++) {                    /* 2 */
    uint32_t mx = 0, ct = 0;
    if (r.gaps[b])
      for (uint32_t e = 0; e < r.K; e++) ing_done_part(&r, b, e, &mx, &ct);
    ing_done_finish(&r, b, mx, ct);
  }
  for (uint32_t s = 0; s < ns; s++) { /* 3 */
    const uint32_t b = sy_cand(&r, &c, &y, s);
    if (b != ING_NONE) base[(size_t)b * c.ntiles + s / ING_TILE]++;
  }
  for (uint32_t b = 0; b < r.nblk; b++) { /* 4 */
    uint32_t run = r.nrep[b];
    for (uint32_t t = 0; t < c.ntiles; t++) { const uint32_t v = base[(size_t)b * c.ntiles + t]; base[(size_t)b * c.ntiles + t] = run; run += v; }
    r.nrep[b] = std::min(run, r.rep_cap);
  }
  for (uint32_t t = 0; t < c.ntiles; t++) { /* 5 */
    std::fill(cnt.begin(), cnt.end(), 0u);
    const uint32_t s1 = std::min(ns, (t + 1u) * ING_TILE);
    std::vector<uint32_t> row(s1 - t * ING_TILE, ING_NONE);
    for (uint32_t s = t * ING_TILE; s < s1; s++) {
      const uint32_t b = sy_cand(&r, &c, &y, s);
      if (b != ING_NONE) row[s - t * ING_TILE] = base[(size_t)b * c.ntiles + t] + cnt[b]++;
    }
    for (uint32_t s = t * ING_TILE; s < s1; s++) sy_classify(&r, &c, &y, s, row[s - t * ING_TILE]);
  }
  const uint32_t off = ing_payload_off(&c);
  for (uint32_t s = 0; s < ns; s++) /* 6 */
    if (dst[s] == poison) return -1;
  for (uint32_t s = 0; s < ns; s++)
    if (dst[s]) memcpy((void *)(uintptr_t)dst[s], pkts + (size_t)(s / G) * pkt_stride + off + (size_t)(s % G) * r.T, r.T);
  for (uint32_t s = 0; s < ns; s++) sy_fold(&r, &c, &y, s); /* 7 */
  return 0;
}

} /* extern "C" */
