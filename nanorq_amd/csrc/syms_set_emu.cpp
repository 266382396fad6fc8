/* CPU emulation of a reception set's ingest and a sender set's emit of packets of several symbols (syms_set_body.h over
 * syms_body.h, ingest_set_body.h and emit_set_body.h): the same bodies the gfx950 kernels run, called in loops in kernel order, as
 * rxset_emu.cpp, txset_emu.cpp and syms_emu.cpp do for the layers below.  The emit writes a byte at a time in all three header
 * forms: what every wider path -- the 16-byte walk of a run under the 8-byte header among them -- must give.  Test support, not
 * part of the library: build.build_syms_set_emu() makes tests/emu/libsyms_set_emu.so of it.  It also exports the path rule of the
 * set's emit and the word rule of the set's copy, so that a test asks them and does not restate them. */
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "syms_set_body.h"

#define EMU_TILE 4096u /* TX_BIN_TILE: packets per workgroup of the bucketing passes */

extern "C" {

int emu_sys_emit_path(uint64_t al, uint32_t hdr) { return sys_emit_path(al, hdr, 0u); }
uint32_t emu_sys_copy_word(uint64_t al) { return sy_copy_word(al); }

/* The set ingest of n packets of up to G symbols; members, prm, ptr, keys, tags, key_inline as emu_rxset_add (rxset_emu.cpp), nsym
 * nullable, results[n * G].  0, or -1: a slot's destination was left unwritten by the classify pass, -2: a bad table or G */
int emu_sys_rxset_add(uint32_t nmem, const uint32_t *prm, const uint64_t *ptr, const uint8_t *pkts, uint64_t pkt_stride, const uint32_t *keys,
                      const uint32_t *tags, uint32_t key_inline, const uint8_t *nsym, uint32_t n, uint32_t G, int32_t *results) {
  if (nmem > INGS_MAX_MEMBERS || G == 0 || G > SY_G_MAX) return -2;
  std::vector<uint32_t> order(nmem);
  std::iota(order.begin(), order.end(), 0u);
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    const uint32_t *pa = prm + 8u * a, *pb = prm + 8u * b;
    return pa[6] != pb[6] ? pa[6] < pb[6] : pa[3] < pb[3];
  });
  std::vector<ings_tab> tabv(1);
  ings_tab &t = tabv[0];
  memset(&t, 0, sizeof(t));
  t.nmem = nmem;
  for (uint32_t i = 0; i < nmem; i++) {
    const uint32_t *p = prm + 8u * order[i];
    const uint64_t *q = ptr + 8u * order[i];
    ing_rx &r = t.r[i];
    r.K = p[0]; r.T = p[1]; r.nblk = p[2]; r.sbn0 = p[3]; r.max_esi = p[4]; r.rep_cap = p[5];
    r.m1 = r.max_esi + 1u;
    r.bm_words = r.max_esi / 32u + 1u;
    r.src = (uint8_t *)(uintptr_t)q[0]; r.src_stride = (uint64_t)r.K * r.T;
    r.rep = (uint8_t *)(uintptr_t)q[1]; r.rep_stride = (uint64_t)r.rep_cap * r.T;
    r.first = (uint32_t *)(uintptr_t)q[2]; r.seen = (uint32_t *)(uintptr_t)q[3]; r.gaps = (uint32_t *)(uintptr_t)q[4];
    r.nrep = (uint32_t *)(uintptr_t)q[5]; r.rep_esi = (uint32_t *)(uintptr_t)q[6]; r.live = (uint32_t *)(uintptr_t)q[7];
    t.key[i] = p[6]; t.sbn0[i] = r.sbn0; t.cnt[i] = r.nblk; t.objZ[i] = p[7];
    t.blk0[i] = t.nblk;
    t.nblk += r.nblk;
  }
  t.blk0[nmem] = t.nblk;
  if (t.nblk > INGS_MAX_BLOCKS) return -2;
  if (n == 0 || nmem == 0) return 0;
  const uint32_t T = t.r[0].T, ns = n * G;
  ings_call s;
  ing_call &c = s.c;
  c.pkts = pkts; c.pkt_stride = pkt_stride; c.tags = tags; c.n = ns;
  c.ntiles = (ns + ING_TILE - 1u) / ING_TILE;
  s.keys = keys;
  s.key_inline = key_inline;
  std::vector<uint32_t> tagv(ns), mem(n, 0xEEEEEEEEu), fidx(ns), base((size_t)t.nblk * c.ntiles, 0), cnt(t.nblk);
  std::vector<uint8_t> kind(ns, 0xEE);
  const uint64_t poison = 0xDEADBEEFDEADBEEFull; /* (every entry pass 6 reads must have been written by pass 5) */
  std::vector<uint64_t> dst(ns, poison);
  c.tagv = tagv.data(); c.codes = results; c.fidx = fidx.data(); c.dst = dst.data(); c.base = base.data();
  s.mem = mem.data();
  sy_rx y;
  y.G = G; y.nsym = nsym; y.kind = kind.data();
  for (uint32_t sl = 0; sl < ns; sl++) { /* 1 */
    uint32_t key, tag;
    ings_decode(&s, sl / G, &key, &tag);
    sys_first(&t, &s, &y, sl, tag, ings_find(t.key, t.sbn0, t.cnt, t.objZ, t.nmem, key, tag >> 24));
  }
  for (uint32_t g = 0; g < t.nblk; g++) { /* 2 */
    const uint32_t m = ings_member_of_block(t.blk0, t.nmem, g), b = g - t.blk0[m];
    const ing_rx *r = &t.r[m];
    uint32_t mx = 0, ct = 0;
    if (r->gaps[b])
      for (uint32_t e = 0; e < r->K; e++) ing_done_part(r, b, e, &mx, &ct);
    ing_done_finish(r, b, mx, ct);
  }
  for (uint32_t sl = 0; sl < ns; sl++) { /* 3 */
    const uint32_t g = sys_cand(&t, &s, &y, sl);
    if (g != ING_NONE) base[(size_t)g * c.ntiles + sl / ING_TILE]++;
  }
  for (uint32_t g = 0; g < t.nblk; g++) { /* 4 */
    const uint32_t m = ings_member_of_block(t.blk0, t.nmem, g), b = g - t.blk0[m];
    const ing_rx *r = &t.r[m];
    uint32_t run = r->nrep[b];
    for (uint32_t i = 0; i < c.ntiles; i++) { const uint32_t v = base[(size_t)g * c.ntiles + i]; base[(size_t)g * c.ntiles + i] = run; run += v; }
    r->nrep[b] = std::min(run, r->rep_cap);
  }
  for (uint32_t i = 0; i < c.ntiles; i++) { /* 5 */
    std::fill(cnt.begin(), cnt.end(), 0u);
    const uint32_t s0 = i * ING_TILE, s1 = std::min(ns, s0 + ING_TILE);
    std::vector<uint32_t> row(s1 - s0, ING_NONE);
    for (uint32_t sl = s0; sl < s1; sl++) { /* (all candidates are found before any slot is classified, as in the kernel) */
      const uint32_t g = sys_cand(&t, &s, &y, sl);
      if (g != ING_NONE) row[sl - s0] = base[(size_t)g * c.ntiles + i] + cnt[g]++;
    }
    for (uint32_t sl = s0; sl < s1; sl++) sys_classify(&t, &s, &y, sl, row[sl - s0]);
  }
  const uint32_t off = ings_payload_off(&s);
  for (uint32_t sl = 0; sl < ns; sl++) /* 6 */
    if (dst[sl] == poison) return -1;
  for (uint32_t sl = 0; sl < ns; sl++)
    if (dst[sl]) memcpy((void *)(uintptr_t)dst[sl], pkts + (size_t)(sl / G) * pkt_stride + off + (size_t)(sl % G) * T, T);
  for (uint32_t sl = 0; sl < ns; sl++) sys_fold(&t, &s, &y, sl); /* 7 */
  return 0;
}

/* The set emit of n packets of up to G symbols over nseg segments sorted by (key, sbn0); prm, ptr, ready, keys, hdr, order_out as
 * emu_txset_emit (txset_emu.cpp; the held columns are not read), tags the first tags, nsym nullable.
 * -1: a bad table or G; -2: the work order is not a permutation of the packets; -3: it is not block-major. */
int emu_sys_txset_emit(uint32_t nseg, const uint32_t *prm, const uint64_t *ptr, const uint32_t *ready, const uint32_t *keys,
                       const uint32_t *tags, const uint8_t *nsym, uint32_t n, uint32_t G, uint32_t hdr, uint8_t *pkts, uint64_t pkt_stride,
                       int32_t *results, uint32_t *order_out) {
  if (nseg > TXS_MAX_SEGS || (hdr != 0u && hdr != 4u && hdr != 8u) || G == 0 || G > SY_G_MAX) return -1;
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
  sy_tx y;
  memset(&y, 0, sizeof(y));
  y.G = G; y.nsym = nsym;
  /* the bucketing passes over the first tags, per tile: segment and bucket of every packet, offsets, placement */
  for (uint32_t k0 = 0; k0 < n; k0 += EMU_TILE)
    for (uint32_t k = k0; k < n && k < k0 + EMU_TILE; k++) {
      const uint32_t sg = txs_find(t.key, t.sbn0, t.cnt, t.nseg, txs_key_of(&c, k), tags[k] >> 24);
      c.seg[k] = sg;
      cnt[txs_bin(t.sbn0, t.blk0, t.nblk, sg, tags[k])]++;
    }
  uint32_t run_ = 0;
  for (uint32_t b = 0; b <= t.nblk; b++) { const uint32_t v = cnt[b]; cnt[b] = run_; run_ += v; }
  for (uint32_t k = 0; k < n; k++) c.order[cnt[txs_bin(t.sbn0, t.blk0, t.nblk, c.seg[k], tags[k])]++] = k;
  if (order_out) memcpy(order_out, c.order, (size_t)n * 4u);
  /* every packet in work order */
  std::vector<uint8_t> hit(n ? n : 1u, 0);
  uint32_t last_bin = 0;
  for (uint32_t w = 0; w < n; w++) {
    const uint32_t k = c.order[w];
    if (k >= n || hit[k]++) return -2;
    const uint32_t tag = tags[k], sg = c.seg[k];
    const uint32_t bin = txs_bin(t.sbn0, t.blk0, t.nblk, sg, tag);
    if (bin < last_bin) return -3;
    last_bin = bin;
    int32_t code;
    uint32_t pc;
    const bool ok = sys_tx_admit(&t, &r, &y, k, tag, sg, &code, &pc);
    if (results) results[k] = code;
    if (ok) sys_emit_bytes(&t.seg[sg], &c, k, txs_key_of(&c, k), tag, pc);
  }
  return 0;
}

} /* extern "C" */
