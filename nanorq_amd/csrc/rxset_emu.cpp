/* CPU emulation of a reception set's ingest (ingest_set_body.h over ingest_body.h): the same per-packet and per-block bodies the
 * gfx950 kernels run (nrq_ings_*_kernel, nrq_device.hip), called in loops in kernel order.  As in tests/emu/ingest_emu.cpp the
 * one piece the kernels do with wave ballots -- a repair candidate's rank among its block's candidates in its tile -- is a
 * counter per global block over the tile in packet order here. */
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "ingest_set_body.h"

extern "C" {

/* nmem members in any order (sorted here by (key, sbn0), as the library's host side does):
 *   prm[m] = {K, T, nblk, sbn0, max_esi, rep_cap, key, objZ}
 *   ptr[m] = {src, rep, first, seen, gaps, nrep, rep_esi, live} (host addresses; src_stride K*T, rep_stride rep_cap*T)
 * keys / tags nullable as in nrq_rxset_add (tags NULL: inline; key_inline: key, FEC Payload ID, payload at +8).
 * results[n] receives the codes.  0, or -1: a packet's destination was left unwritten by the classify pass, -2: a bad table */
int emu_rxset_add(uint32_t nmem, const uint32_t *prm, const uint64_t *ptr, const uint8_t *pkts, uint64_t pkt_stride, const uint32_t *keys,
                  const uint32_t *tags, uint32_t key_inline, uint32_t n, int32_t *results) {
  if (nmem > INGS_MAX_MEMBERS) return -2;
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
  const uint32_t T = t.r[0].T;
  ings_call s;
  ing_call &c = s.c;
  c.pkts = pkts; c.pkt_stride = pkt_stride; c.tags = tags; c.n = n;
  c.ntiles = (n + ING_TILE - 1u) / ING_TILE;
  s.keys = keys;
  s.key_inline = key_inline;
  std::vector<uint32_t> tagv(n), mem(n), fidx(n), base((size_t)t.nblk * c.ntiles, 0), cnt(t.nblk);
  const uint64_t poison = 0xDEADBEEFDEADBEEFull; /* the device's per-call scratch holds whatever the last user left: every entry pass 6
                                                  * reads must have been written by pass 5 */
  std::vector<uint64_t> dst(n, poison);
  c.tagv = tagv.data(); c.codes = results; c.fidx = fidx.data(); c.dst = dst.data(); c.base = base.data();
  s.mem = mem.data();
  for (uint32_t k = 0; k < n; k++) { /* 1 */
    uint32_t key, tag;
    ings_decode(&s, k, &key, &tag);
    ings_first(&t, &s, k, tag, ings_find(t.key, t.sbn0, t.cnt, t.objZ, t.nmem, key, tag >> 24));
  }
  for (uint32_t g = 0; g < t.nblk; g++) { /* 2 */
    const uint32_t m = ings_member_of_block(t.blk0, t.nmem, g), b = g - t.blk0[m];
    const ing_rx *r = &t.r[m];
    uint32_t mx = 0, ct = 0;
    if (r->gaps[b])
      for (uint32_t e = 0; e < r->K; e++) ing_done_part(r, b, e, &mx, &ct);
    ing_done_finish(r, b, mx, ct);
  }
  for (uint32_t k = 0; k < n; k++) { /* 3 */
    const uint32_t g = ings_cand(&t, &s, k);
    if (g != ING_NONE) base[(size_t)g * c.ntiles + k / ING_TILE]++;
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
    const uint32_t k0 = i * ING_TILE, k1 = std::min(n, k0 + ING_TILE);
    std::vector<uint32_t> row(k1 - k0, ING_NONE);
    for (uint32_t k = k0; k < k1; k++) { /* (all candidates are found before any packet is classified, as in the kernel) */
      const uint32_t g = ings_cand(&t, &s, k);
      if (g != ING_NONE) row[k - k0] = base[(size_t)g * c.ntiles + i] + cnt[g]++;
    }
    for (uint32_t k = k0; k < k1; k++) ings_classify(&t, &s, k, row[k - k0]);
  }
  const uint32_t off = ings_payload_off(&s);
  for (uint32_t k = 0; k < n; k++) /* 6 */
    if (dst[k] == poison) return -1;
  for (uint32_t k = 0; k < n; k++)
    if (dst[k]) memcpy((void *)(uintptr_t)dst[k], pkts + (size_t)k * pkt_stride + off, T);
  for (uint32_t k = 0; k < n; k++) ings_fold(&t, &s, k); /* 7 */
  return 0;
}

} /* extern "C" */
