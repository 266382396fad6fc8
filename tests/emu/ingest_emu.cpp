/* CPU emulation of the device-resident receiver's ingest (nanorq_amd/csrc/ingest_body.h): the same per-packet and per-block
 * bodies the gfx950 kernels run, called in loops in kernel order.  The one piece the kernels do with wave ballots -- a repair
 * candidate's rank among its block's candidates in its tile -- is a per-block counter over the tile in packet order here. */
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../nanorq_amd/csrc/ingest_body.h"

extern "C" {

/* prm = {K, T, nblk, sbn0, max_esi, rep_cap}; state arrays as struct ing_rx; results[n] receives the codes.  -1: a packet's
 * destination was left unwritten by the classify pass */
int emu_rx_add(const uint32_t *prm, uint8_t *src, uint64_t src_stride, uint8_t *rep, uint64_t rep_stride, uint32_t *first, uint32_t *seen,
               uint32_t *gaps, uint32_t *nrep, uint32_t *rep_esi, uint32_t *live, const uint8_t *pkts, uint64_t pkt_stride,
               const uint32_t *tags, uint32_t n, int32_t *results) {
  ing_rx r;
  r.K = prm[0]; r.T = prm[1]; r.nblk = prm[2]; r.sbn0 = prm[3]; r.max_esi = prm[4]; r.rep_cap = prm[5];
  r.m1 = r.max_esi + 1u;
  r.bm_words = r.max_esi / 32u + 1u;
  r.src = src; r.src_stride = src_stride; r.rep = rep; r.rep_stride = rep_stride;
  r.first = first; r.seen = seen; r.gaps = gaps; r.nrep = nrep; r.rep_esi = rep_esi; r.live = live;
  if (n == 0) return 0;
  ing_call c;
  c.pkts = pkts; c.pkt_stride = pkt_stride; c.tags = tags; c.n = n;
  c.ntiles = (n + ING_TILE - 1u) / ING_TILE;
  std::vector<uint32_t> tagv(n), fidx(n), base((size_t)r.nblk * c.ntiles, 0), cnt(r.nblk);
  const uint64_t poison = 0xDEADBEEFDEADBEEFull; /* the device's per-call scratch holds whatever the last user left: every entry pass 6
                                                  * reads must have been written by pass 5 */
  std::vector<uint64_t> dst(n, poison);
  c.tagv = tagv.data(); c.codes = results; c.fidx = fidx.data(); c.dst = dst.data(); c.base = base.data();
  for (uint32_t k = 0; k < n; k++) ing_first(&r, &c, k); /* 1 */
  for (uint32_t b = 0; b < r.nblk; b++) {                /* 2 */
    uint32_t mx = 0, ct = 0;
    if (r.gaps[b])
      for (uint32_t e = 0; e < r.K; e++) ing_done_part(&r, b, e, &mx, &ct);
    ing_done_finish(&r, b, mx, ct);
  }
  for (uint32_t k = 0; k < n; k++) { /* 3 */
    const uint32_t b = ing_cand(&r, &c, k);
    if (b != ING_NONE) base[(size_t)b * c.ntiles + k / ING_TILE]++;
  }
  for (uint32_t b = 0; b < r.nblk; b++) { /* 4 */
    uint32_t run = r.nrep[b];
    for (uint32_t t = 0; t < c.ntiles; t++) { const uint32_t v = base[(size_t)b * c.ntiles + t]; base[(size_t)b * c.ntiles + t] = run; run += v; }
    r.nrep[b] = std::min(run, r.rep_cap);
  }
  for (uint32_t t = 0; t < c.ntiles; t++) { /* 5 */
    std::fill(cnt.begin(), cnt.end(), 0u);
    const uint32_t k1 = std::min(n, (t + 1u) * ING_TILE);
    std::vector<uint32_t> row(k1 - t * ING_TILE, ING_NONE);
    for (uint32_t k = t * ING_TILE; k < k1; k++) { /* (all candidates are found before any packet is classified, as in the kernel) */
      const uint32_t b = ing_cand(&r, &c, k);
      if (b != ING_NONE) row[k - t * ING_TILE] = base[(size_t)b * c.ntiles + t] + cnt[b]++;
    }
    for (uint32_t k = t * ING_TILE; k < k1; k++) ing_classify(&r, &c, k, row[k - t * ING_TILE]);
  }
  const uint32_t off = ing_payload_off(&c);
  for (uint32_t k = 0; k < n; k++) /* 6 */
    if (dst[k] == poison) return -1;
  for (uint32_t k = 0; k < n; k++)
    if (dst[k]) memcpy((void *)(uintptr_t)dst[k], pkts + (size_t)k * pkt_stride + off, r.T);
  for (uint32_t k = 0; k < n; k++) ing_fold(&r, &c, k); /* 7 */
  return 0;
}

} /* extern "C" */
