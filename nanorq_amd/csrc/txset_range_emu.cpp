/* CPU emulation of the map pass of a sender set's range mode (emit_set_range_body.h): the bodies nrq_txs_range_kernel runs --
 * the staging of the per-segment words, their prefix, the map of one work item -- called in loops in kernel order, workgroup by
 * workgroup of 256 items, over a table given as emu_txset_emit's prm rows.  It returns the lists the pass leaves for the set's
 * emit kernels; the packets of the CPU tier come from feeding those lists to emu_txset_emit / emu_sys_txset_emit, which are not
 * changed.  Test support, not part of the library: build.build_txset_range_emu() makes tests/emu/libtxset_range_emu.so of it. */
#include <stdint.h>
#include <string.h>

#include <vector>

#include "emit_set_range_body.h"

extern "C" {

/* The map over nseg segments sorted by (key, sbn0).
 *   prm [nseg][8] = {K, K', T, nblk, sbn0, key, -, -} (emu_txset_emit's rows; K', T and the last two are not read)
 *   call [5] = {source, rep0, nrep, G, order}; n: the packets of the call (the caller's count)
 *   keys, tags, seg_out, order_out [n]; nsym [n] nullable
 * -1: a bad table or call; -2: the work order is not a permutation of the packets; -3: it is not block-major; -4: n is not the
 * table's count. */
int emu_txset_range(uint32_t nseg, const uint32_t *prm, const uint32_t *call, uint32_t n, uint32_t *keys, uint32_t *tags, uint8_t *nsym,
                    uint32_t *seg_out, uint32_t *order_out) {
  if (nseg > TXS_MAX_SEGS || call[0] > 1u || call[3] == 0u || call[3] > 64u || call[4] > 1u) return -1;
  std::vector<txs_tab> tv(1);
  txs_tab &t = tv[0];
  memset(&t, 0, sizeof(t));
  t.nseg = nseg;
  for (uint32_t g = 0; g < nseg; g++) {
    const uint32_t *q = prm + 8u * g;
    txs_seg &S = t.seg[g];
    if (q[0] == 0 || q[3] == 0) return -1;
    S.b.K = q[0]; S.b.nblk = q[3]; S.b.sbn0 = q[4];
    S.key = q[5]; S.blk0 = t.nblk;
    t.key[g] = S.key; t.sbn0[g] = S.b.sbn0; t.cnt[g] = S.b.nblk; t.blk0[g] = S.blk0;
    t.nblk += S.b.nblk;
  }
  if (t.nblk > TXS_MAX_BLOCKS) return -1;
  txr_call c;
  memset(&c, 0, sizeof(c));
  c.source = call[0]; c.rep0 = call[1]; c.nrep = call[2]; c.G = call[3]; c.order = call[4];
  c.n = n;
  c.keys = keys; c.tags = tags; c.nsym = nsym; c.seg = seg_out; c.worder = order_out;
  uint64_t total = 0;
  for (uint32_t g = 0; g < nseg; g++) total += (uint64_t)t.cnt[g] * txr_len(t.seg[g].b.K, c.source, c.nrep, c.G);
  if (total != n) return -4;
  for (uint32_t k = 0; k < n; k++) order_out[k] = seg_out[k] = TX_NONE;
  /* the pass, a workgroup of 256 work items at a time: staging, barrier, prefix, barrier, one item per thread */
  std::vector<txr_stage_t> sv(1);
  txr_stage_t &s = sv[0];
  for (uint32_t w0 = 0; w0 < n; w0 += 256u) {
    memset(&s, 0xA5, sizeof(s));
    for (uint32_t i = 0; i < 256u; i++)
      if (i < nseg) txr_stage(&t, &c, i, &s);
    for (uint32_t i = 0; i < 256u; i++)
      if (i <= nseg) txr_stage_prefix(nseg, i, &s);
    for (uint32_t i = 0; i < 256u; i++) {
      const uint32_t w = w0 + i;
      if (w < c.n && w < s.pre[nseg]) txr_map(&s, nseg, &c, w);
    }
  }
  /* what the emit kernels rely on: a permutation, block-major */
  std::vector<uint8_t> hit(n ? n : 1u, 0);
  uint32_t last = 0;
  for (uint32_t w = 0; w < n; w++) {
    const uint32_t k = order_out[w];
    if (k >= n || hit[k]++) return -2;
    if (seg_out[k] >= nseg) return -2;
    const uint32_t bin = txs_bin(t.sbn0, t.blk0, t.nblk, seg_out[k], tags[k]);
    if (bin < last || bin >= t.nblk) return -3;
    last = bin;
  }
  return 0;
}

} /* extern "C" */
