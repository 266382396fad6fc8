/* CPU emulation of the device-resident sender's emit (nanorq_amd/csrc/emit_body.h): the same per-packet bodies the gfx950
 * kernels run, called in loops in the kernels' work order (block-major; a tag list bucketed by block first).  The payload is
 * written a byte at a time -- what the kernels' byte path does; their wider paths must give the same bytes. */
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../nanorq_amd/csrc/emit_body.h"

static int setup(const uint32_t *prm, const uint8_t *src, uint64_t src_stride, const uint8_t *inter, uint64_t inter_stride, tx_blk *t) {
  /* prm = {K, K', T, nblk, sbn0} */
  memset(t, 0, sizeof(*t));
  if (!rq_params_init(prm[1], &t->p) || t->p.Kp != prm[1] || prm[0] == 0 || prm[0] > prm[1]) return -1;
  t->p.K = prm[0];
  t->K = prm[0]; t->T = prm[2]; t->nblk = prm[3]; t->sbn0 = prm[4];
  t->src = src; t->src_stride = src_stride; t->inter = inter; t->inter_stride = inter_stride;
  return 0;
}

/* every work item in order; -2: the work order is not a permutation of the packets */
static int run(const tx_blk *t, const tx_call *c) {
  std::vector<uint8_t> hit(c->n, 0);
  uint32_t cols[TX_COLS];
  for (uint32_t w = 0; w < c->n; w++) {
    const uint32_t k = tx_work_packet(t, c, w);
    if (k >= c->n || hit[k]++) return -2;
    const uint32_t tag = tx_packet_tag(t, c, k);
    if (c->tags_out) c->tags_out[k] = tag;
    const uint32_t n = tx_rows(t, tag, cols);
    if (c->results) c->results[k] = n ? 0 : -1;
    if (n) tx_emit_bytes(t, c, k, tag, cols, n);
  }
  return 0;
}

extern "C" {

int emu_tx_emit(const uint32_t *prm, const uint8_t *src, uint64_t src_stride, const uint8_t *inter, uint64_t inter_stride,
                const uint32_t *tags, uint32_t n, uint32_t inl, uint8_t *pkts, uint64_t pkt_stride, int32_t *results) {
  tx_blk t;
  if (setup(prm, src, src_stride, inter, inter_stride, &t)) return -1;
  /* the bucketing passes: per-bucket counts, exclusive scan, placement (the kernels place inside a bucket in any order) */
  std::vector<uint32_t> cnt(t.nblk + 1u, 0), order(n ? n : 1u);
  for (uint32_t k = 0; k < n; k++) cnt[tx_bin(&t, tags[k])]++;
  uint32_t run_ = 0;
  for (uint32_t b = 0; b <= t.nblk; b++) { const uint32_t v = cnt[b]; cnt[b] = run_; run_ += v; }
  for (uint32_t k = 0; k < n; k++) order[cnt[tx_bin(&t, tags[k])]++] = k;
  tx_call c;
  memset(&c, 0, sizeof(c));
  c.pkts = pkts; c.pkt_stride = pkt_stride; c.n = n; c.inl = inl; c.tags = tags; c.order = order.data(); c.results = results;
  return run(&t, &c);
}

int emu_tx_emit_range(const uint32_t *prm, const uint8_t *src, uint64_t src_stride, const uint8_t *inter, uint64_t inter_stride,
                      uint32_t esi0, uint32_t per_blk, uint32_t interleave, uint32_t inl, uint8_t *pkts, uint64_t pkt_stride,
                      uint32_t *tags_out) {
  tx_blk t;
  if (setup(prm, src, src_stride, inter, inter_stride, &t)) return -1;
  tx_call c;
  memset(&c, 0, sizeof(c));
  c.pkts = pkts; c.pkt_stride = pkt_stride; c.n = per_blk * t.nblk; c.inl = inl;
  c.esi0 = esi0; c.per_blk = per_blk; c.interleave = interleave; c.tags_out = tags_out;
  return run(&t, &c);
}

} /* extern "C" */
