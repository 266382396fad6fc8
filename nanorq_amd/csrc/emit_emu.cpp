/* CPU emulation of the device-resident emit (emit_body.h): the same per-packet bodies the gfx950 kernel runs, called in loops in
 * its work order (block-major; a tag list bucketed by block first), over a table of segments.  The payload is written a byte at a
 * time -- what the kernel's byte path does; its wider paths must give the same bytes.  Test support, not part of the library:
 * build.build_emit_emu() makes tests/emu/libemit_emu.so of it.  It lives beside the bodies it drives, and its C entry points
 * (emu_tx_emit, emu_tx_emit_range, emu_emit_table, emu_emit_table_ready) are what the tests call. */
#include <stdint.h>
#include <string.h>

#include <vector>

#include "emit_emu.h"

/* every work item in order; -2: the work order is not a permutation of the packets */
template <bool MULTI>
static int run(const tx_src *s, const tx_call *c) {
  std::vector<uint8_t> hit(c->n, 0);
  uint32_t cols[TX_COLS];
  for (uint32_t w = 0; w < c->n; w++) {
    const uint32_t k = tx_packet_of<MULTI>(s, c, w);
    if (k >= c->n || hit[k]++) return -2;
    const uint32_t tag = tx_tag_of<MULTI>(s, c, k);
    if (c->tags_out) c->tags_out[k] = tag;
    int32_t code;
    const uint32_t g = tx_admit<MULTI>(s, tag, &code);
    const tx_blk t = tx_pick(s, g);
    const uint32_t n = g < TX_SEGS ? tx_rows(&t, tag, cols) : 0u;
    if (c->results) c->results[k] = code;
    if (n) tx_emit_bytes(&t, c, k, tag, cols, n);
  }
  return 0;
}

extern "C" {

/* The emit from a table of nseg segments WITH A READY MASK (a relay's table): ready = 8 words, bit b = block b of the span may
 * be emitted; a packet of another block of the span is left untouched with the result -2.  Otherwise as emu_emit_table, which
 * is this with all ones (ready = NULL). */
int emu_emit_table_ready(const uint32_t *prm, uint32_t nseg, const uint32_t *span, const uint8_t *const *src, const uint64_t *src_stride,
                         const uint8_t *const *inter, const uint64_t *inter_stride, const uint32_t *tags, uint32_t n, const uint32_t *range,
                         uint32_t inl, uint8_t *pkts, uint64_t pkt_stride, int32_t *results, uint32_t *tags_out, const uint32_t *ready);

/* The emit from a table of nseg segments: prm = nseg x {K, K', T, nblk, sbn0}, segment g's rows at src[g] / inter[g] with strides
 * src_stride[g] / inter_stride[g]; span = {sbn0, Z, ZL}.  List mode when tags is not NULL (n tags; results), else range mode with
 * range = {esi0, nL, nS, interleave} (tags_out; one segment: nL = nS).  -1: a bad table. */
int emu_emit_table(const uint32_t *prm, uint32_t nseg, const uint32_t *span, const uint8_t *const *src, const uint64_t *src_stride,
                   const uint8_t *const *inter, const uint64_t *inter_stride, const uint32_t *tags, uint32_t n, const uint32_t *range,
                   uint32_t inl, uint8_t *pkts, uint64_t pkt_stride, int32_t *results, uint32_t *tags_out) {
  return emu_emit_table_ready(prm, nseg, span, src, src_stride, inter, inter_stride, tags, n, range, inl, pkts, pkt_stride, results,
                              tags_out, nullptr);
}

int emu_emit_table_ready(const uint32_t *prm, uint32_t nseg, const uint32_t *span, const uint8_t *const *src, const uint64_t *src_stride,
                         const uint8_t *const *inter, const uint64_t *inter_stride, const uint32_t *tags, uint32_t n, const uint32_t *range,
                         uint32_t inl, uint8_t *pkts, uint64_t pkt_stride, int32_t *results, uint32_t *tags_out, const uint32_t *ready) {
  tx_src s;
  if (!emu_tx_table(&s, prm, nseg, span, src, src_stride, inter, inter_stride, ready)) return -1;
  tx_call c;
  memset(&c, 0, sizeof(c));
  c.pkts = pkts; c.pkt_stride = pkt_stride; c.inl = inl;
  std::vector<uint32_t> order;
  if (tags) {
    order = emu_tx_bucket(&s, tags, n);
    c.n = n; c.tags = tags; c.order = order.data(); c.results = results;
  } else {
    c.esi0 = range[0]; c.nL = range[1]; c.nS = range[2]; c.interleave = range[3]; c.tags_out = tags_out;
    c.n = s.ZL * c.nL + (s.Z - s.ZL) * c.nS;
  }
  return nseg > 1u ? run<true>(&s, &c) : run<false>(&s, &c); /* (the form the launcher picks) */
}

/* one segment, prm = {K, K', T, nblk, sbn0}: a transmission (nrq_tx) */
int emu_tx_emit(const uint32_t *prm, const uint8_t *src, uint64_t src_stride, const uint8_t *inter, uint64_t inter_stride,
                const uint32_t *tags, uint32_t n, uint32_t inl, uint8_t *pkts, uint64_t pkt_stride, int32_t *results) {
  const uint32_t span[3] = {prm[4], prm[3], prm[3]};
  return emu_emit_table(prm, 1, span, &src, &src_stride, &inter, &inter_stride, tags, n, nullptr, inl, pkts, pkt_stride, results,
                        nullptr);
}

int emu_tx_emit_range(const uint32_t *prm, const uint8_t *src, uint64_t src_stride, const uint8_t *inter, uint64_t inter_stride,
                      uint32_t esi0, uint32_t per_blk, uint32_t interleave, uint32_t inl, uint8_t *pkts, uint64_t pkt_stride,
                      uint32_t *tags_out) {
  const uint32_t span[3] = {prm[4], prm[3], prm[3]}, range[4] = {esi0, per_blk, per_blk, interleave};
  return emu_emit_table(prm, 1, span, &src, &src_stride, &inter, &inter_stride, nullptr, 0, range, inl, pkts, pkt_stride, nullptr,
                        tags_out);
}

} /* extern "C" */
