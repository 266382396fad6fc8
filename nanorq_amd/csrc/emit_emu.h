/* emit_emu.h -- what the emit emulation drivers (emit_emu.cpp, held_emu.cpp, syms_emu.cpp) share: the source table from the flat
 * arrays their C entry points take, and a tag list bucketed into the work order.  Test support, not part of the library. */
#ifndef NRQ_EMIT_EMU_H
#define NRQ_EMIT_EMU_H

#include <stdint.h>
#include <string.h>

#include <vector>

#include "emit_body.h"

/* The table of nseg segments: prm = nseg x {K, K', T, nblk, sbn0}, segment g's rows at src[g] / inter[g] with strides src_stride[g]
 * / inter_stride[g] (src NULL: a table for the packet maps only); span = {sbn0, Z, ZL}; ready = 8 words, a bit per block of the
 * span (NULL: all ones).  false: a bad table. */
static inline bool emu_tx_table(tx_src *s, const uint32_t *prm, uint32_t nseg, const uint32_t *span, const uint8_t *const *src,
                                const uint64_t *src_stride, const uint8_t *const *inter, const uint64_t *inter_stride, const uint32_t *ready) {
  memset(s, 0, sizeof(*s));
  if (nseg == 0 || nseg > TX_SEGS) return false;
  for (uint32_t g = 0; g < nseg; g++) {
    const uint32_t *q = prm + 5u * g;
    tx_blk &t = s->seg[g];
    if (!rq_params_init(q[1], &t.p) || t.p.Kp != q[1] || q[0] == 0 || q[0] > q[1]) return false;
    t.p.K = q[0];
    t.K = q[0]; t.T = q[2]; t.nblk = q[3]; t.sbn0 = q[4];
    if (src) { t.src = src[g]; t.src_stride = src_stride[g]; t.inter = inter[g]; t.inter_stride = inter_stride[g]; }
  }
  s->nseg = nseg; s->sbn0 = span[0]; s->Z = span[1]; s->ZL = span[2];
  if (ready) memcpy(s->ready, ready, sizeof(s->ready));
  else memset(s->ready, 0xFF, sizeof(s->ready));
  return true;
}

/* the bucketing passes over n tags: per-bucket counts, exclusive scan, placement (the kernels place inside a bucket in any order) */
static inline std::vector<uint32_t> emu_tx_bucket(const tx_src *s, const uint32_t *tags, uint32_t n) {
  std::vector<uint32_t> order(n ? n : 1u), cnt(s->Z + 1u, 0);
  for (uint32_t k = 0; k < n; k++) cnt[tx_bin(s->sbn0, s->Z, tags[k])]++;
  uint32_t run = 0;
  for (uint32_t b = 0; b <= s->Z; b++) { const uint32_t v = cnt[b]; cnt[b] = run; run += v; }
  for (uint32_t k = 0; k < n; k++) order[cnt[tx_bin(s->sbn0, s->Z, tags[k])]++] = k;
  return order;
}

#endif /* NRQ_EMIT_EMU_H */
