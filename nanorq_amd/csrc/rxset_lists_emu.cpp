/* CPU emulation of a reception set's listing passes (lists_set_body.h: nrq_ings_counts_kernel, nrq_ings_lists_count_kernel,
 * nrq_ings_lists_scan_kernel, nrq_ings_lists_fill_kernel of nrq_device.hip): the same per-block and per-word bodies, called in
 * loops in the kernels' order and rounds -- the fill places LSS_ROUND seen words per round with a running sum over the words'
 * counts where the kernel scans them in LDS -- and rxset_plan.h's grouping behind a C interface (host code as it is, no emulation).
 * Test support, not part of the library: build.build_rxset_lists_emu() makes tests/emu/librxset_lists_emu.so of it. */
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "lists_set_body.h"
#include "rxset_plan.h"

#define EMU_GUARD 64u          /* words behind the list buffer that no pass may touch */
#define EMU_GUARD_WORD 0xA5C3F00Du

/* the table of emu_rxset_add's arguments, members sorted by (key, sbn0); false: a bad table */
static bool emu_table(uint32_t nmem, const uint32_t *prm, const uint64_t *ptr, ings_tab &t, std::vector<uint32_t> &order) {
  if (nmem > INGS_MAX_MEMBERS) return false;
  order.resize(nmem);
  std::iota(order.begin(), order.end(), 0u);
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    const uint32_t *pa = prm + 8u * a, *pb = prm + 8u * b;
    return pa[6] != pb[6] ? pa[6] < pb[6] : pa[3] < pb[3];
  });
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
  return t.nblk <= INGS_MAX_BLOCKS;
}

extern "C" {

/* words of the list buffer the library allocates for these members: every block's K + rep_cap list words, gaps and offsets, the total */
uint64_t emu_rxset_lists_words(uint32_t nmem, const uint32_t *prm) {
  uint64_t w = 1;
  for (uint32_t m = 0; m < nmem; m++) w += (uint64_t)prm[8u * m + 2u] * ((uint64_t)prm[8u * m] + prm[8u * m + 5u] + 2u);
  return w;
}

/* Members as in emu_rxset_add (prm[m] = {K, T, nblk, sbn0, max_esi, rep_cap, key, objZ}, ptr[m] = {src, rep, first, seen, gaps,
 * nrep, rep_esi, live}).  keys / sbn [nblk]: the block order.  counts [2 * nblk]: the counts pass (gaps, nrep).  buf: the list
 * buffer, emu_rxset_lists_words() words as the library sizes it, written as the three listing passes write it (gaps, offsets and
 * total, lists); it lies in a buffer of the emulation's own with guard words behind it.  Returns the number of blocks, -2: a bad
 * table, -3: a guard word was overwritten. */
int emu_rxset_lists(uint32_t nmem, const uint32_t *prm, const uint64_t *ptr, uint32_t *keys, uint32_t *sbn, uint32_t *counts, uint32_t *buf) {
  std::vector<ings_tab> tabv(1);
  ings_tab &t = tabv[0];
  std::vector<uint32_t> order;
  if (!emu_table(nmem, prm, ptr, t, order)) return -2;
  const uint32_t nb = t.nblk;
  const uint64_t words = emu_rxset_lists_words(nmem, prm);
  std::vector<uint32_t> work(words + EMU_GUARD, EMU_GUARD_WORD);
  uint32_t *w = work.data();
  for (uint32_t g = 0; g < nb; g++) { /* the block order, and the counts pass */
    uint32_t b;
    const ing_rx *r = lss_block(&t, g, &b);
    keys[g] = t.key[ings_member_of_block(t.blk0, t.nmem, g)];
    sbn[g] = r->sbn0 + b;
    lss_counts(&t, g, &counts[g], &counts[nb + g]);
  }
  if (nb) {
    for (uint32_t g = 0; g < nb; g++) lss_list_count(&t, g, w); /* count */
    { /* scan: nb + 1 entries in place, a run of entries per thread of the one workgroup, a scan over the threads' sums */
      uint32_t *cnt = w + nb, ps[256];
      const uint32_t n = nb + 1u, per = (n + 255u) / 256u;
      for (uint32_t i = 0; i < 256u; i++) {
        const uint32_t j0 = std::min(n, i * per), j1 = std::min(n, j0 + per);
        ps[i] = (i ? ps[i - 1u] : 0u) + std::accumulate(cnt + j0, cnt + j1, 0u);
      }
      for (uint32_t i = 0; i < 256u; i++) {
        const uint32_t j0 = std::min(n, i * per), j1 = std::min(n, j0 + per);
        uint32_t run = i ? ps[i - 1u] : 0u;
        for (uint32_t j = j0; j < j1; j++) { const uint32_t v = cnt[j]; cnt[j] = run; run += v; }
      }
    }
    for (uint32_t g = 0; g < nb; g++) { /* fill: a workgroup per block, LSS_ROUND words per round */
      uint32_t b;
      const ing_rx *r = lss_block(&t, g, &b);
      uint32_t *out = w + 2u * nb + 1u + w[nb + g];
      const uint32_t nrep = r->nrep[b], nw = ing_src_words(r);
      for (uint32_t q = 0; q < nrep; q++) out[q] = r->rep_esi[(uint64_t)b * r->rep_cap + q];
      uint32_t o = nrep;
      for (uint32_t w0 = 0; w0 < nw; w0 += LSS_ROUND) {
        uint32_t ps = 0; /* (the inclusive scan over the round's threads) */
        for (uint32_t i = 0; i < LSS_ROUND; i++) {
          const uint32_t miss = lss_miss(r, b, w0 + i), cnt = ing_popc(miss);
          ps += cnt;
          lss_put(w0 + i, miss, out + o + ps - cnt);
        }
        o += ps;
      }
    }
  } else {
    w[0] = 0; /* (an empty set launches nothing: the total is 0 by definition) */
  }
  for (uint32_t i = 0; i < EMU_GUARD; i++)
    if (w[words + i] != EMU_GUARD_WORD) return -3;
  memcpy(buf, w, words * 4u);
  return (int)nb;
}

/* rxset_plan(): mem [nmem][4] = {K, K', max_esi, has_relay}; member / ng / nr [nb].  Out: chunk_of[nb] = the chunk a block is in
 * or 0xFFFFFFFF, pos_of[nb] = its place in the chunk, chunk_prm [cap][4] = {K, K', has_relay, blocks}.  Returns the number of
 * chunks, or -1: more than cap. */
int emu_rxset_plan(const uint32_t *mem, uint32_t nmem, const uint32_t *member, const uint32_t *ng, const uint32_t *nr, uint32_t nb,
                   uint32_t *chunk_of, uint32_t *pos_of, uint32_t *chunk_prm, uint32_t cap) {
  std::vector<rxset_plan_member> pm(nmem);
  for (uint32_t m = 0; m < nmem; m++) pm[m] = rxset_plan_member{mem[4u * m], mem[4u * m + 1u], mem[4u * m + 2u], mem[4u * m + 3u]};
  const std::vector<rxset_chunk> ch = rxset_plan(pm.data(), member, ng, nr, nb);
  if (ch.size() > cap) return -1;
  for (uint32_t j = 0; j < nb; j++) chunk_of[j] = pos_of[j] = 0xFFFFFFFFu;
  for (size_t c = 0; c < ch.size(); c++) {
    chunk_prm[4u * c] = ch[c].K; chunk_prm[4u * c + 1u] = ch[c].Kp; chunk_prm[4u * c + 2u] = ch[c].has_relay;
    chunk_prm[4u * c + 3u] = (uint32_t)ch[c].blocks.size();
    for (size_t i = 0; i < ch[c].blocks.size(); i++) {
      const uint32_t j = ch[c].blocks[i];
      if (j >= nb || chunk_of[j] != 0xFFFFFFFFu) return -2; /* (a block twice) */
      chunk_of[j] = (uint32_t)c;
      pos_of[j] = (uint32_t)i;
    }
  }
  return (int)ch.size();
}

} /* extern "C" */
