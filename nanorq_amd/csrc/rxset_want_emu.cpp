/* CPU emulation of a reception set's want and held listings (want_set_body.h: nrq_ings_want_count_kernel / nrq_ings_held_count_kernel,
 * nrq_ings_lists_scan_kernel, nrq_ings_want_fill_kernel / nrq_ings_held_fill_kernel of nrq_device.hip, and the host flow of
 * rxset_list around them): the same per-block and per-word bodies, called in loops in the kernels' order and rounds -- 256 seen
 * words per round, the workgroup's sum and scan as running sums, the keys of a block by the 256 "threads" in turn -- over members
 * described as rxset_lists_emu.cpp describes them.  Test support, not part of the library: build.build_rxset_want_emu() makes
 * tests/emu/librxset_want_emu.so of it. */
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "emu_scan.h"
#include "want_set_body.h"

#define EMU_GUARD 64u /* words behind the nb + 1 counts / offsets that no pass may touch */
#define EMU_GUARD_WORD 0xA5C3F00Du

/* the table of the arguments (prm[m] = {K, T, nblk, sbn0, max_esi, rep_cap, key, objZ}, ptr[m] = {src, rep, first, seen, gaps,
 * nrep, rep_esi, live}), members sorted by (key, sbn0); false: a bad table */
static bool emu_table(uint32_t nmem, const uint32_t *prm, const uint64_t *ptr, ings_tab &t) {
  if (nmem > INGS_MAX_MEMBERS) return false;
  std::vector<uint32_t> order(nmem);
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

/* wn_count_wg */
static void emu_want_count(const ing_rx *r, const wn_q *q, uint32_t b, uint32_t *cnt) {
  const uint32_t w_end = wn_end(q), need = wn_need(r, q, b);
  uint32_t found = 0;
  for (uint32_t w0 = wn_first(q); w0 < w_end && found < need; w0 += WN_ROUND)
    for (uint32_t t = 0; t < WN_ROUND; t++)
      if (w0 + t < w_end) found += ing_popc(wn_bits(r, q, b, w0 + t));
  *cnt = std::min(found, need);
}

/* wn_fill_wg */
static void emu_want_fill(const ing_rx *r, const wn_q *q, uint32_t b, uint32_t *dst) {
  const uint32_t w_end = wn_end(q), need = wn_need(r, q, b);
  uint32_t placed = 0, bits[WN_ROUND], ps[WN_ROUND];
  for (uint32_t w0 = wn_first(q); w0 < w_end && placed < need; w0 += WN_ROUND) {
    uint32_t run = 0;
    for (uint32_t t = 0; t < WN_ROUND; t++) {
      bits[t] = w0 + t < w_end ? wn_bits(r, q, b, w0 + t) : 0u;
      run += ing_popc(bits[t]);
      ps[t] = run;
    }
    for (uint32_t t = 0; t < WN_ROUND; t++) wn_put(r, b, w0 + t, bits[t], placed + ps[t] - ing_popc(bits[t]), need, dst);
    placed += ps[WN_ROUND - 1u];
  }
}

/* hl_count_wg */
static void emu_held_count(const ing_rx *r, uint32_t b, uint32_t *cnt) {
  const uint32_t nw = ing_src_words(r);
  uint32_t n = 0;
  for (uint32_t t = 0; t < 256u; t++)
    for (uint32_t w = t; w < nw; w += 256u) n += ing_popc(hl_have(r, b, w));
  *cnt = n + hl_nrep(r, b);
}

/* hl_fill_wg */
static void emu_held_fill(const ing_rx *r, uint32_t b, uint32_t *out, uint32_t o) {
  const uint32_t nw = ing_src_words(r);
  for (uint32_t w0 = 0; w0 < nw; w0 += 256u) {
    uint32_t ps = 0; /* (the inclusive scan over the round's threads) */
    for (uint32_t t = 0; t < 256u; t++) {
      const uint32_t w = w0 + t, have = w < nw ? hl_have(r, b, w) : 0u, cnt = ing_popc(have);
      ps += cnt;
      hl_put(r, b, w, have, out + o + ps - cnt);
    }
    o += ps;
  }
  const uint32_t nrep = hl_nrep(r, b);
  for (uint32_t t = 0; t < 256u; t++)
    for (uint32_t q = t; q < nrep; q += 256u) out[o + q] = hl_rep_tag(r, b, q);
}

/* rxset_list: count, scan, "download", cap check, fill.  c NULL: the held listing */
static int emu_list(uint32_t nmem, const uint32_t *prm, const uint64_t *ptr, const wns_call *c, uint32_t *keys, uint32_t *tags, uint32_t cap,
                    uint32_t *h_cnt, uint32_t *n) {
  *n = 0;
  if (keys && !tags) return -1;
  std::vector<ings_tab> tabv(1);
  ings_tab &t = tabv[0];
  if (!emu_table(nmem, prm, ptr, t)) return -2;
  const uint32_t nb = t.nblk;
  if (nb == 0) return 0; /* (an empty set launches nothing) */
  std::vector<uint32_t> work((size_t)nb + 1u + EMU_GUARD, EMU_GUARD_WORD);
  uint32_t *off = work.data();
  for (uint32_t g = 0; g < nb; g++) { /* count: a workgroup per global block */
    uint32_t b;
    const ing_rx *r = lss_block(&t, g, &b);
    if (c) {
      const wn_q q = wns_query(r, c);
      emu_want_count(r, &q, b, off + g);
    } else {
      emu_held_count(r, b, off + g);
    }
    wns_count_end(&t, g, off);
  }
  emu_scan(off, nb + 1u);
  *n = off[nb];
  if (h_cnt)
    for (uint32_t g = 0; g < nb; g++) h_cnt[g] = off[g + 1u] - off[g];
  int rc = 0;
  if (tags && cap < *n) rc = -1;
  if (tags && rc == 0) {
    for (uint32_t g = 0; g < nb; g++) { /* fill: a workgroup per global block */
      const uint32_t lo = off[g], hi = off[g + 1u];
      if (lo == hi) continue;
      uint32_t b, key;
      const ing_rx *r = wns_block(&t, g, &b, &key);
      if (c) {
        const wn_q q = wns_query(r, c);
        emu_want_fill(r, &q, b, tags + lo);
      } else {
        emu_held_fill(r, b, tags, lo);
      }
      if (keys)
        for (uint32_t i = 0; i < 256u; i++) wns_put_keys(keys, lo, hi, key, i, 256u);
    }
  }
  for (uint32_t i = 0; i < EMU_GUARD; i++)
    if (off[nb + 1u + i] != EMU_GUARD_WORD) return -3;
  return rc;
}

extern "C" {

/* nrq_rxset_want over emulated members: *n = the total, cnt (nullable) [blocks] the tags per block, tags / keys (nullable) with
 * room for cap entries.  0, -1 as the call (wn_check's refusals, keys without tags, cap < *n: nothing written), -2: a bad table,
 * -3: a pass wrote behind the counts. */
int emu_rxset_want(uint32_t nmem, const uint32_t *prm, const uint64_t *ptr, uint32_t flags, uint32_t extra, uint32_t esi_from, uint32_t *keys,
                   uint32_t *tags, uint32_t cap, uint32_t *cnt, uint32_t *n) {
  *n = 0;
  if (wn_check(flags, extra, esi_from)) return -1;
  const wns_call c{flags, extra, esi_from};
  return emu_list(nmem, prm, ptr, &c, keys, tags, cap, cnt, n);
}

/* nrq_rxset_held likewise */
int emu_rxset_held(uint32_t nmem, const uint32_t *prm, const uint64_t *ptr, uint32_t *keys, uint32_t *tags, uint32_t cap, uint32_t *cnt,
                   uint32_t *n) {
  return emu_list(nmem, prm, ptr, nullptr, keys, tags, cap, cnt, n);
}

} /* extern "C" */
