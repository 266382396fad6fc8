/* CPU emulation of a reception set's want and held listings as runs (nrq_rxset_want_syms / nrq_rxset_held_syms) and of a sender
 * set's held emit of packets of several symbols (NRQ_TX_HELD in nrq_txset_emit_syms), over runs_set_body.h.  The listings run in
 * the rounds of the gfx950 kernels (nrq_ings_want_syms_* / nrq_ings_held_syms_*, nrq_ings_lists_scan_kernel and the host flow of
 * rxset_list_syms around them): one "workgroup" per global block finds its member and key, WN_ROUND words (rows) per round, one per
 * "thread", the workgroup's sum-scan and max-scan done in loops, the run start, the symbols found and the packets placed carried
 * from round to round, the keys of a block by the 256 "threads" in turn -- over members described as rxset_want_emu.cpp describes
 * them.  The held emit runs the bucketing passes of txset_emu.cpp and, per packet in work order, the kernel's admission
 * (hss_packet, hss_slot_held; the ballot over a packet's lanes is an AND over its slots) and its walk over the block's repair list
 * in trips of 64 entries, and moves the payload a byte at a time; the wave-level code -- ballots, the row indices handed through
 * LDS, the wider payload paths -- is covered by the byte-exact GPU tests only (tests/test_gpu_rxset_runs.py).  Test support, not
 * part of the library: build.build_rxset_runs_emu() makes tests/emu/librxset_runs_emu.so of it. */
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "emu_scan.h"
#include "runs_emu_walks.h"
#include "runs_set_body.h"

#define EMU_GUARD 64u /* words behind the nb + 2 counts / offsets / totals that no pass may touch */
#define EMU_GUARD_WORD 0xA5C3F00Du
#define EMU_TILE 4096u /* TX_BIN_TILE: packets per workgroup of the bucketing passes */

/* the member table of the arguments, as rxset_want_emu.cpp: prm[m] = {K, T, nblk, sbn0, max_esi, rep_cap, key, objZ}, ptr[m] =
 * {src, rep, first, seen, gaps, nrep, rep_esi, live}, members sorted here by (key, sbn0); false: a bad table */
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

/* the walks of global block g's member: c NULL the held listing.  Count (tags NULL): returns the packets, *syms the symbols; fill:
 * returns the place behind the block's packets */
static uint32_t block_walk(const ing_rx *r, uint32_t b, const wns_call *c, uint32_t G, uint32_t *tags, uint8_t *nsym, uint32_t at, uint32_t *syms) {
  if (c) {
    const wn_q q = wns_query(r, c);
    const rn_walk k = rn_walk_want(r, &q, b);
    return bits_walk(r, &k, G, tags, nsym, at, syms);
  }
  const rn_walk k = rn_walk_held(r, b);
  uint32_t n = bits_walk(r, &k, G, tags, nsym, at, syms);
  if (n == RN_ALL) return n;
  if (syms) *syms += hl_nrep(r, b);
  return tags ? rows_walk(r, b, G, tags, nsym, n) : n + rows_walk(r, b, G, nullptr, nullptr, 0u);
}

/* rxset_list_syms: the symbol total zeroed, count, scan, "download", cap check, fill.  c NULL: the held listing */
static int emu_list_syms(uint32_t nmem, const uint32_t *prm, const uint64_t *ptr, const wns_call *c, uint32_t G, uint32_t *keys, uint32_t *tags,
                         uint8_t *nsym, uint32_t cap, uint32_t *h_cnt, uint32_t *npkt, uint32_t *nsym_total) {
  if (!npkt) return -1; /* rn_check */
  *npkt = 0;
  if (nsym_total) *nsym_total = 0;
  if (G == 0 || G > SY_G_MAX || !tags != !nsym) return -1;
  if (c && wn_check(c->flags, c->extra, c->esi_from)) return -1;
  if (keys && !tags) return -1;
  std::vector<ings_tab> tabv(1);
  ings_tab &t = tabv[0];
  if (!emu_table(nmem, prm, ptr, t)) return -2;
  const uint32_t nb = t.nblk;
  if (nb == 0) return 0; /* (an empty set launches nothing) */
  std::vector<uint32_t> work((size_t)nb + 2u + EMU_GUARD, EMU_GUARD_WORD);
  uint32_t *off = work.data();
  off[nb + 1u] = 0; /* (the memset in front of the count kernel) */
  for (uint32_t g = 0; g < nb; g++) { /* count: a workgroup per global block */
    uint32_t b, syms = 0;
    const ing_rx *r = lss_block(&t, g, &b);
    off[g] = block_walk(r, b, c, G, nullptr, nullptr, 0u, &syms);
    wns_count_end(&t, g, off);
    off[nb + 1u] += syms; /* (the atomic add) */
  }
  emu_scan(off, nb + 1u);
  *npkt = off[nb];
  if (nsym_total) *nsym_total = off[nb + 1u];
  if (h_cnt)
    for (uint32_t g = 0; g < nb; g++) h_cnt[g] = off[g + 1u] - off[g];
  int rc = 0;
  if (tags && cap < *npkt) rc = -1;
  if (tags && rc == 0) {
    for (uint32_t g = 0; g < nb; g++) { /* fill: a workgroup per global block */
      const uint32_t lo = off[g], hi = off[g + 1u];
      if (lo == hi) continue;
      uint32_t b, key;
      const ing_rx *r = wns_block(&t, g, &b, &key);
      if (block_walk(r, b, c, G, tags, nsym, lo, nullptr) != hi) return -4; /* (the passes disagree) */
      if (keys)
        for (uint32_t i = 0; i < 256u; i++) wns_put_keys(keys, lo, hi, key, i, 256u);
    }
  }
  for (uint32_t i = 0; i < EMU_GUARD; i++)
    if (off[nb + 2u + i] != EMU_GUARD_WORD) return -3;
  return rc;
}

/* one whole packet of cnt symbols in any header form, a byte at a time: slot i from the rows the kind names (rows[i]: the repair
 * row found for ESI e + i, TX_HELD_REP only), symbol 0 with the header as a one-symbol packet, the others behind it */
static void emit_bytes(const txs_seg *S, const txs_call *c, uint32_t k, uint32_t key, uint32_t tag, uint32_t cnt, uint32_t kind, const uint32_t *rows) {
  uint32_t cols[TX_COLS];
  for (uint32_t i = 0; i < cnt; i++) {
    uint32_t n;
    const uint8_t *base;
    if (kind == TX_HELD_REP) {
      cols[0] = rows[i];
      n = 1u;
      base = tx_held_rep_base(&S->h, tx_block(&S->b, tag));
    } else {
      n = tx_rows(&S->b, tag + i, cols);
      base = tx_base(&S->b, tag + i);
    }
    txs_call c1 = *c;
    if (i) { c1.pkts = c->pkts + c->hdr + (uint64_t)i * c->T; c1.hdr = 0u; }
    txs_emit_bytes(base, &c1, k, key, tag + i, cols, n);
  }
}

extern "C" {

/* nrq_rxset_want_syms over emulated members: *npkt = the packets, *nsym_total (nullable) = the symbols, cnt (nullable) [blocks] the
 * packets per block, keys (nullable) / tags / nsym with room for cap packets.  0, -1 as the call (its refusals; cap < *npkt: totals
 * and counts filled, nothing written), -2: a bad table, -3: a pass wrote behind the offsets and totals, -4: count and fill disagree. */
int emu_rxset_want_syms(uint32_t nmem, const uint32_t *prm, const uint64_t *ptr, uint32_t flags, uint32_t extra, uint32_t esi_from, uint32_t G,
                        uint32_t *keys, uint32_t *tags, uint8_t *nsym, uint32_t cap, uint32_t *cnt, uint32_t *npkt, uint32_t *nsym_total) {
  const wns_call c{flags, extra, esi_from};
  return emu_list_syms(nmem, prm, ptr, &c, G, keys, tags, nsym, cap, cnt, npkt, nsym_total);
}

/* nrq_rxset_held_syms likewise */
int emu_rxset_held_syms(uint32_t nmem, const uint32_t *prm, const uint64_t *ptr, uint32_t G, uint32_t *keys, uint32_t *tags, uint8_t *nsym,
                        uint32_t cap, uint32_t *cnt, uint32_t *npkt, uint32_t *nsym_total) {
  return emu_list_syms(nmem, prm, ptr, nullptr, G, keys, tags, nsym, cap, cnt, npkt, nsym_total);
}

/* The set emit with NRQ_TX_HELD of n packets of up to G symbols over nseg segments sorted by (key, sbn0); prm, ptr (with the held
 * columns), ready, keys, hdr, order_out as emu_txset_emit (txset_emu.cpp), tags the first tags, nsym nullable.
 * -1: a bad table or G; -2: the work order is not a permutation of the packets; -3: it is not block-major. */
int emu_txset_emit_held_syms(uint32_t nseg, const uint32_t *prm, const uint64_t *ptr, const uint32_t *ready, const uint32_t *keys,
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
    S.h.seen = (const uint32_t *)(uintptr_t)a[4]; S.h.rep_esi = (const uint32_t *)(uintptr_t)a[5];
    S.h.nrep = (const uint32_t *)(uintptr_t)a[6]; S.h.rep = (const uint8_t *)(uintptr_t)a[7]; S.h.rep_stride = a[8];
    S.h.bm_words = q[6]; S.h.rep_cap = q[7];
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
  /* every packet in work order, as nrq_emit_set_held_syms_kernel */
  std::vector<uint8_t> hit(n ? n : 1u, 0);
  uint32_t last_bin = 0, rows[SY_G_MAX];
  for (uint32_t w = 0; w < n; w++) {
    const uint32_t k = c.order[w];
    if (k >= n || hit[k]++) return -2;
    const uint32_t tag = tags[k], e = tag & SY_ESI_MAX;
    const uint32_t bin = txs_bin(t.sbn0, t.blk0, t.nblk, c.seg[k], tag);
    if (bin < last_bin) return -3;
    last_bin = bin;
    int32_t code;
    uint32_t pc, rdy, kind = TX_READY;
    uint32_t sg = hss_packet(&t, &r, &y, k, tag, c.seg[k], &code, &pc, &rdy);
    if (sg < TXS_MAX_SEGS && !rdy) {
      bool all = true;
      for (uint32_t i = 0; i < pc; i++) all = all && hss_slot_held(&t, sg, tag, e + i); /* (the ballot over the packet's lanes) */
      if (!all) { code = TX_NOT_READY; sg = TXS_NONE; }
      else kind = hss_kind(&t, sg, tag);
    }
    if (sg < TXS_MAX_SEGS && kind == TX_HELD_REP) { /* the wave's walk over the block's repair list, 64 entries a trip */
      const tx_held_seg *hs = &t.seg[sg].h;
      const uint32_t b = tx_block(&t.seg[sg].b, tag), nrep = tx_held_nrep(hs, b);
      for (uint32_t i = 0; i < pc; i++) rows[i] = TX_NONE;
      for (uint32_t q0 = 0; q0 < nrep; q0 += 64u)
        for (uint32_t lane = 0; lane < 64u && q0 + lane < nrep; lane++) {
          const uint32_t x = hs->rep_esi[(uint64_t)b * hs->rep_cap + q0 + lane] - e;
          if (x < pc) rows[x] = q0 + lane;
        }
      for (uint32_t i = 0; i < pc; i++)
        if (rows[i] == TX_NONE) { code = TX_NOT_READY; sg = TXS_NONE; }
    }
    if (results) results[k] = code;
    if (sg < TXS_MAX_SEGS) emit_bytes(&t.seg[sg], &c, k, txs_key_of(&c, k), tag, pc, kind, rows);
  }
  return 0;
}

} /* extern "C" */
