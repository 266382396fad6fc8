/*
 * want_body.h -- the bodies of the listing of what a reception still WANTS (nrq_rx_want / nrq_orx_want, include/nanorq_hip.h): the
 * tags (nanorq_tag() form) a node sends upstream to top its blocks up, block-major, within a block ascending.  Per block with
 * g = gaps[b] missing source symbols and r repair rows in use (hl_nrep):
 *   g == 0              nothing
 *   NRQ_WANT_SOURCE     the g source ESIs whose seen bit is clear
 *   repair mode         the need = min(max(g + extra - r, 0), rep_cap - r) lowest ESIs of [max(K, esi_from), max_esi] whose seen
 *                       bit is clear (fewer when the range holds fewer)
 * Both modes are one walk: the clear bits of the seen words from ESI lo to ESI hi, the first `need` of them.
 *
 * nrq_device.hip runs them in three short kernels on the reception's stream -- count (per block: popcounts, 256 words per round,
 * until `need` clear bits are found), an exclusive scan over the blocks, fill (per block: per round a scan over the words' counts
 * places each word's tags, until `need` are placed) -- and want_emu.cpp in the same rounds on the CPU.  They only read the
 * reception's books (ingest_body.h); every decision depends on the books alone, so the list is deterministic.
 */
#ifndef NRQ_WANT_BODY_H
#define NRQ_WANT_BODY_H

#include <stdint.h>

#include "held_body.h" /* hl_nrep */
#include "ingest_body.h"

#define WN_SOURCE 1u            /* NRQ_WANT_SOURCE */
#define WN_EXTRA_MAX (1u << 24) /* more than there are ESIs */
#define WN_ROUND 256u           /* seen words per round: one per thread of the workgroup */

/* what is wrong with a call's arguments: 0 = nothing, 1 = an unknown flag, 2 = extra / esi_from beside WN_SOURCE, 3 = extra too large */
ING_HD int wn_check(uint32_t flags, uint32_t extra, uint32_t esi_from) {
  if (flags & ~WN_SOURCE) return 1;
  if ((flags & WN_SOURCE) && (extra || esi_from)) return 2;
  if (extra > WN_EXTRA_MAX) return 3;
  return 0;
}

/* one call over one reception: the ESI range [lo, hi] that is walked (lo > hi: empty) */
struct wn_q {
  uint32_t source, extra, lo, hi;
};

ING_HD struct wn_q wn_query(const struct ing_rx *r, uint32_t flags, uint32_t extra, uint32_t esi_from) {
  struct wn_q q;
  q.source = flags & WN_SOURCE;
  q.extra = extra;
  q.lo = q.source ? 0u : (esi_from > r->K ? esi_from : r->K);
  q.hi = q.source ? r->K - 1u : r->max_esi; /* (the bitmap's last word has bits above max_esi: never set, never to be asked for) */
  return q;
}

/* the seen words [wn_first, wn_end) cover the range */
ING_HD uint32_t wn_first(const struct wn_q *q) { return q->lo >> 5; }
ING_HD uint32_t wn_end(const struct wn_q *q) { return q->lo > q->hi ? q->lo >> 5 : (q->hi >> 5) + 1u; }

/* tags block b lists at most: what it lacks, less the repair rows it has, no more than its free repair rows can take */
ING_HD uint32_t wn_need(const struct ing_rx *r, const struct wn_q *q, uint32_t b) {
  const uint32_t g = r->gaps[b];
  if (g == 0 || q->source) return g;
  const uint32_t rr = hl_nrep(r, b), want = g + q->extra, free_rows = r->rep_cap - rr;
  const uint32_t need = want > rr ? want - rr : 0u;
  return need < free_rows ? need : free_rows;
}

/* the wanted ESIs of word w (wn_first <= w < wn_end) of block b: the clear seen bits, without those below lo and above hi */
ING_HD uint32_t wn_bits(const struct ing_rx *r, const struct wn_q *q, uint32_t b, uint32_t w) {
  uint32_t m = ~r->seen[(uint64_t)b * r->bm_words + w];
  if (w == q->lo >> 5) m &= 0xFFFFFFFFu << (q->lo & 31u);
  if (w == q->hi >> 5) m &= 0xFFFFFFFFu >> (31u - (q->hi & 31u));
  return m;
}

/* the tags of word w's wanted ESIs (`bits` = wn_bits), ascending, to out[rank ..] -- `rank` = wanted ESIs of the block below this
 * word, `out` = the block's place in the list -- as far as their rank stays below need */
ING_HD void wn_put(const struct ing_rx *r, uint32_t b, uint32_t w, uint32_t bits, uint32_t rank, uint32_t need, uint32_t *out) {
  while (bits && rank < need) {
    out[rank++] = ((r->sbn0 + b) << 24) | (w * 32u + ing_lowbit(bits));
    bits &= bits - 1u;
  }
}

#endif /* NRQ_WANT_BODY_H */
