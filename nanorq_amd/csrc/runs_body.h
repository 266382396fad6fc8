/*
 * runs_body.h -- the request side of packets of several symbols (syms_body.h): the want and held listings as RUNS
 * (nrq_rx_want_syms / nrq_rx_held_syms and their object forms, include/nanorq_hip.h) and the admission of a held emit of such
 * packets (NRQ_TX_HELD in nrq_tx_emit_syms / nrq_otx_emit_syms), built over want_body.h, held_body.h and syms_body.h.
 *
 * The packetisation of a list.  Take the tag list L of one block as the one-symbol listing gives it (want_body.h, held_body.h), in
 * that order.  A RUN is a maximal stretch L[i..j] with L[i+m] == L[i] + m; the source part and the repair part of a held list are
 * lists of their own (nothing joins ESI K-1 to ESI K).  Every run is cut into packets of G from its START, the last one short; a
 * packet is (first tag, count).  The expansion of the result (syms_body.h) is L word for word.
 *
 * Two walks give every list there is:
 *   bitmap walk (rn_walk)  the listed ESIs are the set bits of a word function over [w_first, w_end), the first `need` of them:
 *                          want in both modes (wn_bits), and the source part of held (hl_have, need = all).  The run of a listed
 *                          ESI starts one above the nearest NOT listed ESI below it (or at lo).
 *   row walk               the repair part of held: position = the row index q, a run breaks where rep_esi[q] != rep_esi[q-1] + 1
 *                          (arrival order: a run lies in consecutive rows).
 * A listed item starts a packet iff (its position - its run's start) % G == 0; the packet's count is min(G, what is left of the
 * run, what is left of `need`).
 *
 * nrq_device.hip runs them in the count / scan / fill shape of the one-symbol listings: one workgroup of 256 per block, rounds of
 * WN_ROUND words (rows).  Per round a sum-scan over the words' popcounts gives each word the rank of its first listed ESI, a
 * max-scan over the words' marks (rn_mark: one above the word's highest not listed ESI) the run start entering it; the run start,
 * the symbols found and the packets placed are CARRIED ACROSS ROUNDS.  A packet's count looks ahead in the books (rn_ahead,
 * rn_rep_ahead: at most G - 1 positions, whatever round they lie in).  runs_emu.cpp runs the same bodies in the same rounds.
 *
 * The held emit.  A packet of a block that is not ready is written iff EVERY symbol e .. e+c-1 is held -- all or nothing: no packet
 * is ever half written -- as copies of source rows e .. e+c-1, or of the repair rows found for the c ESIs in one walk over the
 * block's repair list.  hs_packet is the packet-level part of the admission, hs_slot_held the per-symbol part.
 */
#ifndef NRQ_RUNS_BODY_H
#define NRQ_RUNS_BODY_H

#include <stdint.h>

#include "held_body.h"
#include "ingest_body.h"
#include "syms_body.h"
#include "want_body.h"

#define RN_ALL 0xFFFFFFFFu /* need of a walk that lists every set bit */

/* leading zeros of v (v != 0) */
ING_HD uint32_t rn_clz(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__clz((int)v);
#else
  return (uint32_t)__builtin_clz(v);
#endif
}

/* ---- the bitmap walk ---- */
/* one block's walk: the listed ESIs are the set bits of rn_word over the words [w_first, w_end), from ESI lo, the first `need` */
struct rn_walk {
  uint32_t held;          /* 0: what the block wants (q); 1: the source symbols it holds */
  uint32_t b, lo, w_first, w_end, need;
  struct wn_q q;
};

ING_HD struct rn_walk rn_walk_want(const struct ing_rx *r, const struct wn_q *q, uint32_t b) {
  struct rn_walk k;
  k.held = 0u; k.b = b; k.q = *q;
  k.lo = q->lo; k.w_first = wn_first(q); k.w_end = wn_end(q); k.need = wn_need(r, q, b);
  return k;
}

ING_HD struct rn_walk rn_walk_held(const struct ing_rx *r, uint32_t b) {
  struct rn_walk k;
  k.held = 1u; k.b = b;
  k.q.source = 1u; k.q.extra = 0u; k.q.lo = 0u; k.q.hi = r->K - 1u;
  k.lo = 0u; k.w_first = 0u; k.w_end = ing_src_words(r); k.need = RN_ALL;
  return k;
}

/* the listed ESIs of word w; a word outside [w_first, w_end) lists nothing (and is not read) */
ING_HD uint32_t rn_word(const struct ing_rx *r, const struct rn_walk *k, uint32_t w) {
  if (w < k->w_first || w >= k->w_end) return 0u;
  return k->held ? hl_have(r, k->b, w) : wn_bits(r, &k->q, k->b, w);
}

/* the word's mark for the max-scan: one above its highest NOT listed ESI -- where a run that reaches past the word starts at the
 * earliest; 0 for a word whose 32 ESIs are all listed (it hands the run start it was given on) */
ING_HD uint32_t rn_mark(uint32_t w, uint32_t bits) { return bits == 0xFFFFFFFFu ? 0u : w * 32u + 32u - rn_clz(~bits); }

/* listed ESIs in a row from ESI e (listed itself) on, G at the most: the rest of e's run, wherever its words lie */
ING_HD uint32_t rn_ahead(const struct ing_rx *r, const struct rn_walk *k, uint32_t e, uint32_t G) {
  uint32_t c = 0, w = e >> 5, sh = e & 31u;
  while (c < G) {
    const uint32_t inv = ~(rn_word(r, k, w) >> sh); /* (the bits shifted in are zeros: they end the count at the word's end) */
    const uint32_t ones = inv ? ing_lowbit(inv) : 32u;
    c += ones;
    if (ones < 32u - sh) break;
    w++;
    sh = 0u;
  }
  return c < G ? c : G;
}

/* The packets that START in word w of the walk: `bits` = rn_word, S = the run start entering the word (for its ESI w * 32), rank =
 * listed ESIs of the block below the word.  Returns their number; with tags not NULL they are written, ascending, to tags[0 ..]
 * and nsym[0 ..].  Only ESIs of rank below need are listed. */
ING_HD uint32_t rn_word_pkts(const struct ing_rx *r, const struct rn_walk *k, uint32_t G, uint32_t w, uint32_t bits, uint32_t S,
                             uint32_t rank, uint32_t *tags, uint8_t *nsym) {
  uint32_t n = 0, m = bits;
  while (m && rank < k->need) {
    /* the stretch of set bits from bit p: ESIs e0 .. e0+len-1, of a run that starts at `start` */
    const uint32_t p = ing_lowbit(m), inv = ~(m >> p);
    const uint32_t len = inv ? ing_lowbit(inv) : 32u;
    const uint32_t e0 = w * 32u + p, start = p ? e0 : S;
    const uint32_t room = k->need - rank, end = e0 + (len < room ? len : room);
    const uint32_t first = e0 + (G - (e0 - start) % G) % G; /* the first ESI of the stretch that starts a packet */
    if (first < end) {
      if (!tags) {
        n += (end - 1u - first) / G + 1u;
      } else {
        for (uint32_t e = first; e < end; e += G) {
          const uint32_t left = k->need - (rank + (e - e0)), run = rn_ahead(r, k, e, G);
          tags[n] = ((r->sbn0 + k->b) << 24) | e;
          nsym[n] = (uint8_t)(run < left ? run : left);
          n++;
        }
      }
    }
    rank += len;
    m = p + len >= 32u ? 0u : m & (0xFFFFFFFFu << (p + len));
  }
  return n;
}

/* ---- the row walk: the repair part of a held list ---- */
/* row q (below hl_nrep) of block b begins a run */
ING_HD bool rn_rep_break(const struct ing_rx *r, uint32_t b, uint32_t q) {
  const uint32_t *e = r->rep_esi + (uint64_t)b * r->rep_cap;
  return q == 0u || e[q] != e[q - 1u] + 1u;
}

/* the row's mark for the max-scan: q + 1 where a run begins, else 0 -- the inclusive maximum up to a row, less one, is the row
 * its run starts at (row 0 always begins one) */
ING_HD uint32_t rn_rep_mark(const struct ing_rx *r, uint32_t b, uint32_t q, uint32_t nrep) {
  return q < nrep && rn_rep_break(r, b, q) ? q + 1u : 0u;
}

/* rows in a row from row q on whose ESIs are consecutive, G at the most: the rest of q's run */
ING_HD uint32_t rn_rep_ahead(const struct ing_rx *r, uint32_t b, uint32_t q, uint32_t nrep, uint32_t G) {
  uint32_t c = 1u;
  while (c < G && q + c < nrep && !rn_rep_break(r, b, q + c)) c++;
  return c;
}

/* does row q, whose run starts at row `start`, begin a packet */
ING_HD bool rn_rep_starts(uint32_t q, uint32_t nrep, uint32_t start, uint32_t G) { return q < nrep && (q - start) % G == 0u; }

/* the packet that begins at row q */
ING_HD void rn_rep_put(const struct ing_rx *r, uint32_t b, uint32_t q, uint32_t nrep, uint32_t G, uint32_t *tag, uint8_t *nsym) {
  *tag = hl_rep_tag(r, b, q);
  *nsym = (uint8_t)rn_rep_ahead(r, b, q, nrep, G);
}

/* ---- the held emit of packets of several symbols ---- */
/* The packet-level part of the admission of packet k (first tag `tag`): its segment, or TX_SEGS when it stays untouched for what
 * *code says (TX_FOREIGN, TX_BAD_RANGE).  *cnt = its symbols, *ready = its block's ready bit.  A ready block's packet is then
 * written as without the flag; one of a block that is not ready iff hs_slot_held says yes for each of its cnt symbols (else
 * TX_NOT_READY). */
template <bool MULTI>
TX_HD uint32_t hs_packet(const struct tx_src *s, const struct sy_tx *y, uint32_t tag, uint32_t k, int32_t *code, uint32_t *cnt, uint32_t *ready) {
  const uint32_t g = tx_seg<MULTI>(s, tag);
  *cnt = 0u;
  *ready = 0u;
  if (g == TX_SEGS) { *code = TX_FOREIGN; return TX_SEGS; }
  const struct tx_blk t = tx_pick(s, MULTI ? g : 0u);
  *cnt = sy_tx_count(t.K, tag & SY_ESI_MAX, y->G, y->nsym, k);
  if (*cnt == 0u) { *code = TX_BAD_RANGE; return TX_SEGS; }
  *ready = tx_ready(s, tag);
  *code = 0;
  return g;
}

/* does the reception behind segment h hold ESI `esi` of its block b (nrq_rx_held's meaning: the seen bit) */
TX_HD bool hs_slot_held(const struct tx_held_seg *h, uint32_t b, uint32_t esi) { return tx_held_seen(h, b, esi) != 0u; }

#endif /* NRQ_RUNS_BODY_H */
