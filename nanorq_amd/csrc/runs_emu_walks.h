/* The workgroup walks of the listings as runs (rn_bits_wg / rn_rows_wg of nrq_device.hip) a round at a time, for the CPU emulations
 * of the single reception (runs_emu.cpp) and of the set (rxset_runs_emu.cpp): WN_ROUND words (rows) per round, one per "thread", the
 * workgroup's sum-scan and max-scan done in loops, the run start, the symbols found and the packets placed carried from round to
 * round; the per-word and per-row bodies are the ones the kernels run (runs_body.h).  Test support, not part of the library. */
#ifndef NRQ_RUNS_EMU_WALKS_H
#define NRQ_RUNS_EMU_WALKS_H

#include <stdint.h>

#include <algorithm>

#include "runs_body.h"

/* rn_bits_wg, a round at a time: tags NULL counts (returns the packets, *syms the symbols), else the packets go to tags[at ..] /
 * nsym[at ..] (returns `at` behind them; RN_ALL: the two passes over a word disagree) */
static inline uint32_t bits_walk(const ing_rx *r, const rn_walk *k, uint32_t G, uint32_t *tags, uint8_t *nsym, uint32_t at, uint32_t *syms) {
  uint32_t found = 0, pk = 0, S = k->lo;
  uint32_t bits[WN_ROUND], ps[WN_ROUND], pm[WN_ROUND];
  for (uint32_t w0 = k->w_first; w0 < k->w_end && found < k->need; w0 += WN_ROUND) {
    uint32_t run = 0, mx = 0;
    for (uint32_t t = 0; t < WN_ROUND; t++) { /* the words, the inclusive sum-scan of their counts and max-scan of their marks */
      bits[t] = rn_word(r, k, w0 + t);
      run += ing_popc(bits[t]);
      mx = std::max(mx, rn_mark(w0 + t, bits[t]));
      ps[t] = run;
      pm[t] = mx;
    }
    uint32_t placed = 0;
    for (uint32_t t = 0; t < WN_ROUND; t++) {
      const uint32_t rank = found + ps[t] - ing_popc(bits[t]), Sin = std::max(S, t ? pm[t - 1u] : 0u);
      const uint32_t n = rn_word_pkts(r, k, G, w0 + t, bits[t], Sin, rank, nullptr, nullptr);
      if (tags && rn_word_pkts(r, k, G, w0 + t, bits[t], Sin, rank, tags + at + pk + placed, nsym + at + pk + placed) != n) return RN_ALL;
      placed += n;
    }
    pk += placed;
    found += ps[WN_ROUND - 1u];
    S = std::max(S, pm[WN_ROUND - 1u]);
  }
  if (syms) *syms = std::min(found, k->need);
  return tags ? at + pk : pk;
}

/* rn_rows_wg, a round at a time */
static inline uint32_t rows_walk(const ing_rx *r, uint32_t b, uint32_t G, uint32_t *tags, uint8_t *nsym, uint32_t at) {
  const uint32_t nrep = hl_nrep(r, b);
  uint32_t pk = 0, M = 0, pm[WN_ROUND];
  for (uint32_t q0 = 0; q0 < nrep; q0 += WN_ROUND) {
    uint32_t mx = 0;
    for (uint32_t t = 0; t < WN_ROUND; t++) { mx = std::max(mx, rn_rep_mark(r, b, q0 + t, nrep)); pm[t] = mx; }
    for (uint32_t t = 0; t < WN_ROUND; t++) {
      if (!rn_rep_starts(q0 + t, nrep, std::max(M, pm[t]) - 1u, G)) continue;
      if (tags) rn_rep_put(r, b, q0 + t, nrep, G, tags + at + pk, nsym + at + pk);
      pk++;
    }
    M = std::max(M, pm[WN_ROUND - 1u]);
  }
  return tags ? at + pk : pk;
}

#endif
