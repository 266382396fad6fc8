/* CPU emulation of the listing of what a reception wants (want_body.h), in the rounds of nrq_want_count_kernel and
 * nrq_want_fill_kernel: WN_ROUND seen words per round, one per "thread", the workgroup's reduction and scan done in a loop.  The
 * argument check, the per-block need, the word masks and the placement are the bodies the gfx950 kernels run.  Test support, not
 * part of the library: build.build_want_emu() makes tests/emu/libwant_emu.so of it. */
#include <stdint.h>
#include <string.h>

#include <vector>

#include "want_body.h"

extern "C" {

/* The listing of one reception: prm = {K, nblk, sbn0, max_esi, rep_cap}; the count pass, the scan over the blocks, the fill pass.
 * *n = tags wanted; out (nullable) receives them when cap >= *n, else -1 and nothing written.  -1 too for arguments wn_check refuses. */
int emu_rx_want(const uint32_t *prm, const uint32_t *seen, const uint32_t *gaps, const uint32_t *nrep, uint32_t flags, uint32_t extra,
                uint32_t esi_from, uint32_t *out, uint32_t cap, uint32_t *n) {
  ing_rx r;
  memset(&r, 0, sizeof(r));
  r.K = prm[0]; r.nblk = prm[1]; r.sbn0 = prm[2]; r.max_esi = prm[3]; r.rep_cap = prm[4];
  r.m1 = r.max_esi + 1u;
  r.bm_words = r.max_esi / 32u + 1u;
  r.seen = const_cast<uint32_t *>(seen); r.gaps = const_cast<uint32_t *>(gaps); r.nrep = const_cast<uint32_t *>(nrep);
  *n = 0;
  if (wn_check(flags, extra, esi_from)) return -1;
  const wn_q q = wn_query(&r, flags, extra, esi_from);
  const uint32_t w_first = wn_first(&q), w_end = wn_end(&q);
  std::vector<uint32_t> off(r.nblk + 1u, 0);
  for (uint32_t b = 0; b < r.nblk; b++) { /* count: rounds until `need` wanted ESIs are found */
    const uint32_t need = wn_need(&r, &q, b);
    uint32_t found = 0;
    for (uint32_t w0 = w_first; w0 < w_end && found < need; w0 += WN_ROUND)
      for (uint32_t t = 0; t < WN_ROUND; t++)
        if (w0 + t < w_end) found += ing_popc(wn_bits(&r, &q, b, w0 + t));
    off[b] = found < need ? found : need;
  }
  uint32_t run_ = 0; /* scan */
  for (uint32_t b = 0; b <= r.nblk; b++) { const uint32_t v = off[b]; off[b] = run_; run_ += v; }
  *n = off[r.nblk];
  if (!out) return 0;
  if (cap < *n) return -1;
  for (uint32_t b = 0; b < r.nblk; b++) { /* fill: per round the words' counts, their inclusive scan, the placement */
    const uint32_t need = wn_need(&r, &q, b);
    uint32_t placed = 0, bits[WN_ROUND], ps[WN_ROUND];
    for (uint32_t w0 = w_first; w0 < w_end && placed < need; w0 += WN_ROUND) {
      uint32_t run = 0;
      for (uint32_t t = 0; t < WN_ROUND; t++) {
        bits[t] = w0 + t < w_end ? wn_bits(&r, &q, b, w0 + t) : 0u;
        run += ing_popc(bits[t]);
        ps[t] = run;
      }
      for (uint32_t t = 0; t < WN_ROUND; t++) wn_put(&r, b, w0 + t, bits[t], placed + ps[t] - ing_popc(bits[t]), need, out + off[b]);
      placed += ps[WN_ROUND - 1u];
    }
  }
  return 0;
}

} /* extern "C" */
