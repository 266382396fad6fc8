/* The output lists of a solve job, built on the host: what nrq_job's out_cptr / out_slots / out_row name (solve_body.h, ph_store).
 * Host code only; nrq_device.hip builds the lists of an encode call and of a host-planned decode with it, the CPU tier checks it
 * against the device planner's lists (planner_body.h, pl_final_d / pl_final_e). */
#ifndef NRQ_OUT_LISTS_H
#define NRQ_OUT_LISTS_H
#include <stdint.h>
#include <string.h>
#include <vector>
#include "plan.h"
#include "rq_math.h"

/* LT neighbour lists of the symbols to generate, already translated to LDS slots through the plan's
 * colslot[], in the layout ph_store() reads */
inline void build_out_lists(const rq_params &p, const uint16_t *colslot, uint32_t n, const uint32_t *isis,
                     std::vector<uint32_t> &cptr, std::vector<uint16_t> &cols, std::vector<uint32_t> &order) {
  /* The lists in non-increasing length, equal lengths in the order of isis[] (a stable counting sort, the order the device planner
   * gives them too: pl_final_d): ph_store deals the lists to its threads in the stored order, and the 64 lists of a wave are then
   * of near-equal length.  order[i] = the symbol of isis[] whose list is stored i-th: the caller names out_row[i] by it. */
  std::vector<uint32_t> at(n + 1);
  std::vector<uint16_t> byq;
  byq.reserve((size_t)n * 9);
  uint32_t tmp[RQ_MAX_LT_COLS], start[RQ_MAX_LT_COLS + 2] = {0};
  for (uint32_t q = 0; q < n; q++) {
    at[q] = (uint32_t)byq.size();
    const uint32_t m = rq_lt_columns(&p, isis[q], tmp);
    for (uint32_t k = 0; k < m; k++) byq.push_back(colslot[tmp[k]]); /* slot that holds C[col] */
    start[RQ_MAX_LT_COLS - m + 1]++; /* (bucket RQ_MAX_LT_COLS - m: the longest lists first) */
  }
  at[n] = (uint32_t)byq.size();
  for (uint32_t l = 0; l <= RQ_MAX_LT_COLS; l++) start[l + 1] += start[l];
  order.resize(n);
  for (uint32_t q = 0; q < n; q++) order[start[RQ_MAX_LT_COLS - (at[q + 1] - at[q])]++] = q;
  cptr.resize(n + 1);
  cols.resize(byq.size());
  uint32_t o = 0;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t q = order[i], m = at[q + 1] - at[q];
    cptr[i] = o;
    if (m) memcpy(&cols[o], &byq[at[q]], (size_t)m * 2);
    o += m;
  }
  cptr[n] = o;
}

/* The out view's image of such lists over a host-built plan (plan.h off_wout): word w of list q's row at [w * out_pad + q],
 * W'_q = XOR of the plan's W rows over the entries of list q that are a pivot's slot, entry for entry as cols[] holds them (an
 * inactive column's slot adds nothing: ph_park puts the column's value itself there).  Empty when the plan has no inactive column. */
inline void build_out_w(const uint8_t *plan, const std::vector<uint32_t> &cptr, const std::vector<uint16_t> &cols,
                        std::vector<uint32_t> &wout) {
  const nrq_plan_hdr *h = reinterpret_cast<const nrq_plan_hdr *>(plan);
  const uint32_t n = cptr.empty() ? 0u : (uint32_t)cptr.size() - 1u, wpr = h->wpr, opad = (n + 63u) & ~63u;
  wout.assign((size_t)wpr * opad, 0u);
  if (!wpr || !n) return;
  const uint16_t *pivslot = reinterpret_cast<const uint16_t *>(plan + h->off_pivslot);
  const uint32_t *wt = reinterpret_cast<const uint32_t *>(plan + h->off_wt);
  std::vector<uint32_t> pivot_of(h->M + h->r2 + 1u, 0xFFFFFFFFu); /* slot -> pivot */
  for (uint32_t k = 0; k < h->npiv; k++) pivot_of[pivslot[k]] = k;
  for (uint32_t q = 0; q < n; q++)
    for (uint32_t e = cptr[q]; e < cptr[q + 1]; e++) {
      const uint32_t k = pivot_of[cols[e]];
      if (k == 0xFFFFFFFFu) continue;
      for (uint32_t w = 0; w < wpr; w++) wout[(size_t)w * opad + q] ^= wt[(size_t)w * h->npiv_pad + k];
    }
}

#endif
