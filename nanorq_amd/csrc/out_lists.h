/* The output lists of a solve job, built on the host: what nrq_job's out_cptr / out_slots / out_row name (solve_body.h, ph_store).
 * Host code only; nrq_device.hip builds the lists of an encode call and of a host-planned decode with it, the CPU tier checks it
 * against the device planner's lists (planner_body.h, pl_final_d / pl_final_e). */
#ifndef NRQ_OUT_LISTS_H
#define NRQ_OUT_LISTS_H
#include <stdint.h>
#include <string.h>
#include <vector>
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

#endif
