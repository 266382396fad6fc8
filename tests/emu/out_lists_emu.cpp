/*
 * out_lists_emu.cpp -- the host's builder of a solve job's output lists behind a C entry point (TEST SUPPORT ONLY).
 * nanorq_amd/csrc/out_lists.h is host code as it is (encode calls and host-planned decodes of nrq_device.hip): no emulation.
 * The tests hold its lists against the ones the device planner's emulation leaves (tests/emu/planner_emu.cpp).
 */
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../nanorq_amd/csrc/out_lists.h"

/* cptr[n + 1], order[n], at most cols_cap entries of cols[]; returns the entries, ~0 when they do not fit or K is no block size */
extern "C" uint32_t emu_out_lists(uint32_t K, uint32_t Kp_hint, const uint16_t *colslot, uint32_t n, const uint32_t *isis,
                                  uint32_t *cptr, uint16_t *cols, uint32_t cols_cap, uint32_t *order) {
  rq_params p;
  if (!rq_params_init(Kp_hint ? Kp_hint : K, &p)) return ~0u;
  p.K = K;
  std::vector<uint32_t> cp, ord;
  std::vector<uint16_t> cl;
  build_out_lists(p, colslot, n, isis, cp, cl, ord);
  if (cl.size() > cols_cap) return ~0u;
  memcpy(cptr, cp.data(), cp.size() * 4);
  if (n) memcpy(order, ord.data(), (size_t)n * 4);
  if (!cl.empty()) memcpy(cols, cl.data(), cl.size() * 2);
  return (uint32_t)cl.size();
}
