/*
 * out_view_emu.cpp -- the host's builder of the out view's image (plan.h off_wout) behind a C entry point (TEST SUPPORT ONLY).
 * nanorq_amd/csrc/out_lists.h is host code as it is (host-planned decodes of nrq_device.hip): no emulation.  The tests hold the
 * image against the plan's own W rows and against the one the device planner's emulation leaves (tests/emu/planner_emu.cpp).
 */
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../nanorq_amd/csrc/out_lists.h"

/* the image of the n lists (cptr[n + 1], cols[]) over a host-built plan: wpr * ((n + 63) & ~63) words into wout[]; returns the
 * words, ~0 when they do not fit cap_words */
extern "C" uint32_t emu_out_w(const uint8_t *plan, uint32_t n, const uint32_t *cptr, const uint16_t *cols, uint32_t *wout,
                              uint32_t cap_words) {
  std::vector<uint32_t> cp(cptr, cptr + n + 1), w;
  std::vector<uint16_t> cl(cols, cols + cptr[n]);
  build_out_w(plan, cp, cl, w);
  if (w.size() > cap_words) return ~0u;
  if (!w.empty()) memcpy(wout, w.data(), w.size() * 4);
  return (uint32_t)w.size();
}
