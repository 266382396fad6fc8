/* nrq_ings_lists_scan_kernel for the CPU emulations of the sets' listings (rxset_want_emu.cpp, rxset_runs_emu.cpp): n entries in
 * place, a run of entries per thread of the one workgroup, a scan over the threads' sums.  Test support, not part of the library. */
#ifndef NRQ_EMU_SCAN_H
#define NRQ_EMU_SCAN_H

#include <stdint.h>

#include <algorithm>
#include <numeric>

static inline void emu_scan(uint32_t *cnt, uint32_t n) {
  uint32_t ps[256];
  const uint32_t per = (n + 255u) / 256u;
  for (uint32_t i = 0; i < 256u; i++) {
    const uint32_t j0 = std::min(n, i * per), j1 = std::min(n, j0 + per);
    ps[i] = (i ? ps[i - 1u] : 0u) + std::accumulate(cnt + j0, cnt + j1, 0u);
  }
  for (uint32_t i = 0; i < 256u; i++) {
    const uint32_t j0 = std::min(n, i * per), j1 = std::min(n, j0 + per);
    uint32_t run = i ? ps[i - 1u] : 0u;
    for (uint32_t j = j0; j < j1; j++) { const uint32_t v = cnt[j]; cnt[j] = run; run += v; }
  }
}

#endif
