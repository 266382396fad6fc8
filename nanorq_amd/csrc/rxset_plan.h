/*
 * rxset_plan.h -- which blocks one nrq_rxset_decode or nrq_rx_decode (a set of one member) decodes, and in which decode calls.
 *
 *   rxset_selected()   whether a block is decoded now
 *   rxset_nuse()       the repair symbols such a block hands the decode up front
 *   rxset_plan()       the selected blocks of a set as chunks of one (K, K', has_relay) each
 *
 * Values in, a record out: no context, no runtime call, so the host compiler builds it on its own (rxset_lists_emu.cpp,
 * tests/test_rxset_decode_emu.py); nrq_device.hip issues one nrq_decode_blocks_vi per chunk.
 */
#ifndef NRQ_RXSET_PLAN_H
#define NRQ_RXSET_PLAN_H

#include <stdint.h>

#include <vector>

/* blocks of one decode call at most: the largest batch the decode path has been put through (the tests, bench.py).  A set holds
 * up to 1024 blocks; a group beyond this is cut, the decode path's envelope is not widened here.  Not below 256: a reception has
 * up to 256 blocks, and nrq_rx_decode counts on them being ONE chunk, in block order (one decode call whose failure leaves no
 * block marked; nrq_device.hip asserts it). */
#define RXSET_CHUNK_BLOCKS 256u

struct rxset_plan_member {
  uint32_t K, Kp, max_esi;
  uint32_t has_relay; /* a relay is attached: its blocks' decode also writes the intermediate symbols */
};

/* one decode call: blocks[] are global block numbers, ascending, all of members of equal (K, Kp, has_relay) */
struct rxset_chunk {
  uint32_t K, Kp, has_relay;
  std::vector<uint32_t> blocks;
};

/* a block with ng missing source symbols and nr repair rows is decoded now (nanorq_repair_block's rules): it has gaps, at least
 * as many repair symbols as gaps, and no more extra symbols than the rows beyond L (max_esi - K) */
static inline bool rxset_selected(uint32_t ng, uint32_t nr, uint32_t K, uint32_t max_esi) {
  return ng != 0 && nr >= ng && nr - ng <= max_esi - K;
}

/* as the object layer: two extra symbols up front, the rest on demand */
static inline uint32_t rxset_nuse(uint32_t ng, uint32_t nr) { return nr - ng > 2u ? ng + 2u : nr; }

/* nb blocks in block order: member[j] indexes mem[], ng[j] / nr[j] are the block's counts.  The selected blocks, partitioned into
 * groups of equal (K, Kp, has_relay) in the order in which the groups first appear, every group cut into chunks of at most
 * `chunk` blocks (0: RXSET_CHUNK_BLOCKS); inside a chunk the blocks are in block order. */
static inline std::vector<rxset_chunk> rxset_plan(const rxset_plan_member *mem, const uint32_t *member, const uint32_t *ng, const uint32_t *nr,
                                                  uint32_t nb, uint32_t chunk = 0) {
  if (!chunk) chunk = RXSET_CHUNK_BLOCKS;
  std::vector<rxset_chunk> groups;
  for (uint32_t j = 0; j < nb; j++) {
    const rxset_plan_member &m = mem[member[j]];
    if (!rxset_selected(ng[j], nr[j], m.K, m.max_esi)) continue;
    const uint32_t rel = m.has_relay ? 1u : 0u;
    size_t g = 0;
    while (g < groups.size() && !(groups[g].K == m.K && groups[g].Kp == m.Kp && groups[g].has_relay == rel)) g++;
    if (g == groups.size()) groups.push_back(rxset_chunk{m.K, m.Kp, rel, {}});
    groups[g].blocks.push_back(j);
  }
  std::vector<rxset_chunk> out;
  for (const rxset_chunk &g : groups)
    for (size_t at = 0; at < g.blocks.size(); at += chunk) {
      const size_t end = at + chunk < g.blocks.size() ? at + chunk : g.blocks.size();
      out.push_back(rxset_chunk{g.K, g.Kp, g.has_relay, std::vector<uint32_t>(g.blocks.begin() + at, g.blocks.begin() + end)});
    }
  return out;
}

#endif /* NRQ_RXSET_PLAN_H */
