/*
 * solve_roles.h -- what an instance nrq_solve_kernel<WB, NT, WV, G, AL> decides about itself, stated once: the role knobs (each
 * with the measurement behind its value), solve_roles() -- the waves that run the forward passes, gather and scatter, the movers'
 * form, the op-word ring, the HDPC threads, the late parts, the compiled forms of the phases --, the rules for one wave and one
 * strip index, and whether such an instance can work at all.  nrq_solve_kernel (nrq_device.hip), the launch emulation
 * (tests/emu/launch_emu.cpp) and the row-pipeline probe (tests/gpu/rows_probe.hip) all read this file: who moves what in which
 * window is changed here alone.  Host- and device-compilable, no HIP include.
 */
#ifndef NRQ_SOLVE_ROLES_H
#define NRQ_SOLVE_ROLES_H

#include <stdint.h>

#include "plan.h"
/* ---- the forward window: NFW waves run the forward passes (two, half the strip width each, when the strip is wide enough and
 * the workgroup big enough to spare a second SIMD); the waves on the other SIMDs move data meanwhile: NGW gather, NSW scatter ---- */
#ifndef NRQ_W12_FW
#define NRQ_W12_FW 3 /* forward waves of the 12-byte strip: 3 (a dword each) or 2 (two dwords, one dword) */
#endif
#ifndef NRQ_W12_GW
#define NRQ_W12_GW 2 /* gather / scatter waves beside the three forward waves of the 12-byte strip */
#endif
#ifndef NRQ_W12_SW
#define NRQ_W12_SW 2
#endif
#ifndef NRQ_GATHER_WAVES_NARROW
#define NRQ_GATHER_WAVES_NARROW 2u /* gather waves of the 768-thread workgroup on strips of at most NRQ_GATHER_WAVES_NARROW_WB bytes */
#endif
#ifndef NRQ_GATHER_WAVES_NARROW_WB
#define NRQ_GATHER_WAVES_NARROW_WB 2
#endif
#ifndef NRQ_MOVER_WAVES
#define NRQ_MOVER_WAVES 2u
#endif
#ifndef NRQ_PIPE_SMALL
#define NRQ_PIPE_SMALL 0 /* (round 3: with the movers' aligned-only form the software-pipelined loops of the 256-thread variant keep so many
                          * requests in flight that its forward wave waits for its op words: K=1000 9.7 / 8.6 ms with them, 8.2 / 7.7 without;
                          * K=500 14.6 / 13.4 vs 12.4 / 11.8; K=2000 8.5 / 7.3 vs 7.2 / 6.5) */
#endif
/* software-pipelined data movers in the 768-thread workgroup (168 registers per thread); the 256-thread variant had them in
 * round 2 (K=1000 977 -> 1031 Gbit/s with the loops as they were then), see NRQ_PIPE_SMALL */
#ifndef NRQ_PIPE_BIG
#define NRQ_PIPE_BIG 1
#endif
/* ---- op-word ring of the forward wave(s), in rows: what the variant's register budget holds without spilling ---- */
#ifndef NRQ_RING_TINY
#define NRQ_RING_TINY 24u /* the single-wave variant: a dozen workgroups per CU hide each other's op-word latency, and a short ring is less code for
                           * them to share the instruction cache with (K=100 T=1024 / K=256, ring 60 / 36 / 24 / 12 rows: 460 / 468 / 471 / 473 and
                           * 815 / 833 / 835 / 836 Gbit/s; the 256-thread variant loses with a shorter ring: K=1000 1156 / 1093 / 1087 / 1057) */
#endif
#ifndef NRQ_RING_4W
#define NRQ_RING_4W NRQ_RING
#endif
#ifndef NRQ_RING_5W
#define NRQ_RING_5W 36u /* five waves per SIMD: 102 registers per thread */
#endif
#ifndef NRQ_BIG_RING
#define NRQ_BIG_RING NRQ_RING_MAX /* op-word ring (rows) of the two forward waves of the 768-thread workgroup */
#endif
/* ---- the HDPC phase ---- */
#ifndef NRQ_HDPC_NT
#define NRQ_HDPC_NT 512 /* threads of the HDPC phase; measured: 256 / 512 / 768 -> 34 k / 28 k / 29 k clocks (the closing fold is per thread) */
#endif
/* (the 256-thread variant: NRQ_HDPC_NT_SMALL threads -- every thread of the phase ends in a closing fold of 8 x H masked XORs,
 * ~800 instructions whatever its chunk holds, and four such workgroups share a CU's issue slots) */
#ifndef NRQ_HDPC_NT_SMALL
#define NRQ_HDPC_NT_SMALL 256
#endif
/* (narrow strips: the H sums in registers -- on 16-byte strips that form is slower, 24 k against 17.5 k clocks for the
 * recurrence: 4 x H operations per column instead of four LDS atomics) */
#ifndef NRQ_HDPC_REGS_MAX_WB
#define NRQ_HDPC_REGS_MAX_WB 4
#endif
#ifndef NRQ_HDPC_REGS_12
#define NRQ_HDPC_REGS_12 0
#endif
/* ---- the late parts: part of the scatter portion is left to the waves that the HDPC phase does not use (when there are any) ---- */
#ifndef NRQ_SCATTER_LATE_PCT
#define NRQ_SCATTER_LATE_PCT 20u
#endif
/* ... and part of the gather portion: the gather of an encode strip is bound by its bytes in flight against the memory
 * latency and ends with the forward waves (more of it in flight there would delay their op words); in the HDPC window
 * nobody waits for op words.  K=8192 T=1280, encode / decode solve kernel in ms at gather % / scatter %: 0/35 7.09 / 6.28,
 * 40/20 6.61 / 6.30, 35/35 6.79 / 6.25, 50/25 6.82 / 6.37, 60/35 7.02 / 6.34 (beyond 40 % the HDPC window grows by more
 * than the forward window shrinks) */
#ifndef NRQ_GATHER_LATE_PCT
#define NRQ_GATHER_LATE_PCT 40u
#endif
#ifndef NRQ_SCATTER_LATE_PCT_NARROW
#define NRQ_SCATTER_LATE_PCT_NARROW 10u
#endif
#ifndef NRQ_GATHER_LATE_PCT_NARROW
#define NRQ_GATHER_LATE_PCT_NARROW 15u
#endif
#ifndef NRQ_W12_SLATE
#define NRQ_W12_SLATE NRQ_SCATTER_LATE_PCT
#endif
#ifndef NRQ_W12_GLATE
#define NRQ_W12_GLATE NRQ_GATHER_LATE_PCT
#endif
#ifndef NRQ_FOLD_PRE256
#define NRQ_FOLD_PRE256 0 /* coefficients the 256-thread variant's dense fold asks for at once (0: one per term, a trip to L2 each) */
#endif

struct SolveRoles {
  uint32_t WBE, VNT;           /* bytes of a strip; virtual threads (G lanes each) */
  bool ALX;                    /* the movers compiled without their byte-wise forms */
  uint32_t NFW, NMV, NGW, NSW; /* forward waves; waves that share no SIMD with them; of those (NFW == 3: of all other waves) gather, scatter */
  bool MPIPE;                  /* software-pipelined movers */
  uint32_t RU, HNT;            /* op-word ring in rows; threads of the HDPC phase */
  bool LATE;                   /* the HDPC phase leaves waves idle: they move the late parts of the portions, */
  uint32_t SLATE, GLATE;       /* this many percent of the scatter and of the gather portion */
  /* the compiled form of the phases: ph_hdpc<REGS>, ph_dense_fold<BATCH>, ph_dense_free / ph_dense_cu <BATCH>,
   * ph_backsub / ph_store <FAST>, pf_commit<PB> */
  bool hdpc_regs, batch, fast;
  int fold_batch, commit_pb;
};

constexpr SolveRoles solve_roles(int WB, int NT, int WV, int G, bool AL) {
  SolveRoles r{};
  const uint32_t nt = (uint32_t)NT, wb = (uint32_t)WB, hdpc_nt = (uint32_t)NRQ_HDPC_NT;
  r.WBE = wb * (uint32_t)G;
  r.VNT = nt / (uint32_t)G;
  r.ALX = AL && G == 1 && WB >= 4;
  r.NFW = (G == 1 && WB == 12 && NT >= 512) ? (uint32_t)NRQ_W12_FW : (G == 1 && WB >= 8 && NT >= 512) ? 2u : 1u;
  r.NMV = (nt / 64u) / 4u * (4u - r.NFW) + ((nt / 64u) % 4u > r.NFW ? (nt / 64u) % 4u - r.NFW : 0u);
  /* two gather and two scatter waves in the big workgroup, not three: every mover wave that keeps loads in
   * flight slows the forward waves' op words down (measured, headline encode: 3+3 -> row pipeline 89 k clocks,
   * gather done at 70 k; 2+2 -> 79 k / 83 k; 1+1 -> 72 k / 125 k) */
  /* (2-byte strips: the GATHER, not the forward wave, ends the window -- with work slots of 8 strips a row piece is
   * 16 bytes of a 128-byte line and the two gather waves are bound by their requests in flight; round 6, NRQ_PROF
   * marks at K'=56403: forward wave done 77 k clocks before the window's end, gather at its end) */
  /* (12-byte strips: three forward waves leave one SIMD free of them, three waves -- two gathering and one scattering
   * ended the forward window at 1.5 x (encode) and 2.7 x (decode) the forward waves' own time at K=10000; so the
   * movers are NRQ_W12_GW + NRQ_W12_SW of ALL nine other waves, the free SIMD's first) */
  r.NGW = r.NFW == 3u ? (uint32_t)NRQ_W12_GW : r.NMV >= 6u ? (WB <= NRQ_GATHER_WAVES_NARROW_WB ? NRQ_GATHER_WAVES_NARROW : NRQ_MOVER_WAVES) : r.NMV >= 3u ? 2u : 1u;
  r.NSW = r.NFW == 3u ? (uint32_t)NRQ_W12_SW : r.NMV >= 6u ? NRQ_MOVER_WAVES : r.NMV - r.NGW;
  r.MPIPE = (NRQ_PIPE_BIG && NT >= 512) || (NRQ_PIPE_SMALL && NT == 256 && WV == 4);
  r.RU = NT >= 512 ? NRQ_BIG_RING : NT == 64 ? NRQ_RING_TINY : WV >= 5 ? NRQ_RING_5W : NRQ_RING_4W;
  r.HNT = NT == 256 ? (uint32_t)NRQ_HDPC_NT_SMALL : nt < hdpc_nt ? nt : hdpc_nt;
  r.LATE = nt > hdpc_nt;
  r.SLATE = WB == 12 ? NRQ_W12_SLATE : WB >= 8 ? NRQ_SCATTER_LATE_PCT : NRQ_SCATTER_LATE_PCT_NARROW;
  r.GLATE = WB == 12 ? NRQ_W12_GLATE : WB >= 8 ? NRQ_GATHER_LATE_PCT : NRQ_GATHER_LATE_PCT_NARROW;
  r.hdpc_regs = NT >= 512 && G == 1 && (WB <= NRQ_HDPC_REGS_MAX_WB || (WB == 12 && NRQ_HDPC_REGS_12));
  r.fold_batch = NT == 64 ? 8 : NT == 256 ? NRQ_FOLD_PRE256 : 0;
  r.batch = NT == 64;
  r.fast = NT >= 512;
  r.commit_pb = NT == 64 ? 4 : 8;
  return r;
}

/* wide strips are made of 16-byte lanes; 12-byte strips run in the 768-thread workgroup only (blocks whose 16-byte image does
 * not fit the LDS); a workgroup of more than one wave needs a gather and a scatter wave */
constexpr bool solve_roles_valid(int WB, int NT, int WV, int G, bool AL) {
  return (G == 1 || WB == 16) && (WB != 12 || NT >= 512) && (solve_roles(WB, NT, WV, G, AL).NMV >= 2u || NT == 64);
}

/* The rules for one wave and one strip index are macros, not functions: nrq_solve_kernel expands them on its compile-time
 * constants and the compiler folds them where it folded the expressions they replace (a function, even one always inlined, changed
 * the kernels' register allocation); the launch emulation expands them on the fields of a run-time SolveRoles. */
/* Wave wv >= NFW while the NFW forward waves run.  NRQ_WAVE_MOVES: it shares no SIMD with a forward wave (three forward waves:
 * every other wave counts); NRQ_MOVER_INDEX: its index among those -- below NGW that gather wave, below NGW + NSW scatter wave
 * (index - NGW), beyond that idle like the rest. */
#define NRQ_WAVE_MOVES(NFW, wv) (((wv) & 3u) >= (NFW) || (NFW) == 3u)
#define NRQ_MOVER_INDEX(NFW, wv)                                                                                                 \
  ((NFW) == 3u ? (((wv) & 3u) == 3u ? ((wv) >> 2) : ((wv) >> 2) * 3u + ((wv) & 3u)) /* (SIMD 3's: 0-2; waves 4-6, 8-10: 3-8) */ \
               : ((wv) >> 2) * (4u - (NFW)) + ((wv) & 3u) - (NFW))
/* Strip index sidx of a work slot's 1 << lsub moves the units [u0, u1) = [NRQ_PORTION_AT(.., sidx, ..), NRQ_PORTION_AT(.., sidx + 1, ..))
 * of its gather or scatter; from NRQ_PORTION_LATE_AT on, pct percent of them, they wait for the waves the HDPC phase leaves idle
 * (late: there are such waves, SolveRoles::LATE). */
#define NRQ_PORTION_AT(units, sidx, lsub) ((uint32_t)(((uint64_t)(units) * (sidx)) >> (lsub)))
#define NRQ_PORTION_LATE_AT(u0, u1, pct, late) ((late) ? (u1) - (uint32_t)((uint64_t)((u1) - (u0)) * (pct) / 100u) : (u1))

#endif /* NRQ_SOLVE_ROLES_H */
