/*
 * solve_emu.cpp -- CPU emulation of the gfx950 solve workgroup (TEST SUPPORT ONLY).
 *
 * Compiles nanorq_amd/csrc/solve_body.h -- the exact per-thread phase functions the HIP kernel
 * runs -- with g++ and executes the 256 threads of each phase sequentially, with the workgroup
 * barriers of nrq_solve_kernel turned into loop boundaries.  It lets the non-GPU test tier
 * exercise strip indexing, the packed GF(256) arithmetic, the HDPC Horner evaluation and the
 * chunk/sync schedule against the oracle.  It is not part of the product and is never shipped in
 * libnanorq_hip.so.
 *
 * The split solve of narrow strips (emu_solve_split): the strips stop after the dense stage and hand Y and C_u to a work
 * buffer (ph_store_raw + the scatter), then split_body.h -- the bodies of nrq_backsub_kernel<SB> and nrq_collect_kernel --
 * runs for every workgroup of the grids the launch would use.  emu_backsub / emu_collect run those bodies on arrays of the
 * caller's.
 */
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

static uint32_t g_dense_shared_min_nt = 512; /* workgroup size from which the dense fold shares the multiples (kernel: 512) */
#define NRQ_DENSE_SHARED_MIN_NT g_dense_shared_min_nt
#include "../../nanorq_amd/csrc/solve_body.h"
#include "../../nanorq_amd/csrc/split_body.h"
#include "strip_emu.h" /* the phases of one strip, the split tail: shared with launch_emu.cpp */
extern "C" void emu_set_dense_shared_min_nt(uint32_t v) { g_dense_shared_min_nt = v; }
static int g_hdpc_regs = 0; /* 1: the HDPC phase in the form of the big workgroup (register accumulators) */
extern "C" void emu_set_hdpc_regs(int v) { g_hdpc_regs = v; }

/* ybuf: the block's work buffer of a split solve ((M + u) rows of T bytes); nullptr: the whole solve in the strip */
template <int WB> static int run_strip(const nrq_job &job, uint32_t T, uint32_t strip, const uint8_t *kc, std::vector<uint8_t> &ostage,
                                       uint8_t *ybuf = nullptr) {
  const uint32_t NT = 256;
  StripCtx<WB> c;
  c.job = &job;
  c.plan = reinterpret_cast<const uint8_t *>(job.plan);
  c.h = reinterpret_cast<const nrq_plan_hdr *>(c.plan);
  if (c.h->status) return 0;
  c.kc = kc;
  c.lay = nrq_lds_plan(c.h, WB);
  std::vector<uint8_t> lds(c.lay.total + 64, 0xA5); /* garbage-filled like real LDS */
  c.lds = reinterpret_cast<uint8_t *>((reinterpret_cast<uintptr_t>(lds.data()) + 15) & ~(uintptr_t)15);
  c.T = T;
  c.strip = strip;
  uint32_t rem = T - strip * WB;
  c.valid = rem < (uint32_t)WB ? rem : (uint32_t)WB;
  constexpr uint32_t SPL = nrq_group_strips(WB);
  const size_t stride = ((size_t)c.h->M * WB + 255u) & ~(size_t)255u;
  std::vector<uint8_t> stage(stride * SPL + 64, 0x5A);
  { /* the way the persistent kernel fills the image: the gathering threads bring the whole line group of this
     * strip into the per-strip staging buffers, then all threads copy this strip's buffer into the image (strip_phases) */
    GroupSrc<WB> g;
    g.rowsrc = gptr<uint32_t>(c.job->rowsrc); g.src = gptr<uint8_t>(c.job->src); g.rep = gptr<uint8_t>(c.job->rep);
    g.M = c.h->M; g.T = T; g.strip0 = (strip / SPL) * SPL; g.nstrips = (T + WB - 1) / WB; g.lsub = __builtin_ctz(SPL);
    const uint32_t np = NT - NRQ_ROW, units = g.M * SPL, half = units / 2;
    for (uint32_t p = 0; p < np; p++) pf_gather<WB>(g, stage.data(), stride, 0, half, p, np);   /* in two portions, */
    for (uint32_t p = 0; p < np; p++) pf_gather<WB, 1, true>(g, stage.data(), stride, half, units, p, np); /* as the kernel does */
  }
  const uint32_t nstrips = (T + WB - 1) / WB, ne = ybuf ? c.h->M + c.h->u : out_elems<WB>(c.job, c.h);
  const size_t ostride = ((size_t)ne * WB + 255u) & ~(size_t)255u;
  if (strip % SPL == 0) ostage.assign(ostride * SPL + 64, 0x3C);
  SolveRoles f = solve_roles(WB, NT, 4, 1, false); /* (overridden: the forms this emulation has always run, whatever the kernel's 256 threads run) */
  f.HNT = NT; f.hdpc_regs = g_hdpc_regs != 0; f.fold_batch = 8; f.batch = true; f.fast = true; f.commit_pb = 4;
  const int r = strip_phases<WB, 1>(&c, NT, f, stage.data() + (size_t)(strip % SPL) * stride, ostage.data() + (size_t)(strip % SPL) * ostride, ybuf != nullptr);
  if (r != 1) return r;
  if (ybuf) { /* the split solve: slot image and C_u, staged per strip, scattered to full-width rows of the work buffer */
    if (strip % SPL == SPL - 1 || strip + 1 == nstrips) {
      GroupDst<WB> g; /* (nrq_solve_kernel group_dst with a work buffer) */
      g.inter = ybuf; g.out = gptr_w<uint8_t>(c.job->out); g.orow = gptr<uint32_t>(c.job->out_row);
      g.ni = ne; g.nout = 0u; g.T = T; g.strip0 = (strip / SPL) * SPL; g.nstrips = nstrips; g.lsub = __builtin_ctz(SPL);
      const uint32_t np = NT - NRQ_ROW, units = ne * SPL, cut = units / 3;
      for (uint32_t p = 0; p < np; p++) pf_scatter<WB>(g, ostage.data(), ostride, 0, cut, p, np);
      for (uint32_t p = 0; p < np; p++) pf_scatter<WB, 1, true>(g, ostage.data(), ostride, cut, units, p, np);
    }
    return 1;
  }
  /* results: staged per strip, then scattered to the symbol rows a line group at a time */
  if (strip % SPL == SPL - 1 || strip + 1 == nstrips) {
    GroupDst<WB> g;
    g.inter = gptr_w<uint8_t>(c.job->inter); g.out = gptr_w<uint8_t>(c.job->out); g.orow = gptr<uint32_t>(c.job->out_row);
    g.ni = c.job->inter ? c.h->L : 0u; g.nout = c.job->nout; g.T = T; g.strip0 = (strip / SPL) * SPL; g.nstrips = nstrips; g.lsub = __builtin_ctz(SPL);
    const uint32_t np = NT - NRQ_ROW, units = ne * SPL, cut = units / 3;
    for (uint32_t p = 0; p < np; p++) pf_scatter<WB>(g, ostage.data(), ostride, 0, cut, p, np);
    for (uint32_t p = 0; p < np; p++) pf_scatter<WB, 1, true>(g, ostage.data(), ostride, cut, units, p, np);
  }
  return 1;
}

extern "C" uint32_t emu_lds_bytes(const uint8_t *plan, uint32_t wb) {
  return nrq_lds_plan(reinterpret_cast<const nrq_plan_hdr *>(plan), wb).total;
}

/* every pointer in `job` is a host pointer here */
extern "C" int emu_solve(const nrq_job *job, uint32_t T, uint32_t wb, const uint8_t *kc) {
  const uint32_t nstrips = (T + wb - 1) / wb;
  int r = 1;
  std::vector<uint8_t> ostage;
  for (uint32_t s = 0; s < nstrips && r; s++) {
    switch (wb) {
      case 16: r = run_strip<16>(*job, T, s, kc, ostage); break;
      case 12: r = run_strip<12>(*job, T, s, kc, ostage); break;
      case 8: r = run_strip<8>(*job, T, s, kc, ostage); break;
      case 4: r = run_strip<4>(*job, T, s, kc, ostage); break;
      case 2: r = run_strip<2>(*job, T, s, kc, ostage); break;
      default: return -1;
    }
  }
  return r;
}

/* ---- the second half of a split solve (split_body.h; run_backsub / run_collect: strip_emu.h) ---- */

extern "C" uint32_t emu_backsub_strip_of(uint32_t sb, uint32_t wg, uint32_t gridx) {
  return sb == 32 ? sp_strip_of<32>(wg, gridx) : sp_strip_of<16>(wg, gridx);
}
extern "C" void emu_backsub_chunk(uint32_t npiv, uint32_t chunk, uint32_t nchunks, uint32_t *k01) {
  sp_chunk_bounds(npiv, chunk, nchunks, &k01[0], &k01[1]);
}
/* the back-substitution of one block on the caller's plan and work buffer, strips of sb bytes, grid ((T + sb - 1) / sb, nchunks) */
extern "C" int emu_backsub(const uint8_t *plan, uint8_t *Y, uint32_t T, uint32_t sb, uint32_t nchunks) {
  if (sb != 32 && sb != 16) return -1;
  const uint32_t gridx = (T + sb - 1) / sb;
  return sb == 32 ? run_backsub<32>(plan, Y, T, gridx, nchunks) : run_backsub<16>(plan, Y, T, gridx, nchunks);
}
/* the results of one block from the caller's slot image */
extern "C" int emu_collect(const nrq_job *job, uint32_t T, const uint8_t *F, uint32_t grid_e) { return run_collect(job, T, F, grid_e); }

/* the split solve of one block at strip width wb (4 or 2): every pointer in `job` is a host pointer */
extern "C" int emu_solve_split(const nrq_job *job, uint32_t T, uint32_t wb, const uint8_t *kc, uint32_t sb, uint32_t nchunks) {
  const uint8_t *plan = reinterpret_cast<const uint8_t *>(job->plan);
  const nrq_plan_hdr *h = reinterpret_cast<const nrq_plan_hdr *>(plan);
  if (h->status) return 0;
  if ((wb != 4 && wb != 2) || (sb != 32 && sb != 16) || nchunks < 1) return -1;
  std::vector<uint8_t> ybuf((size_t)(h->M + h->u) * T + 64, 0x77); /* (device memory nobody cleared) */
  uint8_t *Y = reinterpret_cast<uint8_t *>((reinterpret_cast<uintptr_t>(ybuf.data()) + 15) & ~(uintptr_t)15);
  const uint32_t nstrips = (T + wb - 1) / wb;
  std::vector<uint8_t> ostage;
  int r = 1;
  for (uint32_t s = 0; s < nstrips && r == 1; s++)
    r = wb == 4 ? run_strip<4>(*job, T, s, kc, ostage, Y) : run_strip<2>(*job, T, s, kc, ostage, Y);
  if (r != 1) return r;
  r = emu_backsub(plan, Y, T, sb, nchunks);
  if (r != 1) return r;
  return run_collect(job, T, Y, sc_elems(job, h) + 3u);
}
