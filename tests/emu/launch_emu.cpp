/*
 * launch_emu.cpp -- one solve LAUNCH on the CPU, on fenced memory (TEST SUPPORT ONLY; tests/test_launch_bounds_emu.py).
 *
 * solve_emu.cpp runs one work slot of one block on arrays of the caller's.  This file runs what nrq_solve_kernel runs for a whole
 * launch: the shape as the host decides it (solve_lists / solve_shape of launch_shape.h on the call's real plan headers), every
 * workgroup of the grid, its work slots by nrq_map_group / nrq_next_group, the portions of the gather and the scatter that each
 * strip index moves and the threads that move them, the two staging sets, the aligned-only movers on the HOST's word, the device
 * form of ph_store's list reads (NRQ_STORE_TRIP_UNBOUNDED), and the two kernels behind a split launch.
 *
 * Every array the kernel reads or writes lives in an anonymous mapping of its own between two pages nobody may touch
 * (lemu_fenced): either its last byte lies in front of the upper page or its first byte behind the lower one.  An access past
 * the array ends in SIGSEGV; the handler names the array and the side and ends the process (the cases run in a child process).
 * What is left of an array's own pages is filled with a pattern that lemu_check_margins finds again afterwards.
 */
#include <signal.h>
#include <stdio.h>
#include <sys/mman.h>
#include <unistd.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#define NRQ_STORE_TRIP_UNBOUNDED 1
#include "wave_emu.h" /* NRQ_WAVE_ANY with the wave's answer: in front of solve_body.h */
#include "../../nanorq_amd/csrc/launch_shape.h" /* (solve_body.h, planner_body.h, the shape of a launch) */
#include "../../nanorq_amd/csrc/split_body.h"
#include "strip_emu.h"

/* ============================================================================================
 * Fences
 * ========================================================================================== */
namespace {

constexpr size_t PAGE = 4096;
constexpr uint8_t MARGIN_BYTE = 0xFE;
struct Fence {
  char name[40];
  uint8_t *map;    /* lower page; the array's pages; upper page */
  size_t maplen;
  uint8_t *user;
  size_t len;
};
Fence g_fences[4096];
int g_nfences = 0;
/* where the emulation is, for the handler's line */
struct Where { const char *role; uint32_t wg, slot, sidx; } g_where = {"idle", 0, 0, 0};
char g_case[256] = "";

void put(const char *s) { if (write(2, s, strlen(s)) < 0) {} }

void on_fault(int sig, siginfo_t *si, void *) {
  char line[512];
  const uint8_t *a = static_cast<const uint8_t *>(si->si_addr);
  const char *name = "no fenced array", *side = "";
  long dist = 0;
  for (int i = 0; i < g_nfences; i++) {
    const Fence &f = g_fences[i];
    if (a >= f.map && a < f.map + PAGE) { name = f.name; side = "BELOW"; dist = (long)(f.user - a); break; }
    if (a >= f.map + f.maplen - PAGE && a < f.map + f.maplen) { name = f.name; side = "ABOVE"; dist = (long)(a - (f.user + f.len)) + 1; break; }
  }
  snprintf(line, sizeof(line), "FENCE HIT: signal %d at %p: %s the array '%s' (%ld byte(s) outside); %s, workgroup %u, slot %u, strip index %u; case %s\n",
           sig, (const void *)a, side, name, dist, g_where.role, g_where.wg, g_where.slot, g_where.sidx, g_case);
  put(line);
  _exit(97);
}

} // namespace

extern "C" {

void lemu_install_handler(void) {
  struct sigaction sa;
  memset(&sa, 0, sizeof(sa));
  sa.sa_sigaction = on_fault;
  sa.sa_flags = SA_SIGINFO;
  sigaction(SIGSEGV, &sa, nullptr);
  sigaction(SIGBUS, &sa, nullptr);
}
void lemu_set_case(const char *s) { snprintf(g_case, sizeof(g_case), "%s", s); }

/* `len` bytes in a mapping of their own.  side 0: the last byte lies in front of a page nobody may touch (the start's alignment
 * is then len's: a multiple of 16 for the aligned cases); side 1: the array begins `mis` bytes behind such a page (mis = 0: right
 * behind it).  The rest of the array's pages holds MARGIN_BYTE.  nullptr: no memory. */
void *lemu_fenced(const char *name, size_t len, int side, size_t mis) {
  if (g_nfences == (int)(sizeof(g_fences) / sizeof(g_fences[0]))) return nullptr;
  if (side == 0) mis = 0;
  const size_t body = (len + mis + PAGE - 1) / PAGE * PAGE + (len + mis == 0 ? PAGE : 0);
  uint8_t *m = static_cast<uint8_t *>(mmap(nullptr, body + 2 * PAGE, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0));
  if (m == MAP_FAILED) return nullptr;
  memset(m + PAGE, MARGIN_BYTE, body);
  if (mprotect(m, PAGE, PROT_NONE) || mprotect(m + PAGE + body, PAGE, PROT_NONE)) return nullptr;
  Fence &f = g_fences[g_nfences++];
  snprintf(f.name, sizeof(f.name), "%s", name);
  f.map = m; f.maplen = body + 2 * PAGE; f.len = len;
  f.user = side == 0 ? m + PAGE + body - len : m + PAGE + mis;
  return f.user;
}
/* first array whose margin was written (its name), or nullptr */
const char *lemu_check_margins(void) {
  for (int i = 0; i < g_nfences; i++) {
    const Fence &f = g_fences[i];
    for (const uint8_t *p = f.map + PAGE; p < f.map + f.maplen - PAGE; p++)
      if ((p < f.user || p >= f.user + f.len) && *p != MARGIN_BYTE) return f.name;
  }
  return nullptr;
}
void lemu_release_all(void) {
  for (int i = 0; i < g_nfences; i++) munmap(g_fences[i].map, g_fences[i].maplen);
  g_nfences = 0;
}

/* ============================================================================================
 * The shape of the launch, as the host decides it
 * ========================================================================================== */

void *lemu_tuning_new(void) { return new Tuning(); } /* (defaults; the environment is not read) */
void lemu_tuning_free(void *t) { delete static_cast<Tuning *>(t); }
int lemu_tuning_set(void *t, const char *name, long long value) { return static_cast<Tuning *>(t)->set(name, value) ? 0 : -1; }

struct LaunchRec {
  uint32_t err, two_lists, wb, NT, WV, G, AL, lds_bytes, split, by_block, nstrips, spl, grid, lsub, nslots, stage_stride, ostage_stride, res_elems,
      backsub_strip, backsub_nsb, nchunks, pad;
  uint64_t ybuf_stride, stage_bytes;
};

/* pick_and_launch + launch_solve up to the launch itself (nrq_device.hip): plans[i] = the plan arena of header i -- ONE for an
 * encode (all blocks share it: can_split = 0), one per solvable block of a decode.  A batch that needs two lists is reported
 * (two_lists), not launched: the cases keep to one width. */
void lemu_shape(const void *tune, const uint64_t *plans, uint32_t nplans, int can_split, uint32_t nblk, uint32_t T, uint32_t max_out,
                int io_aligned, int ncu, LaunchRec *out) {
  const Tuning &t = *static_cast<const Tuning *>(tune);
  std::vector<const nrq_plan_hdr *> hdrs;
  for (uint32_t i = 0; i < nplans; i++) hdrs.push_back(reinterpret_cast<const nrq_plan_hdr *>((uintptr_t)plans[i]));
  memset(out, 0, sizeof(*out));
  const SolveLists l = solve_lists(t, hdrs.data(), hdrs.size(), can_split != 0);
  if (l.err) { out->err = 100u + (uint32_t)l.err; return; }
  if (!l.nsolv) { out->err = 99u; return; }
  if (l.two) { out->two_lists = 1; return; }
  SolveIn in; /* (launch_solve) */
  in.wb = l.wa; in.nblk = nblk; in.T = T; in.lds_bytes = l.need_a; in.max_out = max_out; in.io_aligned = io_aligned != 0;
  in.hdrs = hdrs.data(); in.nhdrs = hdrs.size();
  for (const nrq_plan_hdr *h : hdrs) {
    if (h->status) continue;
    if (h->M > in.max_slots) in.max_slots = h->M;
    if (h->u > in.max_u) in.max_u = h->u;
    if (h->wpr > in.max_wpr) in.max_wpr = h->wpr;
  }
  const SolveShape s = solve_shape(t, ncu, 0u, in);
  out->err = (uint32_t)s.err;
  if (solve_key_index(s.key) < 0) out->err = 98u; /* (no such instance: the launch refuses) */
  out->wb = (uint32_t)s.key.WB; out->NT = (uint32_t)s.key.NT; out->WV = (uint32_t)s.key.WV; out->G = (uint32_t)s.key.G; out->AL = s.key.AL;
  out->lds_bytes = s.lds_bytes; out->split = s.split; out->by_block = s.by_block; out->nstrips = s.nstrips; out->spl = s.spl;
  out->grid = s.grid; out->lsub = s.lsub; out->nslots = s.nslots; out->stage_stride = s.stage_stride; out->ostage_stride = s.ostage_stride;
  out->res_elems = s.res_elems; out->backsub_strip = s.backsub_strip; out->backsub_nsb = s.backsub_nsb; out->nchunks = s.nchunks;
  out->ybuf_stride = s.ybuf_stride; out->stage_bytes = s.stage_bytes();
}

uint32_t lemu_store_slack(void) { return NRQ_STORE_SLACK; }

} /* extern "C" */

/* ============================================================================================
 * The launch
 * ========================================================================================== */
namespace {

/* the movers in the form the instance is compiled with: MPIPE (software-pipelined, the big workgroup) and ALX (aligned only) */
template <int WB, int G>
void gather(bool pipe, bool alx, const GroupSrc<WB> &g, uint8_t *stage, size_t stride, uint32_t u0, uint32_t u1, uint32_t p, uint32_t np, uint32_t sub) {
  if constexpr (G == 1 && WB >= 4) {
    if (alx) {
      if (pipe) pf_gather_impl<WB, G, true, 1>(g, stage, stride, u0, u1, p, np, sub);
      else pf_gather_impl<WB, G, false, 1>(g, stage, stride, u0, u1, p, np, sub);
      return;
    }
  }
  if (pipe) pf_gather_impl<WB, G, true, 0>(g, stage, stride, u0, u1, p, np, sub);
  else pf_gather_impl<WB, G, false, 0>(g, stage, stride, u0, u1, p, np, sub);
}
template <int WB, int G>
void scatter(bool pipe, bool alx, const GroupDst<WB> &g, const uint8_t *ostage, size_t stride, uint32_t u0, uint32_t u1, uint32_t p, uint32_t np, uint32_t sub) {
  if constexpr (G == 1 && WB >= 4) {
    if (alx) {
      if (pipe) pf_scatter_impl<WB, G, true, 1>(g, ostage, stride, u0, u1, p, np, sub);
      else pf_scatter_impl<WB, G, false, 1>(g, ostage, stride, u0, u1, p, np, sub);
      return;
    }
  }
  if (pipe) pf_scatter_impl<WB, G, true, 0>(g, ostage, stride, u0, u1, p, np, sub);
  else pf_scatter_impl<WB, G, false, 0>(g, ostage, stride, u0, u1, p, np, sub);
}

template <int WB, int G>
int run_launch(const LaunchRec &r, const nrq_job *jobs, uint32_t nblk, uint32_t T, const uint8_t *kc, uint8_t *stage_all, uint8_t *ybuf, uint8_t *smem) {
  /* ---- nrq_solve_kernel, nrq_device.hip: the constants of the instance <WB, NT, WV, G, AL> ---- */
  const uint32_t NT = r.NT, nstrips = r.nstrips, nslots = r.nslots, lsub = r.lsub, grid = r.grid;
  const uint32_t stage_stride = r.stage_stride, ostage_stride = r.ostage_stride;
  const bool by_block = r.by_block != 0;
  const SolveRoles R = solve_roles(WB, (int)NT, (int)r.WV, G, r.AL != 0); /* the kernel's own roles and phase forms (solve_roles.h) */
  constexpr uint32_t WBE = (uint32_t)WB * G, SPL = nrq_group_strips(WBE);
  if (!solve_roles_valid(WB, (int)NT, (int)r.WV, G, r.AL != 0)) return -3;
  const uint32_t sub = 1u << lsub;                 /* strips per slot */
  const uint32_t gpb = (nstrips + sub - 1u) / sub; /* slots per block */
  const size_t wg_bytes = 2u * SPL * ((size_t)stage_stride + ostage_stride);
  if (SPL != r.spl) return -4;

  for (uint32_t bid = 0; bid < grid; bid++) { /* blockIdx.x */
    g_where = {"start", bid, 0, 0};
    memset(smem, 0xA5, r.lds_bytes); /* what the workgroup before left in the LDS */
    uint8_t *stage0 = stage_all + (size_t)bid * wg_bytes;
    uint8_t *ostage0 = stage0 + 2u * SPL * (size_t)stage_stride;
    /* all NT threads of the workgroup move [a, b): thread tid as (tid / G) of NT / G, lane tid % G */
    auto all_gather = [&](const GroupSrc<WB> &g, uint8_t *st, uint32_t a, uint32_t b, uint32_t first, uint32_t n) {
      for (uint32_t k = 0; k < n; k++) gather<WB, G>(R.MPIPE, R.ALX, g, st, stage_stride, a, b, k / G, n / G, (first + k) % G);
    };
    auto all_scatter = [&](const GroupDst<WB> &g, const uint8_t *st, uint32_t a, uint32_t b, uint32_t first, uint32_t n) {
      for (uint32_t k = 0; k < n; k++) scatter<WB, G>(R.MPIPE, R.ALX, g, st, ostage_stride, a, b, k / G, n / G, (first + k) % G);
    };
    uint32_t q = nrq_next_group(bid, grid, nslots, jobs, nblk, gpb, by_block);
    if (q >= nslots) continue;
    uint32_t buf = 0, qp = nslots;
    {
      GroupSrc<WB> g0;
      uint32_t b0;
      nrq_group_src<WB>(q, jobs, nblk, gpb, r.by_block, sub, T, nstrips, lsub, g0, &b0);
      g_where = {"first gather", bid, q, 0};
      all_gather(g0, stage0, 0u, g0.M << lsub, 0u, NT); /* (kernel: the first group, nothing to overlap it with) */
    }
    while (q < nslots) {
      const uint32_t qn = nrq_next_group(q + grid, grid, nslots, jobs, nblk, gpb, by_block);
      GroupSrc<WB> gn;
      GroupDst<WB> gp;
      uint32_t blk, blkn = 0, units_n = 0, units_p = 0;
      if (qn < nslots) { nrq_group_src<WB>(qn, jobs, nblk, gpb, r.by_block, sub, T, nstrips, lsub, gn, &blkn); units_n = gn.M << lsub; }
      if (qp < nslots) units_p = nrq_group_dst<WB>(qp, jobs, nblk, gpb, r.by_block, sub, T, nstrips, lsub, ybuf, (size_t)r.ybuf_stride, gp) << lsub;
      {
        GroupSrc<WB> gc;
        nrq_group_src<WB>(q, jobs, nblk, gpb, r.by_block, sub, T, nstrips, lsub, gc, &blk);
      }
      uint8_t *stage_cur = stage0 + (size_t)buf * SPL * stage_stride, *stage_nxt = stage0 + (size_t)(buf ^ 1u) * SPL * stage_stride;
      uint8_t *ostage_cur = ostage0 + (size_t)buf * SPL * ostage_stride, *ostage_prv = ostage0 + (size_t)(buf ^ 1u) * SPL * ostage_stride;
      const uint32_t strip0 = ((by_block ? (q >> 3) : q) % gpb) * sub;
      for (uint32_t sidx = 0; sidx < sub; sidx++) {
        const uint32_t u0 = NRQ_PORTION_AT(units_n, sidx, lsub), u1 = NRQ_PORTION_AT(units_n, sidx + 1u, lsub);
        const uint32_t s0 = NRQ_PORTION_AT(units_p, sidx, lsub), s1 = NRQ_PORTION_AT(units_p, sidx + 1u, lsub);
        const uint32_t sm = NRQ_PORTION_LATE_AT(s0, s1, R.SLATE, R.LATE), um = NRQ_PORTION_LATE_AT(u0, u1, R.GLATE, R.LATE);
        const uint32_t strip = strip0 + sidx;
        if (strip >= nstrips) { /* no such strip: everybody moves this portion */
          g_where = {"strip-less gather", bid, q, sidx};
          if (u1 > u0) all_gather(gn, stage_nxt, u0, u1, 0u, NT);
          g_where.role = "strip-less scatter";
          if (s1 > s0) all_scatter(gp, ostage_prv, s0, s1, 0u, NT);
          continue;
        }
        /* ---- the forward window: who moves what (kernel: `if constexpr (NT == 64)` ... `else if (wv < NFW)` ... `else if (NRQ_WAVE_MOVES(NFW, wv))`) ---- */
        if (NT == 64) { /* the single wave moves its own portions behind its forward passes */
          g_where = {"gather (single wave)", bid, q, sidx};
          if (u1 > u0) all_gather(gn, stage_nxt, u0, u1, 0u, 64u);
          g_where.role = "scatter (single wave)";
          if (sm > s0) all_scatter(gp, ostage_prv, s0, sm, 0u, 64u);
        } else {
          for (uint32_t tid = 0; tid < NT; tid++) {
            const uint32_t wv = tid >> 6;
            if (wv < R.NFW || !NRQ_WAVE_MOVES(R.NFW, wv)) continue; /* the forward waves; the waves that share a SIMD with one idle */
            const uint32_t mv = NRQ_MOVER_INDEX(R.NFW, wv);
            if (mv < R.NGW) {
              g_where = {"gather waves", bid, q, sidx};
              if (um > u0) gather<WB, G>(R.MPIPE, R.ALX, gn, stage_nxt, stage_stride, u0, um, (mv * 64u + (tid & 63u)) / G, (R.NGW * 64u) / G, tid % G);
            } else if (mv < R.NGW + R.NSW) {
              g_where = {"scatter waves", bid, q, sidx};
              if (sm > s0) scatter<WB, G>(R.MPIPE, R.ALX, gp, ostage_prv, ostage_stride, s0, sm, ((mv - R.NGW) * 64u + (tid & 63u)) / G, (R.NSW * 64u) / G, tid % G);
            }
          }
        }
        /* ---- the HDPC window: the waves the phase leaves idle (kernel: `if (tid < HNT) ... else`) ---- */
        if (NT > R.HNT) {
          g_where = {"late gather (waves HDPC leaves idle)", bid, q, sidx};
          if (u1 > um) all_gather(gn, stage_nxt, um, u1, R.HNT, NT - R.HNT);
          g_where.role = "late scatter (waves HDPC leaves idle)";
          if (s1 > sm) all_scatter(gp, ostage_prv, sm, s1, R.HNT, NT - R.HNT);
        }
        /* ---- the strip itself (the movers above touch the other staging sets and the symbol rows, the phases the LDS image and
         * this strip's two staging buffers: the order between them does not matter) ---- */
        g_where = {"strip phases", bid, q, sidx};
        StripCtx<WB, G> c[G];
        for (uint32_t subl = 0; subl < (uint32_t)G; subl++) {
          StripCtx<WB, G> &x = c[subl];
          x.job = jobs + blk;
          x.plan = reinterpret_cast<const uint8_t *>(x.job->plan);
          x.h = reinterpret_cast<const nrq_plan_hdr *>(x.plan);
          x.kc = kc;
          x.lds = smem + subl * WB;
          x.lay = nrq_lds_plan(x.h, WBE);
          x.T = T;
          x.strip = strip;
          const uint32_t at = strip * WBE + subl * WB, rem = at < T ? T - at : 0u;
          x.valid = rem < (uint32_t)WB ? rem : (uint32_t)WB;
        }
        if (c[0].lay.total > r.lds_bytes) return -5; /* the launch's dynamic LDS does not hold this block's image */
        const uint8_t *st_in = stage_cur + (size_t)sidx * stage_stride;
        uint8_t *st_out = ostage_cur + (size_t)sidx * ostage_stride;
        const int rc = strip_phases<WB, G>(c, NT, R, st_in, st_out, ybuf != nullptr);
        if (rc != 1) return rc;
      }
      qp = q;
      q = qn;
      buf ^= 1u;
    }
    /* the results of the last group */
    if (qp < nslots) {
      GroupDst<WB> gp;
      const uint32_t units_p = nrq_group_dst<WB>(qp, jobs, nblk, gpb, r.by_block, sub, T, nstrips, lsub, ybuf, (size_t)r.ybuf_stride, gp) << lsub;
      g_where = {"last scatter", bid, qp, 0};
      all_scatter(gp, ostage0 + (size_t)(buf ^ 1u) * SPL * ostage_stride, 0u, units_p, 0u, NT);
    }
  }
  g_where = {"split tail", 0, 0, 0};
  if (r.split) { /* launch_solve: nrq_backsub_kernel<strip> on (nsb, nchunks, nblk), nrq_collect_kernel on (res_elems, nblk) */
    for (uint32_t blk = 0; blk < nblk; blk++) {
      const uint8_t *plan = reinterpret_cast<const uint8_t *>(jobs[blk].plan);
      if (reinterpret_cast<const nrq_plan_hdr *>(plan)->status) continue; /* (sp_ctx: nothing for a rank deficient block) */
      uint8_t *Y = ybuf + (size_t)blk * r.ybuf_stride;
      const int rc = r.backsub_strip == 32u ? run_backsub<32>(plan, Y, T, r.backsub_nsb, r.nchunks) : run_backsub<16>(plan, Y, T, r.backsub_nsb, r.nchunks);
      if (rc != 1) return rc < 0 ? rc : -6;
    }
    if (r.res_elems)
      for (uint32_t blk = 0; blk < nblk; blk++) {
        if (reinterpret_cast<const nrq_plan_hdr *>(jobs[blk].plan)->status) continue;
        if (run_collect(jobs + blk, T, ybuf + (size_t)blk * r.ybuf_stride, r.res_elems) != 1) return -6;
      }
  }
  g_where = {"idle", 0, 0, 0};
  return 1;
}

} // namespace

/* The launch `r` describes: jobs[nblk] (every pointer a host pointer, every array fenced by the caller), the constants, the staging
 * area of r->stage_bytes and the work buffers of a split launch (nblk * r->ybuf_stride; else nullptr).  side: where the LDS image's
 * own mapping puts it.  1 = done; negative = the emulation refused (see run_launch). */
extern "C" int lemu_run(const LaunchRec *r, const nrq_job *jobs, uint32_t nblk, uint32_t T, const uint8_t *kc, uint8_t *stage, uint8_t *ybuf, int side) {
  uint8_t *smem = static_cast<uint8_t *>(lemu_fenced("LDS image", r->lds_bytes, side, 0));
  if (!smem) return -2;
  if ((r->split != 0) != (ybuf != nullptr)) return -2;
#define LEMU_RUN(WB, G) return run_launch<WB, G>(*r, jobs, nblk, T, kc, stage, ybuf, smem)
  if (r->G == 1) {
    switch (r->wb) {
      case 16: LEMU_RUN(16, 1);
      case 12: LEMU_RUN(12, 1);
      case 8: LEMU_RUN(8, 1);
      case 4: LEMU_RUN(4, 1);
      case 2: LEMU_RUN(2, 1);
      default: return -1;
    }
  }
  if (r->wb != 16) return -1;
  switch (r->G) {
    case 2: LEMU_RUN(16, 2);
    case 4: LEMU_RUN(16, 4);
    case 8: LEMU_RUN(16, 8);
    default: return -1;
  }
#undef LEMU_RUN
}

/* What the test pins against numbers of its own: "NRQ_W12_FW=3 ...", the role knobs as compiled here (the macros themselves), */
extern "C" const char *lemu_role_knobs(void) {
#define LEMU_K(name) " NRQ_" #name "=%u"
#define LEMU_V(name) , (unsigned)(NRQ_##name)
#define LEMU_KNOBS(X)                                                                                                                \
  X(W12_FW) X(W12_GW) X(W12_SW) X(MOVER_WAVES) X(GATHER_WAVES_NARROW) X(GATHER_WAVES_NARROW_WB) X(PIPE_BIG) X(PIPE_SMALL) X(HDPC_NT) \
  X(HDPC_NT_SMALL) X(SCATTER_LATE_PCT) X(GATHER_LATE_PCT) X(SCATTER_LATE_PCT_NARROW) X(GATHER_LATE_PCT_NARROW) X(HDPC_REGS_MAX_WB)   \
  X(HDPC_REGS_12) X(FOLD_PRE256)
  static char buf[1024];
  snprintf(buf, sizeof(buf), LEMU_KNOBS(LEMU_K) LEMU_KNOBS(LEMU_V));
#undef LEMU_KNOBS
#undef LEMU_V
#undef LEMU_K
  return buf;
}
/* ... and what solve_roles() makes of them for instance i of NRQ_SOLVE_INSTANCES: "WB NT WV G AL: NFW NGW NSW MPIPE ALX RU HNT
 * SLATE GLATE hdpc_regs fold_batch batch fast commit_pb" (nullptr behind the last) */
extern "C" const char *lemu_instance_roles(int i) {
  static char buf[256];
  if (i < 0 || i >= nrq_solve_nkeys) return nullptr;
  const SolveKey k = nrq_solve_keys[i];
  const SolveRoles R = solve_roles(k.WB, k.NT, k.WV, k.G, k.AL);
  snprintf(buf, sizeof(buf), "%d %d %d %d %d: %u %u %u %d %d %u %u %u %u %d %d %d %d %d", k.WB, k.NT, k.WV, k.G, (int)k.AL, R.NFW, R.NGW, R.NSW,
           (int)R.MPIPE, (int)R.ALX, R.RU, R.HNT, R.SLATE, R.GLATE, (int)R.hdpc_regs, R.fold_batch, (int)R.batch, (int)R.fast, R.commit_pb);
  return buf;
}

/* wave_emu.h on its own: lane l of 64 stays in a loop under NRQ_WAVE_ANY while i < l % 5; every lane must go round as often as the
 * neediest (4 times).  Returns the lanes that did not, plus 1000 x the ballots the wave took (5). */
extern "C" int lemu_wave_selftest(void) {
  int rounds[64];
  const size_t ballots = wave_in_step(64u, [&](unsigned l) {
    int n = 0;
    for (unsigned i = 0; NRQ_WAVE_ANY(i < l % 5u); i++) n++;
    rounds[l] = n;
  });
  int bad = 0;
  for (int l = 0; l < 64; l++) bad += rounds[l] != 4;
  return bad + 1000 * (int)ballots;
}
