/* Effects of the library's own kernels for the model HIP runtime (hip_model.h, hm_set_effect): what the DECODE PLANNER leaves
 * behind, so that the host flow of a decode through the device planner -- planner streams, plan arenas and job records in three
 * sets, the events `planned` / `arena_free` / `pstaged` -- runs on the model.  The host half of that flow reads the plan headers
 * the planner kernel writes; here the kernel's effect builds them with the library's HOST planner (nrq_host_plan_build) from the
 * lists the job records name: same verdict per block, a plan the launch decisions accept.  The footprint is exact: a planner
 * run reads its job records, lists and constants and writes its workspace, arenas, headers and the solve's job records; it only
 * FORWARDS the addresses of the symbol buffers.  The symbols themselves are never computed: no kernel runs. */
#include <cstdint>
#include <algorithm>
#include <cstring>
#include <map>
#include <vector>

#include "../../nanorq_amd/csrc/planner_body.h"
#include "../../nanorq_amd/csrc/planner_host.h"
#include "hip_model.h"

namespace {

bool u32_arg(const hm_arg &a, uint32_t *v) {
  if (a.kind != HM_ARG_SCALAR || a.n != 4) return false;
  memcpy(v, a.p, 4);
  return true;
}

/* what every kernel of a planner run touches through its job records (b < nblk) */
bool planjob_footprint(const nrq_planjob *pj, uint32_t nblk, const void *d_kc) {
  if (!hm_effect_touch(pj, (size_t)nblk * sizeof(nrq_planjob), 0)) return false;
  bool ok = !d_kc || hm_effect_touch_tail(d_kc, 0);
  for (uint32_t b = 0; b < nblk; b++) {
    const nrq_planjob &j = pj[b];
    if (j.lost && j.nlost) ok = hm_effect_touch((const void *)(uintptr_t)j.lost, (size_t)j.nlost * 4, 0) && ok;
    if (j.rep_esi && j.nrep_avail) ok = hm_effect_touch((const void *)(uintptr_t)j.rep_esi, (size_t)j.nrep_avail * 4, 0) && ok;
    if (j.work) ok = hm_effect_touch_tail((const void *)(uintptr_t)j.work, 1) && ok; /* (the workspace's size is the planner's own) */
    if (j.arena) ok = hm_effect_touch((const void *)(uintptr_t)j.arena, j.arena_cap, 1) && ok;
    if (j.hdr_out) ok = hm_effect_touch((const void *)(uintptr_t)j.hdr_out, sizeof(nrq_plan_hdr), 1) && ok;
  }
  return ok;
}

/* nrq_plan_kernel<NT, COMPACT>(rq_params p, const uint8_t *kc, const nrq_planjob *pj, nrq_job *jobs, uint32_t nblk, ...) */
void plan_effect(const hm_arg *a, int n) {
  uint32_t nblk;
  if (n < 5 || a[0].kind != HM_ARG_BYTES || a[0].n != sizeof(rq_params) || !u32_arg(a[4], &nblk)) return;
  rq_params p;
  memcpy(&p, a[0].p, sizeof(p));
  const uint8_t *kc = (const uint8_t *)a[1].p;
  const nrq_planjob *pj = (const nrq_planjob *)a[2].p;
  nrq_job *jobs = (nrq_job *)a[3].p;
  if (!planjob_footprint(pj, nblk, kc)) return;
  if (jobs && !hm_effect_touch(jobs, (size_t)nblk * sizeof(nrq_job), 1)) return;
  const uint32_t pad = p.Kp - p.K;
  for (uint32_t b = 0; b < nblk; b++) {
    const nrq_planjob &j = pj[b];
    if (j.mode != 0 || !j.hdr_out) continue; /* (encode plans built on the device: not modelled, their header stays as it is) */
    nrq_plan_hdr hdr;
    memset(&hdr, 0, sizeof(hdr));
    hdr.magic = NRQ_PLAN_MAGIC;
    hdr.status = 1;
    const uint32_t *lost = (const uint32_t *)(uintptr_t)j.lost, *resi = (const uint32_t *)(uintptr_t)j.rep_esi;
    uint8_t *plan = nullptr;
    uint32_t bytes = 0;
    bool sane = j.nlost != 0 && j.nrep >= j.nlost;
    for (uint32_t g = 0; sane && g < j.nlost; g++) sane = lost[g] < p.K && (!g || lost[g] > lost[g - 1]);
    for (uint32_t use = j.nrep; sane && use <= j.nrep_avail; use++) { /* one more symbol while the system is rank deficient */
      const uint32_t over = use - j.nlost;
      std::vector<uint32_t> isis(p.Kp + over);
      for (uint32_t i = 0; i < p.Kp; i++) isis[i] = i;
      for (uint32_t g = 0; g < j.nlost; g++) isis[lost[g]] = resi[g] + pad;
      for (uint32_t e = 0; e < over; e++) isis[p.Kp + e] = resi[j.nlost + e] + pad;
      if (plan) nrq_host_free(plan);
      plan = nullptr;
      if (nrq_host_plan_build(p.Kp, p.Kp + over, isis.data(), kc, &plan, &bytes) != 0) break;
      memcpy(&hdr, plan, sizeof(hdr));
      hdr.reserved[1] = use - j.nrep;
      if (hdr.status == 0) break;
    }
    if (plan && hdr.status == 0 && bytes > j.arena_cap) { /* the planner's own answer to a plan that does not fit */
      hdr.status = 1;
      hdr.reserved[0] = PL_FAIL_CAPACITY;
    } else if (plan && hdr.status == 0) {
      memcpy((void *)(uintptr_t)j.arena, plan, bytes);
      memcpy((void *)(uintptr_t)j.arena, &hdr, sizeof(hdr));
    }
    if (plan) nrq_host_free(plan);
    memcpy((void *)(uintptr_t)j.hdr_out, &hdr, sizeof(hdr));
    if (jobs) { /* the solve's job record: the buffers it forwards, its lists somewhere in the arena */
      nrq_job &o = jobs[b];
      memset(&o, 0, sizeof(o));
      o.plan = o.rowsrc = o.out_cptr = o.out_slots = o.out_row = j.arena;
      o.src = o.out = j.src;
      o.rep = j.rep;
      o.inter = j.inter;
      o.nout = hdr.status == 0 ? j.nlost : 0;
      hm_effect_wrote(&o, sizeof(o));
    }
  }
}

/* the helper kernels of a segmented run: (rq_params, kc, pj, ...) with one block per grid row; nrq_wt_kernel: (pj, ...) */
void plan_helper_effect(const hm_arg *a, int n) {
  unsigned g[3];
  hm_effect_grid(g);
  if (n >= 3 && a[0].kind == HM_ARG_BYTES) (void)planjob_footprint((const nrq_planjob *)a[2].p, g[1], a[1].p);
  else if (n >= 1) (void)planjob_footprint((const nrq_planjob *)a[0].p, g[1], nullptr);
}

/* The kernels that run a batch of job records: nrq_solve_kernel(const nrq_job *jobs, nblk, ...), and the two that finish a split
 * solve, nrq_backsub_kernel(jobs, T, ybuf, ...) with one block per grid z and nrq_collect_kernel(jobs, T, ybuf, ...) with one per
 * grid y.  Exact: the job records, what each record's nine addresses name (from the address to the end of its allocation: the
 * plan and the lists read, the block's rows and its intermediate symbols written) and the launch's other pointer arguments.
 * The footprint from the arguments alone would go one level further, through every word of the plan's allocation -- and the
 * buffer of a device-built encode plan also holds the planner's own job record behind the plan, whose words name the
 * planner's workspace: the solve never reads that record, and the next build of a plan on the planner's stream, which writes
 * the workspace, needs no order against it. */
void jobs_footprint(const hm_arg *a, int n, uint32_t nblk) {
  if (n < 1 || a[0].kind != HM_ARG_CONST_PTR || !a[0].p) return;
  const nrq_job *jobs = (const nrq_job *)a[0].p;
  if (!hm_effect_touch(jobs, (size_t)nblk * sizeof(nrq_job), 0)) return;
  /* one touch per allocation (an operation counts once on the allocations it touches): from the lowest address named, written
   * if any of them is */
  std::map<uint64_t, std::pair<uint64_t, int>> al; /* base -> (lowest address, written) */
  auto name = [&](uint64_t p, int write) {
    if (!p) return;
    const uint64_t base = hm_effect_base((const void *)(uintptr_t)p);
    if (!base) { (void)hm_effect_touch((const void *)(uintptr_t)p, 1, write); return; } /* (H2) */
    auto it = al.emplace(base, std::make_pair(p, write)).first;
    it->second.first = std::min(it->second.first, p);
    it->second.second |= write;
  };
  for (uint32_t b = 0; b < nblk; b++) {
    const nrq_job &j = jobs[b];
    for (uint64_t r : {j.plan, j.rowsrc, j.rep, j.out_cptr, j.out_slots, j.out_row}) name(r, 0);
    for (uint64_t w : {j.src, j.inter, j.out}) name(w, 1);
  }
  for (int i = 1; i < n; i++)
    if (a[i].kind == HM_ARG_PTR || a[i].kind == HM_ARG_CONST_PTR) name((uint64_t)(uintptr_t)a[i].p, a[i].kind == HM_ARG_PTR);
  for (auto &kv : al) (void)hm_effect_touch_tail((const void *)(uintptr_t)kv.second.first, kv.second.second);
}
void solve_effect(const hm_arg *a, int n) {
  uint32_t nblk;
  if (n >= 2 && u32_arg(a[1], &nblk)) jobs_footprint(a, n, nblk);
}
void backsub_effect(const hm_arg *a, int n) {
  unsigned g[3];
  hm_effect_grid(g);
  jobs_footprint(a, n, g[2]);
}
void collect_effect(const hm_arg *a, int n) {
  unsigned g[3];
  hm_effect_grid(g);
  jobs_footprint(a, n, g[1]);
}

struct Register {
  Register() {
    hm_set_effect("nrq_solve_kernel", solve_effect, 1);
    hm_set_effect("nrq_backsub_kernel", backsub_effect, 1);
    hm_set_effect("nrq_collect_kernel", collect_effect, 1);
    hm_set_effect("nrq_plan_kernel", plan_effect, 1);
    for (const char *k : {"nrq_wentry_kernel", "nrq_wpass_kernel", "nrq_mh_kernel", "nrq_wt_kernel"}) hm_set_effect(k, plan_helper_effect, 1);
  }
} reg;

} // namespace
