/* The launch decisions of nanorq_amd/csrc/launch_shape.h behind a C interface (TEST SUPPORT ONLY): knobs by option name, then
 * solve_lists / solve_shape / plan_shape on synthetic plan headers (M, r2, u, wpr, status: the fields nrq_lds_plan and the launch
 * read), results as flat arrays of 32-bit words.  No GPU, no runtime. */
#include "../../nanorq_amd/csrc/launch_shape.h"

static std::vector<nrq_plan_hdr> make_hdrs(const uint32_t *f, uint32_t n) {
  std::vector<nrq_plan_hdr> h(n);
  for (uint32_t i = 0; i < n; i++) {
    memset(&h[i], 0, sizeof(h[i]));
    h[i].M = f[5 * i]; h[i].r2 = f[5 * i + 1]; h[i].u = f[5 * i + 2]; h[i].wpr = f[5 * i + 3]; h[i].status = f[5 * i + 4];
  }
  return h;
}
static std::vector<const nrq_plan_hdr *> ptrs(const std::vector<nrq_plan_hdr> &h) {
  std::vector<const nrq_plan_hdr *> p;
  for (const nrq_plan_hdr &x : h) p.push_back(&x);
  return p;
}

extern "C" {

void *emu_tuning_new(void) { return new Tuning(); } /* (defaults; the environment is not read) */
void emu_tuning_free(void *t) { delete static_cast<Tuning *>(t); }
int emu_tuning_set(void *t, const char *name, long long value) { return static_cast<Tuning *>(t)->set(name, value) ? 0 : -1; }

uint32_t emu_lds_max(void) { return NRQ_LDS_MAX; }
uint32_t emu_lds_alloc(uint32_t bytes) { return lds_alloc(bytes); }
uint32_t emu_lds_need(const uint32_t *f, uint32_t w) { return nrq_lds_plan(&make_hdrs(f, 1)[0], w).total; }
uint32_t emu_map_by_block(uint32_t nblk) { return nrq_map_by_block(nblk) ? 1u : 0u; }
/* nrq_map_group (solve_body.h): bg = {block, group} of work slot q; the verdict: 1 = a block of the launch */
int emu_map_group(uint32_t q, uint32_t nblk, uint32_t gpb, int by_block, uint32_t *bg) {
  return nrq_map_group(q, nblk, gpb, by_block != 0, &bg[0], &bg[1]) ? 1 : 0;
}
int emu_solve_key_compiled(int wb, int nt, int wv, int g, int al) { return solve_key_index(SolveKey{wb, nt, wv, g, al != 0}) >= 0; }
int emu_plan_key_compiled(uint32_t nt, uint32_t compact) { return plan_key_index(nt, compact) >= 0; }
uint32_t emu_widest_fit(const void *t, const uint32_t *f, uint32_t *need) {
  return widest_fit(*static_cast<const Tuning *>(t), &make_hdrs(f, 1)[0], need);
}

/* out = {err, nsolv, two, wa, need_a, wb, need_b}; on_b: per header */
void emu_solve_lists(const void *t, const uint32_t *f, uint32_t n, int can_split, uint32_t *out, uint8_t *on_b) {
  const std::vector<nrq_plan_hdr> h = make_hdrs(f, n);
  const SolveLists l = solve_lists(*static_cast<const Tuning *>(t), ptrs(h).data(), n, can_split != 0);
  const uint32_t o[7] = {(uint32_t)l.err, l.nsolv, l.two, l.wa, l.need_a, l.wb, l.need_b};
  memcpy(out, o, sizeof(o));
  for (uint32_t i = 0; i < n; i++) on_b[i] = l.two ? l.on_b[i] : 0;
}

/* in = {wb, nblk, T, lds_bytes, max_out, io_aligned, ncu, ahead_hint}; the maxima over the headers are taken here as the launch
 * takes them.  out: 26 words (the last two: stage_bytes(), low and high half), see tests/test_launch_shape_emu.py */
void emu_solve_shape(const void *t, const uint32_t *in, const uint32_t *f, uint32_t n, uint32_t *out) {
  const std::vector<nrq_plan_hdr> h = make_hdrs(f, n);
  const std::vector<const nrq_plan_hdr *> hp = ptrs(h);
  SolveIn si;
  si.wb = in[0]; si.nblk = in[1]; si.T = in[2]; si.lds_bytes = in[3]; si.max_out = in[4]; si.io_aligned = in[5] != 0;
  si.hdrs = hp.data(); si.nhdrs = n;
  for (const nrq_plan_hdr &x : h) {
    if (x.status) continue;
    if (x.M > si.max_slots) si.max_slots = x.M;
    if (x.u > si.max_u) si.max_u = x.u;
    if (x.wpr > si.max_wpr) si.max_wpr = x.wpr;
  }
  const SolveShape s = solve_shape(*static_cast<const Tuning *>(t), (int)in[6], in[7], si);
  const uint64_t sb = s.stage_bytes();
  const uint32_t o[26] = {(uint32_t)s.err, (uint32_t)s.key.WB, (uint32_t)s.key.NT, (uint32_t)s.key.WV, (uint32_t)s.key.G, s.key.AL, s.lds_bytes,
                          s.wg_threads, s.wg_waves, s.split, s.by_block, s.nstrips, s.spl, s.occ, s.grid, s.lsub, s.nslots, s.stage_stride,
                          s.ostage_stride, (uint32_t)s.ybuf_stride, s.res_elems, s.backsub_strip, s.backsub_tbl, s.nchunks, (uint32_t)sb, (uint32_t)(sb >> 32)};
  memcpy(out, o, sizeof(o));
}

/* out: 18 words, see tests/test_launch_shape_emu.py */
int emu_plan_shape(const void *t, int ncu, uint32_t K, uint32_t nblk, uint32_t overhead, uint32_t ucap, uint32_t *out) {
  rq_params p;
  if (!rq_params_init(K, &p)) return -1;
  const uint32_t Mcap = p.L + overhead + PL_EXTRA_ROWS + 8u;
  if (!ucap) { ucap = p.P + 768u; if (ucap > 1280u) ucap = 1280u; }
  const PlanShape s = plan_shape(*static_cast<const Tuning *>(t), ncu, p, nblk, Mcap, ucap);
  const uint32_t o[18] = {(uint32_t)s.err, s.wg_threads, s.compact, s.segmented, s.mode, s.nparts, s.parts[0], s.parts[1], s.parts[2],
                          s.qcap, s.lowcap, s.sh_bytes, s.dyn_bytes, s.wentry_wgs, s.wpass_wgs, s.wpass_lds, s.mh_wgs, s.mh_dyn};
  memcpy(out, o, sizeof(o));
  return (int)pl_state_in_lds(p.L, Mcap, s.dyn_bytes); /* where pl_ctx_setup will put the peeling state (0: the workspace) */
}

} /* extern "C" */
