"""-m gpu tier: decodes that take the needed-pivot view (plan.h off_needslot / off_wneed) against the oracle.

A device-planned decode that asks for no intermediate symbols carries the W' image of its lists (the out view, plan.h off_wout) and
back-substitutes nothing; tests/test_gpu_out_view.py is about that.  The needed-pivot view is what such a decode runs on when its
plan has no image -- pl_final_b found no room for it, which pl_arena_bound's reserve keeps from happening -- so every production
plan carries a view that nothing reads.  Its parts exist on the device only or differ there: pl_final_e sets the marks with LDS
atomics, pl_need_a / pl_need_b rank the needed pivots by ballot (the CPU emulation walks a chunk with one thread), nrq_wt_kernel
fills wneed after a segmented run, and backsub_fixed (solve_body.h) walks the view with two register sets in hand-over.  The option
"plan_no_out_view" (tests) withholds the image from device plans, and the call stats say which view the jobs ran on ("out_view",
"need_view", and "nneed" of the first job on the view).  Here, with the option set unless a case says "out":
  - nrq_decode_blocks_lazy (the call bench.py makes) once per view, with and without intermediate symbols, and a batch split over two
    block lists;
  - the loop edges of backsub_fixed: exactly n missing symbols per block, n chosen (by the CPU emulation of the planner) so that
    nneed lies below the workgroup's threads nt, between nt and 2 nt, and above 2 nt.  K = 100 has about 105 pivots and 64 threads:
    nneed > 128 cannot occur there, its cases are "below" and "between" only;
  - the ballot ranking at every planner workgroup size (128, 256, 1024 threads; 1024 threads over a hundred pivots: sixteen chunks,
    one full, one partial, fourteen empty);
  - segmented planner runs, where nrq_wt_kernel fills wneed;
  - 12- and 8-byte strips;
  - device-planned jobs on the view and host re-planned jobs with their image in one call.
GF arithmetic: everything byte for byte.  After a HIP error every later test of the file skips: nothing more is started on a device
that has just faulted."""
import contextlib

import numpy as np
import pytest

import nanorq_amd
import gpu_support as G
from util import loss_pattern, payload

pytestmark = pytest.mark.gpu

_BROKEN = []   # the test whose call returned an error from the HIP runtime: no further launch
_RESET = {"plan_no_out_view": 0, "plan_big_wg": 0, "plan_pack": 1, "plan_split_force": 0, "no_wb12": 0, "plan_ucap": 0, "lds_max": 0}


def _guard():
    if _BROKEN:
        pytest.skip("a call of %s returned a HIP error: no further launches" % (_BROKEN[0],))


@contextlib.contextmanager
def _options(c, what, **opts):
    """the options for the length of a test (back to what gpu_support.ctx() sets); an error of the HIP runtime ends the file"""
    try:
        for k, v in opts.items():
            c.set_option(k, v)
        yield
    except nanorq_amd.NrqError:
        _BROKEN.append(what)
        raise
    finally:
        for k in opts:
            c.set_option(k, _RESET[k])


def _view_opts(view):
    return {"plan_no_out_view": 1} if view == "need" else {}


def _lazy_decode(c, src, lost, esis, rep, want_inter):
    """decode_blocks_lazy of `src` with rows `lost[b]` missing; returns (status, out, inter or None, stats)."""
    nblk, K, T = src.shape
    L = G.nanorq_amd.params(K)["L"]
    lost_cap = max(1, max(len(x) for x in lost))
    rep_cap = len(esis)
    lost_a = np.zeros((nblk, lost_cap), np.uint32)
    resi = np.zeros((nblk, rep_cap), np.uint32)
    for b in range(nblk):
        lost_a[b, :len(lost[b])] = lost[b]
        resi[b] = esis
    nlost = np.array([len(x) for x in lost], np.uint32)
    nrep = nlost + 2
    avail = np.full(nblk, rep_cap, np.uint32)
    work = src.copy()
    for b in range(nblk):
        work[b][lost[b]] = 0xEE
    d_src = c.alloc(nblk * K * T)
    d_rep = c.alloc(nblk * rep_cap * T)
    d_int = c.alloc(nblk * L * T) if want_inter else 0
    try:
        c.upload(d_src, work)
        c.upload(d_rep, np.ascontiguousarray(rep))
        st, _ = c.decode_blocks_lazy(K, T, nblk, d_src, K * T, lost_a, nlost, resi, nrep, avail, d_rep, rep_cap * T,
                                     d_int, L * T)
        c.sync()
        s = c.stats()
        out = c.download(d_src, nblk * K * T).reshape(nblk, K, T)
        inter = c.download(d_int, nblk * L * T).reshape(nblk, L, T) if want_inter else None
    finally:
        c.free(d_src)
        c.free(d_rep)
        if d_int:
            c.free(d_int)
    return st, out, inter, s


_SRC, _INTER = {}, {}


def _blocks(orc, K, T, nblk, nrep, seed):
    """per (K, T, nblk, seed), once: the blocks, repair ESIs K .. and the oracle's repair symbols (grown when a test needs more)"""
    key = (K, T, nblk, seed)
    if key not in _SRC or len(_SRC[key][1]) < nrep:
        src = np.stack([payload(K * T, seed=seed, block=b).reshape(K, T) for b in range(nblk)])
        esis = np.arange(K, K + nrep, dtype=np.uint32)
        _SRC[key] = (src, esis, np.stack([orc.encode_block(src[b], K, T, esis)[0] for b in range(nblk)]))
    src, esis, rep = _SRC[key]
    return src, esis[:nrep], rep[:, :nrep]


def _case(orc, K, T, nblk, loss, seed):
    lost = [loss_pattern(K, loss, seed, block=b) for b in range(nblk)]
    src, esis, rep = _blocks(orc, K, T, nblk, max(len(x) for x in lost) + 8, seed)
    return src, lost, esis, rep


def _ref_inter(orc, K, T, nblk, seed):
    """the oracle's intermediate symbols of _blocks(..., seed), once for both views"""
    key = (K, T, nblk, seed)
    if key not in _INTER:
        src, esis, _ = _SRC[key]
        _INTER[key] = [orc.encode_block(src[b], K, T, esis[:1], want_inter=True)[1] for b in range(nblk)]
    return _INTER[key]


def _on_the_view(s, nblk, what):
    """the call's device-planned jobs all ran on the needed-pivot view"""
    assert (s["planner"], s["host_planned"], s["out_view"], s["need_view"]) == (1, 0, 0, nblk), (what, s)
    assert 0 < s["nneed"] <= s["npiv"], (what, s)


LAZY = [(K, T, loss) for loss in (0.05, 0.10, 0.30) for K, T in [(1000, 64), (5000, 32), (8192, 32), (10000, 24)]]


# (the out view's cases keep the names they had before the view became a parameter)
@pytest.mark.parametrize("view,K,T,loss", [pytest.param(v, K, T, loss, id=("" if v == "out" else "need-") + "%s-%d-%d" % (loss, K, T))
                                           for v in ("out", "need") for K, T, loss in LAZY])
def test_lazy_decode_with_and_without_intermediate_symbols(orc, view, K, T, loss):
    _guard()
    c = G.ctx()
    nblk = 3
    seed = K + int(loss * 100)
    src, lost, esis, rep = _case(orc, K, T, nblk, loss, seed=seed)
    with _options(c, ("lazy decode", view, K, T, loss), **_view_opts(view)):
        st, out, _, s = _lazy_decode(c, src, lost, esis, rep, want_inter=False)
        if K == 10000:
            assert s["strip_bytes"] in (12, 8)
        for b in range(nblk):
            assert st[b] == 1 and np.array_equal(out[b], src[b]), b
        if view == "need":
            _on_the_view(s, nblk, (K, T, loss))
            if loss == 0.05:
                assert s["nneed"] < s["npiv"], s   # a proper subset of the pivots
        else:
            assert (s["planner"], s["host_planned"], s["out_view"], s["need_view"]) == (1, 0, nblk, 0), s
        st, out, inter, s = _lazy_decode(c, src, lost, esis, rep, want_inter=True)
        assert (s["out_view"], s["need_view"], s["nneed"]) == (0, 0, 0), s   # with intermediate symbols: every pivot
        ref = _ref_inter(orc, K, T, nblk, seed)
        for b in range(nblk):
            assert st[b] == 1 and np.array_equal(out[b], src[b]) and np.array_equal(inter[b], ref[b]), b


@pytest.mark.parametrize("view", ["out", "need"])
def test_batch_split_over_two_block_lists(orc, view):
    """A batch whose heavier receptions do not fit the 16-byte image runs as two launches (nrq_device.hip pick_and_launch):
    both take the view."""
    _guard()
    c = G.ctx()
    K, T, nblk = 8192, 48, 8
    src, lost, esis, rep = _case(orc, K, T, nblk, 0.10, seed=77)
    split = False
    with _options(c, ("two lists", view), lds_max=0, **_view_opts(view)):
        for kb in range(162, 146, -1):
            c.set_option("lds_max", kb * 1024)
            st, out, _, s = _lazy_decode(c, src, lost, esis, rep, want_inter=False)
            assert st.all() and np.array_equal(out, src), kb
            if view == "need":
                _on_the_view(s, nblk, kb)
            else:
                assert (s["out_view"], s["need_view"]) == (nblk, 0), (kb, s)
            if 0 < s["blocks_b"] < nblk:
                split = True
                break
    assert split, "no bound split the batch"


# backsub_fixed takes pivots k, k + nt, k + 2 nt, ... of the view, the W words of the next one requested while the current one is
# applied (two register sets): what matters is nneed against nt and 2 nt.  (K, T, threads of the solve workgroup the forced context
# launches, ((n missing symbols per block, regime), ...)); the n's are from the CPU emulation of the planner on these very
# receptions -- nneed of the three blocks: K = 5200: 2 | 378 .. 423 | 1055 .. 1100 | 2187 .. 2271; K = 1000: 3 .. 28 | 146 .. 192 |
# 339 .. 376 | 660 .. 767; K = 100: 2 .. 13 | 24 .. 36 | 85 .. 96 -- and the test asserts the regime from the call's stats.
BACKSUB_EDGES = [(5200, 32, 768, ((1, "below"), (100, "below"), (260, "between"), (600, "above"))),
                 (1000, 32, 256, ((1, "below"), (40, "below"), (90, "between"), (250, "above"))),
                 (100, 32, 64, ((1, "below"), (12, "below"), (50, "between")))]


@pytest.mark.parametrize("K,T,threads,n,regime", [(K, T, th, n, r) for K, T, th, ns in BACKSUB_EDGES for n, r in ns])
def test_loop_edges_of_the_back_substitution_on_the_view(orc, K, T, threads, n, regime):
    _guard()
    c, nblk = G.ctx(), 3
    src, esis, rep = _blocks(orc, K, T, nblk, max(ns[-1][0] for k, _, _, ns in BACKSUB_EDGES if k == K) + 8, seed=K + 11)
    rng = np.random.default_rng(1000 * K + n)
    lost = [np.sort(rng.permutation(K)[:n]).astype(np.uint32) for _ in range(nblk)]
    with _options(c, ("loop edge", K, n), plan_no_out_view=1):
        st, out, _, s = _lazy_decode(c, src, lost, esis[:n + 8], rep[:, :n + 8], want_inter=False)
    assert (s["strip_bytes"], s["wg_threads"]) == (16, threads), s
    _on_the_view(s, nblk, (K, n))
    nt, nneed = s["wg_threads"], s["nneed"]
    assert {"below": nneed < nt, "between": nt < nneed < 2 * nt, "above": nneed > 2 * nt}[regime], (regime, nneed, nt)
    for b in range(nblk):
        assert st[b] == 1 and np.array_equal(out[b], src[b]), b


# pl_need_a / pl_need_b deal the pivots out in nt / 64 chunks, one per wave.  The shapes of
# test_gpu_parity.py::test_planner_workgroup_by_batch_size with and without "plan_pack", and two small blocks under "plan_big_wg";
# the last number is the workgroup plan_shape (launch_shape.h) gives the run, a decision the CPU tier holds on its own
# (tests/test_launch_shape_emu.py).  (K, T, nblk, options, planner threads)
PLAN_WGS = [(300, 64, 5, {"plan_pack": 0}, 1024), (300, 64, 5, {"plan_pack": 1}, 128),
            (1000, 32, 64, {"plan_pack": 0}, 1024), (1000, 32, 64, {"plan_pack": 1}, 256),
            (2500, 16, 9, {"plan_pack": 0}, 1024), (2500, 16, 9, {"plan_pack": 1}, 256),
            (100, 32, 3, {"plan_big_wg": 1}, 1024), (1024, 32, 3, {"plan_big_wg": 1}, 1024)]
assert {w for _, _, _, _, w in PLAN_WGS} == {128, 256, 1024}


@pytest.mark.parametrize("K,T,nblk,opts,plan_wg", PLAN_WGS, ids=["%d-%d-%s" % (K, nblk, "-".join("%s%d" % kv for kv in o.items()))
                                                                 for K, _, nblk, o, _ in PLAN_WGS])
def test_ballot_ranking_at_every_planner_workgroup_size(orc, K, T, nblk, opts, plan_wg):
    _guard()
    c = G.ctx()
    src, lost, esis, rep = _case(orc, K, T, nblk, 0.10, seed=K + 3)
    with _options(c, ("planner workgroup", K, nblk, opts), plan_no_out_view=1, **opts):
        st, out, _, s = _lazy_decode(c, src, lost, esis, rep, want_inter=False)
    assert s["plan_wg_threads"] == plan_wg and s["plan_segmented"] == 0, s
    _on_the_view(s, nblk, (K, nblk, opts))
    for b in range(nblk):
        assert st[b] == 1 and np.array_equal(out[b], src[b]), b


@pytest.mark.parametrize("K,T,nblk", [(1024, 48, 5), (8192, 32, 3)])
def test_segmented_runs_fill_the_view(orc, K, T, nblk):
    """After a segmented planner run (forced: "plan_split_force") pl_need_b leaves the view's W rows to nrq_wt_kernel (pl_wt_fill)."""
    _guard()
    c = G.ctx()
    src, lost, esis, rep = _case(orc, K, T, nblk, 0.10, seed=K + 5)
    with _options(c, ("segmented run", K), plan_no_out_view=1, plan_split_force=1):
        st, out, _, s = _lazy_decode(c, src, lost, esis, rep, want_inter=False)
    assert s["plan_segmented"] == 1 and s["plan_wg_threads"] == 1024, s
    _on_the_view(s, nblk, K)
    for b in range(nblk):
        assert st[b] == 1 and np.array_equal(out[b], src[b]), b


@pytest.mark.parametrize("opts,strip", [({}, 12), ({"no_wb12": 1}, 8)], ids=["strip12", "strip8"])
def test_strip_widths_on_the_view(orc, opts, strip):
    """K = 10000: the 16-byte image does not fit the LDS, the 12-byte one does; without 12-byte strips ("no_wb12") 8."""
    _guard()
    c = G.ctx()
    K, T, nblk = 10000, 24, 3
    src, lost, esis, rep = _case(orc, K, T, nblk, 0.10, seed=K + 10)   # (the blocks of the lazy decode above at this loss)
    with _options(c, ("strip width", strip), plan_no_out_view=1, **opts):
        st, out, _, s = _lazy_decode(c, src, lost, esis, rep, want_inter=False)
    assert s["strip_bytes"] == strip, s
    _on_the_view(s, nblk, strip)
    for b in range(nblk):
        assert st[b] == 1 and np.array_equal(out[b], src[b]), b


def test_jobs_on_the_view_and_jobs_with_their_image_in_one_call(orc):
    """With the inactive-column capacity of the device planner lowered ("plan_ucap", as
    test_gpu_parity.py::test_capacity_fallback_replans_on_the_host does) some blocks of a call are re-planned on the host: those jobs
    carry the host's W' image (out_lists.h build_out_w), the device-planned ones run on the needed-pivot view -- the only reachable
    call whose jobs differ in nrq_job_out_view.  (decode_device launches its jobs, decode_host the re-planned ones behind them on the
    same stream.)  Verdicts and bytes are the oracle's; every decodable block ran on one view or the other, the device-planned on the
    needed-pivot view."""
    _guard()
    c = G.ctx()
    K, T, nblk, loss = 1000, 64, 24, 0.3
    P = nanorq_amd.params(K)["P"]
    lost = [loss_pattern(K, loss * (0.5 + b / nblk), seed=3, block=b) for b in range(nblk)]   # heavier loss towards the end
    src, esis, rep = _blocks(orc, K, T, nblk, max(len(x) for x in lost) + 1, seed=K + 13)
    ok = []
    for b in range(nblk):
        got = np.setdiff1d(np.arange(K, dtype=np.uint32), lost[b])
        n = len(lost[b]) + 1
        v, ref, _ = orc.decode_block(np.concatenate([got, esis[:n]]), np.concatenate([src[b][got], rep[b][:n]]), K, T)
        assert not v or np.array_equal(ref, src[b])
        ok.append(bool(v))
    nbad = nblk - sum(ok)
    work = src.copy()
    for b in range(nblk):
        work[b][lost[b]] = 0xEE
    mixed = False
    with _options(c, ("both kinds of job",), plan_no_out_view=1, plan_ucap=0):
        for extra in (40, 56, 72, 88, 104, 136, 168):
            c.set_option("plan_ucap", P + extra)
            st, out, _ = G.gpu_decode(work, K, T, lost, [esis[:len(x) + 1] for x in lost], [rep[b][:len(lost[b]) + 1] for b in range(nblk)])
            s = c.stats()
            assert [bool(x) for x in st] == ok, extra
            for b in range(nblk):
                if ok[b]:
                    assert np.array_equal(out[b], src[b]), (extra, b)
            hp = s["host_planned"]
            # a decodable block ran on exactly one of the views: re-planned ones with their image, the others on the needed pivots
            assert s["need_view"] + s["out_view"] == nblk - nbad, (extra, s)
            assert nblk - hp - nbad <= s["need_view"] <= nblk - hp and s["out_view"] <= hp, (extra, nbad, s)
            if 0 < hp < nblk:
                mixed = True
                assert s["need_view"] > 0 and (s["out_view"] > 0 or nbad >= hp), (extra, s)
                break
    assert mixed, "no capacity setting split the batch between the device and the host planner"


def test_small_call_planned_on_the_host(orc):
    """One small block is planned on the host (no needed-pivot view: the host's W' image, or with intermediate symbols the full
    back-substitution)."""
    _guard()
    c = G.default_ctx()
    K, T = 1000, 64
    src, lost, esis, rep = _case(orc, K, T, 1, 0.10, seed=5)
    st, out, _, s = _lazy_decode(c, src, lost, esis, rep, want_inter=False)
    assert s["planner"] == 0 and st[0] == 1 and np.array_equal(out[0], src[0])
    assert (s["out_view"], s["need_view"], s["nneed"]) == (1, 0, 0), s
    st, out, inter, s = _lazy_decode(c, src, lost, esis, rep, want_inter=True)
    _, ref_inter, _ = orc.encode_block(src[0], K, T, esis[:1], want_inter=True)
    assert s["planner"] == 0 and st[0] == 1 and np.array_equal(out[0], src[0]) and np.array_equal(inter[0], ref_inter)
