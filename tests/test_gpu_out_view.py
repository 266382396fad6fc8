"""-m gpu tier: decodes that take the out view (plan.h off_wout, nrq_job out_w) against the oracle.

A decode that asks for no intermediate symbols back-substitutes nothing: ph_store (solve_body.h) adds W'_q * C_u to the walk of
missing symbol q's list, W'_q looked up in the back-substitution's tables by the per-word body that exists on the device only
(t4_word: packed nibbles, a byte-select add per address), in a FAST form (768 threads) and a lean one (256 and 64), for 16-, 12- and
8-byte strips, the row's words eight to a trip (one trip up to 256 inactive columns, then two, three ...) -- so for those bodies a decode
on the GPU is the only check.  Here:
  - the device planner through nrq_decode_blocks_lazy (the call bench.py makes), with and without intermediate symbols;
  - the store phase's pass edges: exactly n missing symbols per block around the wave (64) and the workgroup (768 / 256 / 64);
  - a batch split over two block lists;
  - host plans with "plan_force_inact" at the edges of every W-row width class (tests/forced_inact_support.py GPU_CASES), where
    the call stats must say that the launch ran where the row says and that every job carried the view (stats "out_view").
GF arithmetic: everything byte for byte.  After a HIP error every later test of the file skips: nothing more is started on a device
that has just faulted."""
import numpy as np
import pytest

import nanorq_amd
import forced_inact_support as F
from util import loss_pattern, payload

pytestmark = pytest.mark.gpu

_BROKEN = []   # the test whose call returned an error from the HIP runtime: no further launch


@pytest.fixture(scope="module")
def G():
    import gpu_support
    gpu_support.ctx()
    return gpu_support


def _guard(what):
    if _BROKEN:
        pytest.skip("a call of %s returned a HIP error: no further launches" % (_BROKEN[0],))


def _lazy_decode(c, src, lost, esis, rep, want_inter):
    """decode_blocks_lazy of `src` with rows `lost[b]` missing; returns (status, out, inter or None, stats)."""
    nblk, K, T = src.shape
    L = nanorq_amd.params(K)["L"]
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
        st, _ = c.decode_blocks_lazy(K, T, nblk, d_src, K * T, lost_a, nlost, resi, nrep, avail, d_rep, rep_cap * T, d_int, L * T)
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


_SRC = {}


def _blocks(orc, K, T, nblk, nrep, seed):
    """per (K, T, nblk, seed), once: the blocks, repair ESIs K .. and the oracle's repair symbols (grown when a test needs more)"""
    key = (K, T, nblk, seed)
    if key not in _SRC or len(_SRC[key][1]) < nrep:
        src = np.stack([payload(K * T, seed=seed, block=b).reshape(K, T) for b in range(nblk)])
        esis = np.arange(K, K + nrep, dtype=np.uint32)
        _SRC[key] = (src, esis, np.stack([orc.encode_block(src[b], K, T, esis)[0] for b in range(nblk)]))
    src, esis, rep = _SRC[key]
    return src, esis[:nrep], rep[:, :nrep]


@pytest.mark.parametrize("K,T", [(1000, 64), (5000, 32), (8192, 32), (10000, 24)])
def test_device_planner_with_and_without_intermediate_symbols(G, orc, K, T):
    _guard("decode")
    c, nblk = G.ctx(), 3
    lost = [loss_pattern(K, 0.10, K + 7, block=b) for b in range(nblk)]
    src, esis, rep = _blocks(orc, K, T, nblk, max(len(x) for x in lost) + 8, seed=K + 7)
    try:
        st, out, _, s = _lazy_decode(c, src, lost, esis, rep, want_inter=False)
        assert s["planner"] == 1 and s["host_planned"] == 0 and s["out_view"] == nblk, s   # every job carried its lists' image
        for b in range(nblk):
            assert st[b] == 1 and np.array_equal(out[b], src[b]), b
        st, out, inter, s = _lazy_decode(c, src, lost, esis, rep, want_inter=True)
        assert s["out_view"] == 0, s                                                       # ... and none with intermediate symbols
        for b in range(nblk):
            _, ref_inter, _ = orc.encode_block(src[b], K, T, esis[:1], want_inter=True)
            assert st[b] == 1 and np.array_equal(out[b], src[b]) and np.array_equal(inter[b], ref_inter), b
    except nanorq_amd.NrqError:
        _BROKEN.append(("device planner", K, T))
        raise


# exactly n missing symbols per block: a list per thread and pass, so n = 1, a wave less one / whole / and one, a workgroup whole / and
# one, two workgroups and one.  (K, T, threads the forced context launches, the n)
EDGES = [(5200, 32, 768, (1, 63, 64, 65, 768, 769, 1537)), (1000, 32, 256, (1, 63, 65, 256, 257)), (100, 32, 64, (1, 63, 64, 65))]


@pytest.mark.parametrize("K,T,threads,n", [(K, T, th, n) for K, T, th, ns in EDGES for n in ns])
def test_pass_edges_of_the_store_phase(G, orc, K, T, threads, n):
    _guard("decode")
    c, nblk = G.ctx(), 3
    src, esis, rep = _blocks(orc, K, T, nblk, max(ns[-1] for k, _, _, ns in EDGES if k == K) + 8, seed=K + 11)
    rng = np.random.default_rng(1000 * K + n)
    lost = [np.sort(rng.permutation(K)[:n]).astype(np.uint32) for _ in range(nblk)]
    try:
        st, out, _, s = _lazy_decode(c, src, lost, esis[:n + 8], rep[:, :n + 8], want_inter=False)
    except nanorq_amd.NrqError:
        _BROKEN.append(("pass edge", K, n))
        raise
    assert (s["strip_bytes"], s["wg_threads"], s["planner"], s["out_view"]) == (16, threads, 1, nblk), s
    for b in range(nblk):
        assert st[b] == 1 and np.array_equal(out[b], src[b]), b


def test_batch_split_over_two_block_lists(G, orc):
    """A batch whose heavier receptions do not fit the 16-byte image runs as two launches (nrq_device.hip pick_and_launch), the
    job records of the two lists copied side by side: both carry their image and decode."""
    _guard("decode")
    c = G.ctx()
    K, T, nblk = 8192, 48, 8
    lost = [loss_pattern(K, 0.10, 77, block=b) for b in range(nblk)]
    src, esis, rep = _blocks(orc, K, T, nblk, max(len(x) for x in lost) + 8, seed=77)
    split = False
    try:
        for kb in range(162, 146, -1):
            c.set_option("lds_max", kb * 1024)
            st, out, _, s = _lazy_decode(c, src, lost, esis, rep, want_inter=False)
            assert st.all() and np.array_equal(out, src), kb
            assert s["out_view"] == nblk, s
            if 0 < s["blocks_b"] < nblk:
                split = True
                break
    except nanorq_amd.NrqError:
        _BROKEN.append(("two lists", K))
        raise
    finally:
        c.set_option("lds_max", 0)
    assert split, "no bound split the batch"


@pytest.mark.parametrize("index", range(len(F.GPU_CASES)), ids=["%s-u%d" % (c[0], c[1]) for c in F.GPU_CASES])
def test_width_classes_on_host_plans(G, orc, index):
    """Every W-row width class at its edges: host plans with n columns forced inactive, a decode without intermediate symbols at both
    symbol sizes.  (On 4- and 2-byte strips the split solve back-substitutes every pivot and ignores the image its jobs carry.)"""
    _guard("decode")
    from test_gpu_backsub_forms import _forced_plans, _ran_where_it_claims, _reference   # (one oracle run per K for both files)
    form, u, _, n_dec, strip, threads, sb = F.GPU_CASES[index]
    K = F.FORMS[form]["K"]
    lost, esis, src, rep, _ = _reference(orc, K)
    try:
        with _forced_plans(G, F.FORMS[form]["opts"]) as fp:
            fp.force(n_dec)
            for T in F.TS:
                what = (form, u, T)
                work = np.ascontiguousarray(src[:, :, :T]).copy()
                work[:, lost] = 0x3C
                st, out, _ = G.gpu_decode(work, K, T, [lost] * F.NBLK, [esis] * F.NBLK,
                                          [np.ascontiguousarray(rep[b][:, :T]) for b in range(F.NBLK)], want_inter=False)
                s = fp.c.stats()
                _ran_where_it_claims(s, strip, threads, sb, u, what)
                assert s["planner"] == 0 and s["plan_wg_threads"] == 0 and s["out_view"] == F.NBLK, (what, s)
                assert list(st) == [1] * F.NBLK, (what, "verdict", st)
                assert np.array_equal(out, src[:, :, :T]), (what, "recovered block")
    except nanorq_amd.NrqError:
        _BROKEN.append((form, u))
        raise
