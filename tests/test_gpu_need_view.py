"""-m gpu tier: decodes that take the needed-pivot view (plan.h off_needslot) against the oracle.

A device-planned decode that asks for no intermediate symbols back-substitutes only the pivots the missing symbols' LT
lists name; one that asks for them takes every pivot.  Both through nrq_decode_blocks_lazy (the call bench.py makes), at
16-, 12- and 8-byte strips, with a batch split over two block lists and a small call planned on the host."""
import numpy as np
import pytest

import gpu_support as G
from util import loss_pattern, payload

pytestmark = pytest.mark.gpu


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


def _case(orc, K, T, nblk, loss, seed):
    src = np.stack([payload(K * T, seed=seed, block=b).reshape(K, T) for b in range(nblk)])
    lost = [loss_pattern(K, loss, seed, block=b) for b in range(nblk)]
    esis = np.arange(K, K + max(len(x) for x in lost) + 8, dtype=np.uint32)
    rep = np.stack([orc.encode_block(src[b], K, T, esis)[0] for b in range(nblk)])
    return src, lost, esis, rep


@pytest.mark.parametrize("K,T", [(1000, 64), (5000, 32), (8192, 32), (10000, 24)])
@pytest.mark.parametrize("loss", [0.05, 0.10, 0.30])
def test_lazy_decode_with_and_without_intermediate_symbols(orc, K, T, loss):
    c = G.ctx()
    nblk = 3
    src, lost, esis, rep = _case(orc, K, T, nblk, loss, seed=K + int(loss * 100))
    st, out, _, s = _lazy_decode(c, src, lost, esis, rep, want_inter=False)
    if K == 10000:
        assert s["strip_bytes"] in (12, 8)
    for b in range(nblk):
        assert st[b] == 1 and np.array_equal(out[b], src[b]), b
    st, out, inter, _ = _lazy_decode(c, src, lost, esis, rep, want_inter=True)
    for b in range(nblk):
        _, ref_inter, _ = orc.encode_block(src[b], K, T, esis[:1], want_inter=True)
        assert st[b] == 1 and np.array_equal(out[b], src[b]) and np.array_equal(inter[b], ref_inter), b


def test_batch_split_over_two_block_lists(orc):
    """A batch whose heavier receptions do not fit the 16-byte image runs as two launches (nrq_device.hip pick_and_launch):
    both take the view."""
    c = G.ctx()
    K, T, nblk = 8192, 48, 8
    src, lost, esis, rep = _case(orc, K, T, nblk, 0.10, seed=77)
    split = False
    try:
        for kb in range(162, 146, -1):
            c.set_option("lds_max", kb * 1024)
            st, out, _, s = _lazy_decode(c, src, lost, esis, rep, want_inter=False)
            assert st.all() and np.array_equal(out, src), kb
            if 0 < s["blocks_b"] < nblk:
                split = True
                break
    finally:
        c.set_option("lds_max", 0)
    assert split, "no bound split the batch"


def test_small_call_planned_on_the_host(orc):
    """One small block is planned on the host (no view: the full back-substitution), with and without intermediate symbols."""
    c = G.default_ctx()
    K, T = 1000, 64
    src, lost, esis, rep = _case(orc, K, T, 1, 0.10, seed=5)
    st, out, _, s = _lazy_decode(c, src, lost, esis, rep, want_inter=False)
    assert s["planner"] == 0 and st[0] == 1 and np.array_equal(out[0], src[0])
    st, out, inter, s = _lazy_decode(c, src, lost, esis, rep, want_inter=True)
    _, ref_inter, _ = orc.encode_block(src[0], K, T, esis[:1], want_inter=True)
    assert s["planner"] == 0 and st[0] == 1 and np.array_equal(out[0], src[0]) and np.array_equal(inter[0], ref_inter)
