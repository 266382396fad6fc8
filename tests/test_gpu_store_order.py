"""The store phase of the solve kernel (solve_body.h, ph_store) at the edges of how it deals the generated symbols to its threads:
the lists come sorted by length (out_lists.h on the host, pl_final_d on the device) and thread t of the 768-thread variant forms
lists t, t + 768, .. a pass each -- so nout = 1 (one wave), 63, 768 (exactly one list per thread), 769 (a second pass for one
list, the shortest) and 1537 (two full passes and one more list).  K = 5200 is the smallest block whose 16-byte image owns a CU (the 768-thread
variant); K = 1000 (256 threads) and K = 100 (a single wave) keep the lean loop and take the new order through out_row[].
T = 32: two strips.  Repair symbols and intermediate symbols are the oracle's, byte for byte; a decode must give the source
block back from the oracle's repair symbols."""
import numpy as np
import pytest

from util import payload

pytestmark = pytest.mark.gpu

T = 32
NOUTS = (1, 63, 768, 769, 1537)
_REF = {}


@pytest.fixture(scope="module")
def G():
    import gpu_support
    gpu_support.ctx()
    return gpu_support


def _ref(orc, K, nblk, nrep):
    """source blocks and the oracle's repair (ESIs K .. K + nrep - 1) and intermediate symbols of each, computed once"""
    key = (K, nblk)
    if key not in _REF or _REF[key][1].shape[1] < nrep:
        src = np.stack([payload(K * T, seed=500 + K, block=b).reshape(K, T) for b in range(nblk)])
        esis = np.arange(K, K + nrep, dtype=np.uint32)
        enc = [orc.encode_block(src[b], K, T, esis, want_inter=True) for b in range(nblk)]
        _REF[key] = (src, np.stack([e[0] for e in enc]), np.stack([e[1] for e in enc]))
        for a in _REF[key]:
            a.setflags(write=False)
    return _REF[key]


def _lost(K, n, b):
    return np.sort(np.random.RandomState(1000 * n + b).choice(K, n, replace=False)).astype(np.uint32)


def _decode(G, orc, K, nblk, n, expect_threads):
    src, rep, _ = _ref(orc, K, nblk, (max(NOUTS) if K == 5200 else n) + 2)
    lost = [_lost(K, n, b) for b in range(nblk)]
    work = src.copy()
    for b in range(nblk):
        work[b][lost[b]] = 0xA5
    esis = np.arange(K, K + n + 2, dtype=np.uint32)
    st, out, _ = G.gpu_decode(work, K, T, lost, [esis] * nblk, [rep[b][:n + 2] for b in range(nblk)])
    s = G.ctx().stats()
    assert st.all() and np.array_equal(out, src), (K, n)
    assert (s["strip_bytes"], s["wg_threads"]) == (16, expect_threads), s
    return s


@pytest.mark.parametrize("n", NOUTS)
def test_decode_768_threads(G, orc, n):
    s = _decode(G, orc, 5200, 2, n, 768)
    assert s["planner"] == 1 and s["host_planned"] == 0, s  # (the device planner's lists)


def test_decode_768_threads_host_lists(G, orc):
    """the same kernel over the lists of the host's builder (a context without the device planner)"""
    c = G.ctx()
    try:
        c.set_planner(False)
        s = _decode(G, orc, 5200, 2, 769, 768)
        assert s["planner"] == 0, s
    finally:
        c.set_planner(True)


@pytest.mark.parametrize("inter", (False, True))
@pytest.mark.parametrize("n", NOUTS)
def test_encode_768_threads(G, orc, n, inter):
    K, nblk = 5200, 2
    src, rep, ref_inter = _ref(orc, K, nblk, max(NOUTS) + 2)
    got, got_inter = G.gpu_encode(src, K, T, np.arange(K, K + n, dtype=np.uint32), want_inter=inter)
    s = G.ctx().stats()
    assert np.array_equal(got, rep[:, :n]), n
    if inter:
        assert np.array_equal(got_inter, ref_inter), n
    assert (s["strip_bytes"], s["wg_threads"]) == (16, 768), s


@pytest.mark.parametrize("K,nblk,n,threads", [(1000, 4, 257, 256), (100, 4, 33, 64)])
def test_decode_lean_loop(G, orc, K, nblk, n, threads):
    """the 256-thread variant with one list more than threads, a single wave with lists of all lengths; then the same blocks
    through the host's lists"""
    _decode(G, orc, K, nblk, n, threads)
    c = G.ctx()
    try:
        c.set_planner(False)
        s = _decode(G, orc, K, nblk, n, threads)
        assert s["planner"] == 0, s
    finally:
        c.set_planner(True)
