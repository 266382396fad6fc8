"""GPU tier: the piece form of the HDPC phase (solve_body.h hdpc_chunks<.., PB>) in the variants that ship it -- 16-byte strips in
the 768-thread workgroup (pieces of 8 bytes, 256 chunks), the 256-thread one (pieces of 4, 64 chunks) and the single wave (pieces
of 4, 16 chunks) -- at one K per branch of the chunking rule (tests/test_hdpc_piece_emu.py has the rule, the branches and the
choice of K; the CPU tier runs the same cases on the launch emulation): an encode with intermediate symbols and a decode at 10 %
loss against the oracle, byte for byte, with a partial last strip (T = 40: 8 bytes of the third strip).  The variants are reached
by the options the other GPU tests use (big_wg, no_tiny, and tiny_any of the forced context), and the call's stats say which ran."""
import numpy as np
import pytest

import gpu_support as G
from util import loss_pattern, payload

# variant -> (workgroup threads, {branch of the chunking rule: K}): the choices of tests/test_hdpc_piece_emu.py, written out -- a GPU test
# module must not call into the library while pytest collects (torch has to bring the GPU runtime up first: tests/conftest.py);
# test_the_cases_are_the_emulation_s holds the two tables against each other on the CPU tier
CASES = {
    "w16-768": (768, {"g2": 226, "g4": 467, "sparse": 964, "h11": 1033}),
    "w16-256": (256, {"g2": 50, "g4": 102, "sparse": 226, "extra": 467, "h11": 1033}),
    "w16-64": (64, {"g2": 6, "g4": 21, "sparse": 50, "extra": 102}),
}

# what the forced context (tiny_any set) needs to take the variant
OPTS = {"w16-768": {"big_wg": 1}, "w16-256": {"no_tiny": 1}, "w16-64": {}}


def _cases():
    return [pytest.param(name, K, 40, id="%s-%s-K%d" % (name, branch, K)) for name, (_, ks) in CASES.items() for branch, K in ks.items()]


def test_the_cases_are_the_emulation_s():
    from test_hdpc_piece_emu import BRANCHES, KMAX, VARIANTS, pick
    assert set(CASES) == set(VARIANTS)
    for name, v in VARIANTS.items():
        C = v["hnt"] // (v["wb"] // v["pb"])
        picked = {b: pick(C, b, v.get("kmax", KMAX)) for b in BRANCHES}
        assert CASES[name] == (v["NT"], {b: K for b, K in picked.items() if K is not None}), name


def _check(orc, c, K, T, nblk, wb, threads):
    src = np.stack([payload(K * T, seed=K + 3, block=b).reshape(K, T) for b in range(nblk)])
    lost = [loss_pattern(K, 0.1, seed=K + 4, block=b) for b in range(nblk)]
    nrep = max(len(x) for x in lost) + 2
    esis = np.arange(K, K + nrep, dtype=np.uint32)
    rep, inter = G.gpu_encode(src, K, T, esis, want_inter=True, kind=c)
    st = c.stats()
    assert (st["strip_bytes"], st["wg_threads"]) == (wb, threads), st
    for b in {0, nblk - 1}:
        r_rep, r_int, _ = orc.encode_block(src[b], K, T, esis, want_inter=True)
        assert np.array_equal(inter[b], r_int), ("intermediate symbols", K, b)
        assert np.array_equal(rep[b], r_rep), ("repair symbols", K, b)
    work = src.copy()
    for b in range(nblk):
        work[b][lost[b]] = 0
    ok, out, _ = G.gpu_decode(work, K, T, lost, [esis[:len(x) + 2] for x in lost], [rep[b][:len(lost[b]) + 2] for b in range(nblk)], kind=c)
    st = c.stats()
    assert (st["strip_bytes"], st["wg_threads"]) == (wb, threads), st
    assert ok.all() and np.array_equal(out, src), ("recovered symbols", K)


@pytest.mark.gpu
@pytest.mark.parametrize("name,K,T", _cases())
def test_piece_form_matches_oracle(orc, name, K, T):
    threads = CASES[name][0]
    c = G.ctx()
    for k, val in OPTS[name].items():
        c.set_option(k, val)
    try:
        _check(orc, c, K, T, 8 if threads == 256 else 2, 16, threads)
    finally:
        for k in OPTS[name]:
            c.set_option(k, 0)


@pytest.mark.gpu
def test_headline_variant_two_strips(orc):
    """K = 8192 on the launch a caller gets: the 768-thread workgroup on 16-byte strips, two strips of one block"""
    _check(orc, G.ctx("default"), 8192, 32, 1, 16, 768)
