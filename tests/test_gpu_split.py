"""-m gpu tier: the split solve of narrow strips -- nrq_solve_kernel stopping after the dense stage, nrq_backsub_kernel<32 / 16>
and nrq_collect_kernel finishing on full-width rows -- at the shapes where those two kernels take another path: both strip
widths of the back-substitution (the option "backsub_sb" forces 16), grids with and without a whole permuted group of strips,
one chunk and many, a partial last strip, more than four W words per row, the byte-wise collect, an undecodable block inside the
batch, and -- through the host planner, so at the same plan in every run -- nrq_backsub_kernel<16> with a second batch of W
words at K' = 56403.  Everything is compared with the CPU oracle byte for byte: intermediate and repair symbols of an encode,
verdict, recovered rows and untouched undecodable blocks of a decode.  tests/test_split_emu.py runs the same bodies on the CPU."""
import numpy as np
import pytest

import nanorq_amd
from test_split_emu import BIG_K, big_reception
from util import loss_pattern, payload

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import gpu_support
    gpu_support.ctx()
    return gpu_support


def _encode(c, src, K, T, esis, want_inter=True, mis=0):
    """encode with every device row `mis` bytes past its allocation's start -> (repair [nblk, nrep, T], inter [nblk, L, T] or None)"""
    nblk, nrep, L = src.shape[0], len(esis), nanorq_amd.params(K)["L"]
    d_src, d_rep = c.alloc(src.nbytes + 16), c.alloc(nblk * nrep * T + 16)
    d_int = c.alloc(nblk * L * T + 16) if want_inter else 0
    try:
        c.upload(d_src + mis, src)
        c.memset(d_rep, 0xCD, nblk * nrep * T + 16)
        c.encode_blocks(K, T, nblk, d_src + mis, K * T, d_rep + mis, nrep * T, esis, d_int + mis if want_inter else 0, L * T)
        c.sync()
        rep = c.download(d_rep + mis, nblk * nrep * T).reshape(nblk, nrep, T)
        inter = c.download(d_int + mis, nblk * L * T).reshape(nblk, L, T) if want_inter else None
    finally:
        c.free(d_src); c.free(d_rep)
        if d_int:
            c.free(d_int)
    return rep, inter


def _decode(c, work, K, T, lost, esis, reps, want_inter=False, mis=0):
    """decode -> (status, blocks [nblk, K, T], inter or None)"""
    nblk, L = work.shape[0], nanorq_amd.params(K)["L"]
    lost_cap, rep_cap = max(1, max(len(x) for x in lost)), max(1, max(len(x) for x in esis))
    lost_a, resi, rsym = np.zeros((nblk, lost_cap), np.uint32), np.zeros((nblk, rep_cap), np.uint32), np.zeros((nblk, rep_cap, T), np.uint8)
    for b in range(nblk):
        lost_a[b, :len(lost[b])] = lost[b]
        resi[b, :len(esis[b])] = esis[b]
        rsym[b, :len(esis[b])] = reps[b][:len(esis[b])]
    d_src, d_rep = c.alloc(work.nbytes + 16), c.alloc(rsym.nbytes + 16)
    d_int = c.alloc(nblk * L * T + 16) if want_inter else 0
    try:
        c.upload(d_src + mis, work)
        c.upload(d_rep + mis, rsym)
        st = c.decode_blocks(K, T, nblk, d_src + mis, K * T, lost_a, [len(x) for x in lost], resi, [len(x) for x in esis], d_rep + mis,
                             rep_cap * T, d_int + mis if want_inter else 0, L * T)
        c.sync()
        out = c.download(d_src + mis, work.nbytes).reshape(nblk, K, T)
        inter = c.download(d_int + mis, nblk * L * T).reshape(nblk, L, T) if want_inter else None
    finally:
        c.free(d_src); c.free(d_rep)
        if d_int:
            c.free(d_int)
    return st, out, inter


def _check_stats(st, wb, sb):
    assert st["strip_bytes"] == wb and st["backsub_strip"] == sb, st


def _encode_and_decode(c, orc, K, T, nblk, wb, sb, loss, mis=0, short=()):
    """an encode and a decode at overhead 0 and 2 against the oracle; blocks in `short` are given one repair symbol too few"""
    src = np.stack([payload(K * T, seed=K + T + wb, block=b).reshape(K, T) for b in range(nblk)])
    lost = [loss_pattern(K, loss, seed=K + sb, block=b) for b in range(nblk)]
    nrep = max(len(x) for x in lost) + 2
    esis = np.concatenate([np.arange(K, K + nrep), [K + 500, (1 << 24) - 1]]).astype(np.uint32)
    rep, inter = _encode(c, src, K, T, esis, mis=mis)
    _check_stats(c.stats(), wb, sb)
    want = {}
    for b in (range(nblk) if nblk <= 9 else (0, nblk // 2, nblk - 1)):
        want[b] = orc.encode_block(src[b], K, T, esis, want_inter=True)
        assert np.array_equal(inter[b], want[b][1]), ("intermediate symbols", K, T, b)
        assert np.array_equal(rep[b], want[b][0]), ("repair symbols", K, T, b)
    for oh in (0, 2):
        use = [len(lost[b]) - 1 if b in short else len(lost[b]) + oh for b in range(nblk)]
        work = src.copy()
        for b in range(nblk):
            work[b][lost[b]] = 0x3C
        e = [esis[:n] for n in use]
        st, out, dint = _decode(c, work, K, T, lost, e, rep, want_inter=(oh == 2), mis=mis)
        _check_stats(c.stats(), wb, sb)
        for b in range(nblk):
            keep = np.setdiff1d(np.arange(K, dtype=np.uint32), lost[b])
            ok, r_out, _ = orc.decode_block(np.concatenate([keep, e[b]]), np.concatenate([src[b][keep], rep[b][:use[b]]]), K, T)
            assert bool(st[b]) == ok, ("verdict", K, T, oh, b)
            assert not (b in short and ok)
            if ok:
                assert np.array_equal(out[b], r_out) and np.array_equal(out[b], src[b]), ("recovered rows", K, T, oh, b)
                if dint is not None and b in want:
                    assert np.array_equal(dint[b], want[b][1]), ("intermediate symbols of the decode", K, T, b)
            else:
                assert np.array_equal(out[b], work[b]), ("undecodable block touched", K, T, oh, b)
        assert sum(bool(x) for x in st) >= nblk - len(short) - 1


class _forced:
    """the forced context with the split solve at strip width wb and the back-substitution strip chosen by `knob`"""

    def __init__(self, G, wb, knob):
        self.c, self.wb, self.knob = G.ctx(), wb, knob

    def __enter__(self):
        self.c.set_option("max_wb", self.wb)
        self.c.set_option("backsub_sb", self.knob)
        return self.c

    def __exit__(self, *a):
        self.c.set_option("max_wb", 16)
        self.c.set_option("backsub_sb", 0)


#  K, T, nblk: what the shape is for (the chunk counts: tests/test_split_emu.py recomputes them through solve_shape)
SHAPES = [(300, 1040, 9),    # SB 32: 33 strips = a permuted group of 32 and one more, 7 chunks
          (100, 1040, 32),   # SB 16: 65 strips = a permuted group of 64 and one more, 1 chunk
          (300, 1043, 3),    # a last strip of 19 / 3 bytes; byte-wise collect
          (3000, 48, 2),     # 5 W words per row
          (64, 1, 5),        # single-byte symbols
          (100, 17, 17),     # ragged symbol sizes
          (100, 33, 8)]


@pytest.mark.parametrize("knob", [0, 16])
@pytest.mark.parametrize("wb", [4, 2])
@pytest.mark.parametrize("K,T,nblk", SHAPES)
def test_forced_split(G, orc, K, T, nblk, wb, knob):
    with _forced(G, wb, knob) as c:
        _encode_and_decode(c, orc, K, T, nblk, wb, 16 if knob else 32, 0.2 if K < 100 else 0.1)


@pytest.mark.parametrize("knob", [0, 16])
def test_rows_not_16_byte_aligned(G, orc, knob):
    """T = 32 with every device row 8 bytes off a 16-byte boundary: the byte-wise collect although T is a multiple of 16, and
    the solve's general movers"""
    with _forced(G, 4, knob) as c:
        _encode_and_decode(c, orc, 300, 32, 3, 4, 16 if knob else 32, 0.1, mis=8)
        assert c.stats()["movers_aligned"] == 0


@pytest.mark.parametrize("knob", [0, 16])
@pytest.mark.parametrize("wb", [4, 2])
def test_undecodable_neighbour_in_a_split_batch(G, orc, wb, knob):
    """three blocks, the middle one with one repair symbol too few: all three kernels of the split solve leave it alone (verdict
    0, its rows untouched), the outer two are exact"""
    with _forced(G, wb, knob) as c:
        _encode_and_decode(c, orc, 300, 48, 3, wb, 16 if knob else 32, 0.1, short=(1,))


# ---- nrq_backsub_kernel<16> with a second batch of W words, at the same plan in every run ----

@pytest.fixture(scope="module")
def big_case(orc):
    """the K' = 56403 reception of tests/test_split_emu.py at T = 40, from the oracle: source, repair symbols, intermediate
    symbols, the decode's verdict and rows.  (T = 16 takes the first 16 byte columns: the code works on every column alike.)"""
    K, T = BIG_K, 40
    lost, esis = big_reception()
    src = payload(K * T, seed=56).reshape(K, T)
    rep, inter, _ = orc.encode_block(src, K, T, esis, want_inter=True)
    keep = np.setdiff1d(np.arange(K, dtype=np.uint32), lost)
    ok, out, _ = orc.decode_block(np.concatenate([keep, esis]), np.concatenate([src[keep], rep]), K, T)
    assert ok and np.array_equal(out, src)
    return lost, esis, src, rep, inter, out


@pytest.mark.parametrize("want_inter", [False, True])
@pytest.mark.parametrize("T", [16, 40])
def test_backsub16_second_word_batch(G, big_case, T, want_inter):
    """One block of K' = 56403 whose HOST plan has more than 640 inactive columns (21 W words per row): 2-byte strips, then
    nrq_backsub_kernel<16> with its loop over a second batch of W words, then the collect -- the device planner reaches this in
    some runs only (tests/variant_ledger.py BACKSUB[16]).  T = 16: one strip; T = 40: two strips and an 8-byte one."""
    c = G.ctx()
    lost, esis, src, rep, inter, ref = big_case
    work = np.ascontiguousarray(src[:, :T])[None].copy()
    work[0][lost] = 0x3C
    c.set_planner(False)
    try:
        st, out, dint = _decode(c, work, BIG_K, T, [lost], [esis], [np.ascontiguousarray(rep[:, :T])], want_inter=want_inter)
        s = c.stats()
    finally:
        c.set_planner(True)
    assert (s["backsub_strip"], s["strip_bytes"], s["planner"]) == (16, 2, 0), s
    assert st[0] == 1
    assert np.array_equal(out[0], ref[:, :T])
    if want_inter:
        assert np.array_equal(dint[0], inter[:, :T])
