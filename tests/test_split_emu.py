"""CPU tier: the second half of the split solve of narrow strips -- the bodies of nrq_backsub_kernel<32 / 16> and
nrq_collect_kernel (nanorq_amd/csrc/split_body.h) -- run sequentially on the CPU (tests/emu/solve_emu.cpp).

The reference is GF(2) linear algebra in numpy: W is a bit matrix, so the back-substitution is
    Y[pivslot[k]] ^= XOR of Cu[x] over the set bits x of W_k,        Y[uslot[x]] = Cu[x],
and a collected row is the XOR of the rows its list names.  Synthetic plans take the bodies through every branch no fixed
shape of the suite reaches (W words per row from 1 to 40, the second batch of W words, the strip permutation of every grid
size, every chunk count, both collect forms); real plans of the host planner and of the emulated device planner take the whole
split pipeline -- dense stage, ph_store_raw, scatter to the work buffer, back-substitution, collect -- against the oracle and
against the unsplit form of the same strip width."""
import ctypes as C
import itertools

import numpy as np
import pytest

import nanorq_amd
from emu_support import ROW_ZERO, Job, decode_setup, emu, emu_device_plan, emu_solve, lt_lists
from nanorq_amd import build as nbuild
from nanorq_amd.binding import PLAN_FIELDS
from util import loss_pattern, payload, received_set

F = {name: i for i, name in enumerate(PLAN_FIELDS)}
US = (1, 31, 32, 33, 128, 129, 639, 640, 641, 700, 1279)
NPIVS = (1, 255, 256, 257, 1000)
NCHUNKS = (1, 2, 3, 7, 16)
TS = (1, 15, 16, 17, 31, 32, 33, 47)
TS_WIDE = (1040, 1043)


@pytest.fixture(scope="module")
def S():
    L = emu()
    L.emu_backsub.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
    L.emu_collect.argtypes = [C.POINTER(Job), C.c_uint32, C.c_void_p, C.c_uint32]
    L.emu_solve_split.argtypes = [C.POINTER(Job), C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32]
    L.emu_backsub_strip_of.argtypes = [C.c_uint32] * 3
    L.emu_backsub_strip_of.restype = C.c_uint32
    L.emu_backsub_chunk.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    return L


def aligned(nbytes, mis=0, fill=None, rng=None):
    """nbytes of uint8 whose address is `mis` bytes past a 16-byte boundary"""
    raw = np.empty(nbytes + 32, np.uint8)
    off = (mis - raw.ctypes.data) % 16
    a = raw[off:off + nbytes]
    assert a.ctypes.data % 16 == mis
    if rng is not None:
        a[:] = rng.integers(0, 256, nbytes, dtype=np.uint8)
    else:
        a[:] = 0 if fill is None else fill
    return a


# ---- synthetic plans: only what the back-substitution and the collect read ----

def synthetic_plan(rng, u, npiv, extra=5, L=0):
    """(plan bytes, W bits [npiv, u], pivslot, uslot, M, colslot): random W, random distinct slots for the pivots and the
    inactive columns, `extra` rows no slot names; garbage in wt's pad columns [npiv, npiv_pad)"""
    M = npiv + u + extra
    wpr, pad = (u + 31) // 32, (npiv + 63) // 64 * 64
    slots = rng.permutation(M).astype(np.uint16)
    pivslot, uslot = slots[:npiv], slots[npiv:npiv + u]
    W = rng.integers(0, 2, (npiv, u), dtype=np.uint8)
    if npiv > 2:
        W[0] = 0  # a pivot that takes nothing,
        W[1] = 1  # and one that takes every inactive column
    bits = np.zeros((npiv, wpr * 32), np.uint8)
    bits[:, :u] = W
    words = np.packbits(bits.reshape(npiv, wpr, 32), axis=2, bitorder="little").view(np.uint32).reshape(npiv, wpr)
    wt = rng.integers(0, 1 << 32, (wpr, pad), dtype=np.uint32)  # (garbage beyond npiv)
    wt[:, :npiv] = words.T
    colslot = rng.integers(0, M, L).astype(np.uint16)
    hdr = np.zeros(64, np.uint32)
    off = 256
    parts = []
    for name, arr in (("off_pivslot", pivslot), ("off_uslot", uslot), ("off_wt", wt), ("off_colslot", colslot)):
        hdr[F[name]] = off
        b = arr.tobytes()
        b += bytes(-len(b) % 16)
        parts.append(b)
        off += len(b)
    for name, v in (("status", 0), ("M", M), ("npiv", npiv), ("u", u), ("wpr", wpr), ("npiv_pad", pad), ("L", L), ("total_bytes", off)):
        hdr[F[name]] = v
    return hdr.tobytes() + b"".join(parts), W, pivslot, uslot, M, colslot


def gf2_rows(Wbits, Cu):
    """XOR of the rows Cu[x] over the set bits of every row of Wbits: [n, T] bytes.  (Bit counts through a float32 product:
    exact below 2^24 terms.)"""
    cb = np.unpackbits(Cu, axis=1).astype(np.float32)
    out = np.empty((Wbits.shape[0], Cu.shape[1]), np.uint8)
    for a in range(0, Wbits.shape[0], 4096):
        s = Wbits[a:a + 4096].astype(np.float32) @ cb
        out[a:a + 4096] = np.packbits((s.astype(np.int64) & 1).astype(np.uint8), axis=1)
    return out


def backsub_ref(buf, M, W, pivslot, uslot):
    """the work buffer [(M + u), T] after the back-substitution"""
    ref = buf.copy()
    Cu = buf[M:]
    ref[pivslot.astype(np.int64)] ^= gf2_rows(W, Cu)
    ref[uslot.astype(np.int64)] = Cu
    return ref


def run_backsub(S, rng, plan, W, pivslot, uslot, M, T, sb, nchunks, what):
    u = W.shape[1]
    flat = aligned((M + u) * T, rng=rng)  # (the device's work buffer starts on a 256-byte boundary)
    buf = flat.reshape(M + u, T)
    before = buf.copy()
    ref = backsub_ref(before, M, W, pivslot, uslot)
    planb = (C.c_uint8 * len(plan)).from_buffer_copy(plan)
    assert S.emu_backsub(C.addressof(planb), flat.ctypes.data, T, sb, nchunks) == 1, what
    assert np.array_equal(buf, ref), what
    # (implied by the above, said on their own: rows no slot names and the C_u rows are as they were)
    named = np.zeros(M + u, bool)
    named[pivslot.astype(np.int64)] = True
    named[uslot.astype(np.int64)] = True
    assert np.array_equal(buf[~named], before[~named]), what
    assert np.array_equal(buf[M:], before[M:]), what


@pytest.mark.parametrize("sb", [32, 16])
@pytest.mark.parametrize("u", US)
def test_backsub_body_on_synthetic_plans(S, sb, u):
    """every u with every T below 48, npiv and nchunks dealt so that each (npiv, nchunks) pair occurs for both strip widths"""
    rng = np.random.default_rng(1000 * sb + u)
    for i, T in enumerate(TS):
        n = US.index(u) * len(TS) + i
        npiv, nchunks = NPIVS[n % 5], NCHUNKS[(n // 5) % 5]
        plan, W, pivslot, uslot, M, _ = synthetic_plan(rng, u, npiv)
        run_backsub(S, rng, plan, W, pivslot, uslot, M, T, sb, nchunks, (sb, u, npiv, nchunks, T))


def test_backsub_cases_cover_every_pair():
    """the dealing above reaches every (npiv, nchunks) pair, every u with every T, for each strip width"""
    n = len(US) * len(TS)
    assert {(NPIVS[i % 5], NCHUNKS[(i // 5) % 5]) for i in range(n)} == set(itertools.product(NPIVS, NCHUNKS))


@pytest.mark.parametrize("sb", [32, 16])
@pytest.mark.parametrize("T", TS_WIDE)
def test_backsub_body_on_wide_rows(S, sb, T):
    """T = 1040 / 1043: 33 / 65 strips (one whole permuted group and a rest), a last strip of 16 / 19 / 3 bytes; small plans"""
    rng = np.random.default_rng(sb + T)
    for u, npiv, nchunks in [(1, 1, 1), (33, 257, 3), (129, 255, 16), (31, 256, 2), (128, 1, 7)]:
        plan, W, pivslot, uslot, M, _ = synthetic_plan(rng, u, npiv)
        run_backsub(S, rng, plan, W, pivslot, uslot, M, T, sb, nchunks, (sb, u, npiv, nchunks, T))


@pytest.mark.parametrize("sb", [32, 16])
def test_strip_mapping_is_a_permutation(S, sb):
    per = 8 * 128 // sb
    for gridx in range(1, 301):
        strips = [S.emu_backsub_strip_of(sb, i, gridx) for i in range(gridx)]
        assert sorted(strips) == list(range(gridx)), (sb, gridx)
        # whole groups of 8 * 128 / sb workgroups are permuted among themselves; the rest keep their strip
        full = gridx // per * per
        assert strips[full:] == list(range(full, gridx)), (sb, gridx)
        for g in range(0, full, per):
            assert sorted(strips[g:g + per]) == list(range(g, g + per)), (sb, gridx, g)
            # workgroups i, i + 8, ... of a group (one XCD) take the strips of one 128-byte line
            for i in range(8):
                line = {s * sb // 128 for s in strips[g + i:g + per:8]}
                assert len(line) == 1, (sb, gridx, g, i)


def test_chunk_bounds_partition_the_pivots(S):
    k01 = (C.c_uint32 * 2)()
    for npiv in NPIVS + (0, 56000, 65535):
        for nchunks in range(1, 17):
            at = 0
            for chunk in range(nchunks):
                S.emu_backsub_chunk(npiv, chunk, nchunks, k01)
                assert k01[0] == at and k01[1] >= k01[0], (npiv, nchunks, chunk)  # disjoint, in order, no gap
                assert k01[1] - k01[0] in (npiv // nchunks, -(-npiv // nchunks)), (npiv, nchunks, chunk)
                at = k01[1]
            assert at == npiv, (npiv, nchunks)


# ---- the collect body ----

@pytest.mark.parametrize("T,mis", [(1, 0), (16, 0), (17, 0), (48, 0), (48, 8), (1040, 0)])
@pytest.mark.parametrize("want_inter", [True, False])
def test_collect_body(S, T, mis, want_inter):
    """lists of 0, 1, 2, 32 and 33 rows, rows repeated within a list; 16 bytes per thread where T and every address allow it,
    byte-wise otherwise (T = 1, 17; T = 48 into rows 8 bytes off a 16-byte boundary)"""
    rng = np.random.default_rng(T + mis)
    L = 37
    plan, _, _, _, M, colslot = synthetic_plan(rng, 9, 40, L=L)
    Fimg = aligned(M * T, rng=rng).reshape(M, T)
    lens = [0, 1, 2, 32, 33, 2, 33, 1]
    lists = [rng.integers(0, M, n).astype(np.uint16) for n in lens]
    lists[5][1] = lists[5][0]       # a row twice: it cancels
    lists[6][7] = lists[6][3]
    lists[6][20] = lists[6][3]      # ... and three times: it stays
    cptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    osl = np.concatenate(lists + [np.zeros(1, np.uint16)]).astype(np.uint16)
    nrows_out = 12
    out_row = np.array([3, 0, 11, 5, 6, 1, 9, 4], np.uint32)
    inter = aligned(L * T, mis, fill=0xC3).reshape(L, T)
    out = aligned(nrows_out * T, mis, fill=0x3C).reshape(nrows_out, T)
    ref_out = out.copy()
    for q, lst in enumerate(lists):
        r = np.zeros(T, np.uint8)
        for s in lst:
            r ^= Fimg[int(s)]
        ref_out[out_row[q]] = r
    ref_inter = Fimg[colslot.astype(np.int64)] if want_inter else inter.copy()
    planb = (C.c_uint8 * len(plan)).from_buffer_copy(plan)
    j = Job()
    j.plan = C.addressof(planb)
    j.inter = inter.ctypes.data if want_inter else 0
    j.out = out.ctypes.data
    j.out_cptr = cptr.ctypes.data
    j.out_slots = osl.ctypes.data
    j.out_row = out_row.ctypes.data
    j.nout = len(lens)
    before = Fimg.copy()
    assert S.emu_collect(C.byref(j), T, Fimg.ctypes.data, L + len(lens) + 5) == 1  # (a grid wider than the block's rows, as in a batch)
    assert np.array_equal(inter, ref_inter)
    assert np.array_equal(out, ref_out)
    assert np.array_equal(Fimg, before)


# ---- the whole split pipeline on real plans ----

def _job(plan, rowsrc, src, rep, inter, out, lists, out_rows):
    planb = (C.c_uint8 * len(plan)).from_buffer_copy(plan)
    cptr, cols = lists
    j = Job()
    j.plan = C.addressof(planb)
    j.rowsrc = rowsrc.ctypes.data
    j.src = src.ctypes.data
    j.rep = rep.ctypes.data
    j.inter = inter.ctypes.data if inter is not None else 0
    j.out = out.ctypes.data
    j.out_cptr = cptr.ctypes.data
    j.out_slots = cols.ctypes.data
    j.out_row = out_rows.ctypes.data
    j.nout = len(out_rows)
    return j, (planb, cptr, cols, out_rows, rowsrc, src, rep)


def _split_encode(S, orc, K, T, wb, grids, device_plan, kc):
    p = orc.params(K)
    src = payload(K * T, seed=31).reshape(K, T)
    if device_plan:
        plan, hdr = emu_device_plan(K, kc, [], [], encode=True)
    else:
        plan = nanorq_amd.host_plan(K, np.arange(p["Kp"], dtype=np.uint32), kc)
        hdr = nanorq_amd.plan_header(plan)
    assert hdr["status"] == 0
    rowsrc = np.full(p["L"], ROW_ZERO, np.uint32)
    rowsrc[p["S"] + p["H"]: p["S"] + p["H"] + K] = np.arange(K, dtype=np.uint32)
    esis = np.array([K, K + 1, K + 2, K + 7, K + 500, (1 << 24) - 1], np.uint32)
    lists = lt_lists(orc, K, esis + (p["Kp"] - K), plan)
    rows = np.arange(len(esis), dtype=np.uint32)
    ref_rep, ref_inter, _ = orc.encode_block(src, K, T, esis, want_inter=True)
    kcb = (C.c_uint8 * len(kc)).from_buffer_copy(kc)
    out2 = np.full((len(esis), T), 0x3C, np.uint8)
    r, inter2 = emu_solve(plan, kc, rowsrc, src, None, T, p["L"], lists, rows, out2, wb)  # the unsplit form at the same width
    assert r == 1 and np.array_equal(inter2, ref_inter) and np.array_equal(out2, ref_rep)
    for sb, nchunks in grids:
        inter = np.full((p["L"], T), 0xC3, np.uint8)
        out = np.full((len(esis), T), 0x3C, np.uint8)
        j, keep = _job(plan, rowsrc, src, np.zeros((1, T), np.uint8), inter, out, lists, rows)
        assert S.emu_solve_split(C.byref(j), T, wb, C.addressof(kcb), sb, nchunks) == 1
        assert np.array_equal(inter, ref_inter) and np.array_equal(out, ref_rep), (sb, nchunks)
        assert np.array_equal(inter, inter2) and np.array_equal(out, out2), (sb, nchunks)
        del keep


def _split_decode(S, orc, K, T, wb, grids, device_plan, kc, loss, oh, want_wpr=None):
    prm = orc.params(K)
    src = payload(K * T, seed=32).reshape(K, T)
    kcb = (C.c_uint8 * len(kc)).from_buffer_copy(kc)
    for seed in range(1, 8):
        lost = loss_pattern(K, loss, seed)
        if len(lost) == 0:
            continue
        esis = received_set(K, lost, oh)
        rep_esis = esis[esis >= K]
        rep, ref_inter, _ = orc.encode_block(src, K, T, rep_esis, want_inter=True)
        ok, ref_out, _ = orc.decode_block(esis, np.concatenate([src[esis[esis < K]], rep]), K, T)
        isis, rowsrc = decode_setup(orc, K, lost, rep_esis)
        if device_plan:
            plan, hdr = emu_device_plan(K, kc, lost, rep_esis)
        else:
            plan = nanorq_amd.host_plan(K, isis, kc)
            hdr = nanorq_amd.plan_header(plan)
        assert (hdr["status"] == 0) == ok
        if not ok:
            continue
        if want_wpr is not None:
            assert hdr["wpr"] == want_wpr, hdr
        lists = lt_lists(orc, K, lost, plan)
        work2 = src.copy()
        work2[lost] = 0xEE
        r, inter2 = emu_solve(plan, kc, rowsrc, work2, rep, T, prm["L"], lists, lost, work2, wb)  # the unsplit form
        assert r == 1 and np.array_equal(work2, ref_out) and np.array_equal(inter2, ref_inter)
        for sb, nchunks in grids:
            work = src.copy()
            work[lost] = 0xEE  # missing rows hold garbage
            inter = np.full((prm["L"], T), 0xC3, np.uint8)
            j, keep = _job(plan, rowsrc, work, rep, inter, work, lists, np.ascontiguousarray(lost, np.uint32))
            assert S.emu_solve_split(C.byref(j), T, wb, C.addressof(kcb), sb, nchunks) == 1
            assert np.array_equal(work, ref_out) and np.array_equal(work, src) and np.array_equal(inter, ref_inter), (sb, nchunks)
            assert np.array_equal(work, work2) and np.array_equal(inter, inter2), (sb, nchunks)
            del keep
        return
    raise AssertionError("no decodable reception")


GRIDS = list(itertools.product((32, 16), (1, 3, 16)))  # (back-substitution strip bytes, chunks)


@pytest.mark.parametrize("dev", [False, True], ids=["host_plan", "device_plan"])
@pytest.mark.parametrize("T", [2, 17, 48])
@pytest.mark.parametrize("wb", [4, 2])
@pytest.mark.parametrize("K", [10, 100, 1000])
def test_split_pipeline_matches_oracle_and_unsplit(S, orc, K, wb, T, dev):
    """an encode (intermediate and repair symbols) and a decode at overhead 0 and 2 through emu_solve_split, for both strip
    widths of the back-substitution and 1, 3 and 16 chunks: the oracle's bytes, and those of the unsplit solve at the same strip
    width"""
    kc = nanorq_amd.host_kconst(K)
    _split_encode(S, orc, K, T, wb, GRIDS, dev, kc)
    for oh in (0, 2):
        _split_decode(S, orc, K, T, wb, GRIDS, dev, kc, 0.3 if K == 10 else 0.1, oh)


def test_split_pipeline_with_five_w_words(S, orc):
    """K = 3000 at 10 % loss: 142 inactive columns in the host plan, 5 W words per row -- one more than any pivot has at the
    small sizes the GPU suite forces the split at (the first load beyond word 3 that is not a clamped re-read)"""
    K = 3000
    _split_decode(S, orc, K, 4, 4, [(32, 3), (16, 16)], False, nanorq_amd.host_kconst(K), 0.1, 2, want_wpr=5)


# ---- a real plan with more than 20 W words per row ----

BIG_K = 56403


BIG_RECEPTIONS = ((0.02, 2), (0.3, 5))  # (loss rate, loss pattern seed): host plans with u = 655 and, the spare, 663


def big_reception(which=0):
    """(lost, repair ESIs) of a reception of K' = 56403 whose host plan has more than 640 inactive columns: len(lost) + 2 repair
    ESIs from K.  tests/test_gpu_split.py decodes the first on the GPU."""
    loss, seed = BIG_RECEPTIONS[which]
    lost = loss_pattern(BIG_K, loss, seed=seed)
    return lost, np.arange(BIG_K, BIG_K + len(lost) + 2, dtype=np.uint32)


@pytest.fixture(scope="module")
def big_plan(orc):
    kc = nanorq_amd.host_kconst(BIG_K)
    for which in range(len(BIG_RECEPTIONS)):
        lost, rep_esis = big_reception(which)
        isis, _ = decode_setup(orc, BIG_K, lost, rep_esis)
        plan = nanorq_amd.host_plan(BIG_K, isis, kc)
        hdr = nanorq_amd.plan_header(plan)
        if hdr["status"] == 0 and hdr["wpr"] >= 21:
            return plan, hdr
    raise AssertionError("no plan with more than 20 W words")


@pytest.mark.parametrize("T", [16, 40])
def test_backsub_second_word_batch_on_a_real_plan(S, big_plan, T):
    """K' = 56403 with more than 640 inactive columns: nrq_backsub_kernel<16>'s loop over a second batch of W words, on the
    plan's own W, 16 chunks, rows of one whole strip (T = 16) and of two strips and an 8-byte one (T = 40)"""
    plan, hdr = big_plan
    assert hdr["wpr"] >= 21 and hdr["u"] > 640, hdr
    M, u, npiv, wpr, pad = (hdr[k] for k in ("M", "u", "npiv", "wpr", "npiv_pad"))
    pivslot = np.frombuffer(plan, np.uint16, count=npiv, offset=hdr["off_pivslot"])
    uslot = np.frombuffer(plan, np.uint16, count=u, offset=hdr["off_uslot"])
    wt = np.frombuffer(plan, np.uint32, count=wpr * pad, offset=hdr["off_wt"]).reshape(wpr, pad)
    words = np.ascontiguousarray(wt[:, :npiv].T)
    W = np.unpackbits(words.view(np.uint8).reshape(npiv, wpr * 4), axis=1, bitorder="little")
    assert not W[:, u:].any()
    W = W[:, :u]
    assert W[:, 640:].any()  # (the second batch has work)
    # the plan's maps are what the body assumes: distinct slots, pivots and inactive columns apart
    assert len(set(pivslot.tolist()) | set(uslot.tolist())) == npiv + u and max(pivslot.max(), uslot.max()) < M
    run_backsub(S, np.random.default_rng(T), plan, W, pivslot, uslot, M, T, 16, 16, ("K'=56403", T))


# ---- the launch's grid for the shapes tests/test_gpu_split.py runs ----

def test_gpu_split_shapes_get_the_grids_they_name():
    """the chunk counts and strip widths the GPU tier's table names, through solve_shape (a change of the rule shows here)"""
    L = C.CDLL(nbuild.build_shape_emu())
    L.emu_tuning_new.restype = C.c_void_p
    L.emu_tuning_free.argtypes = [C.c_void_p]
    L.emu_tuning_set.argtypes = [C.c_void_p, C.c_char_p, C.c_longlong]
    L.emu_solve_shape.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    out = (C.c_uint32 * 26)()   # (emu_solve_shape writes 26 words: tests/emu/shape_emu.cpp)
    #        T, nblk, backsub_sb, wpr -> strip, nchunks
    for T, nblk, knob, wpr, strip, nchunks in [(1040, 9, 0, 2, 32, 7), (1040, 32, 16, 1, 16, 1), (1043, 3, 0, 2, 32, 16),
                                               (1043, 3, 16, 2, 16, 11), (48, 2, 0, 5, 32, 16), (16, 1, 0, 21, 16, 16),
                                               (40, 1, 0, 21, 16, 16), (40, 1, 0, 20, 32, 16)]:
        t = L.emu_tuning_new()
        try:
            assert L.emu_tuning_set(t, b"backsub_sb", knob) == 0
            hdr = (C.c_uint32 * 5)(400, 0, wpr * 32, wpr, 0)
            for wb in (4, 2):
                L.emu_solve_shape(t, (C.c_uint32 * 8)(wb, nblk, T, 60000, 10, 0, 256, 0), hdr, 1, out)
                assert (out[0], out[9], out[21], out[23]) == (0, 1, strip, nchunks), (T, nblk, knob, wpr, list(out))
        finally:
            L.emu_tuning_free(t)
