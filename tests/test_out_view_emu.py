"""CPU tier: the out view of decodes that ask for no intermediate symbols (plan.h off_wout, nrq_job out_w).

A missing symbol is the XOR of C(c) over its LT list, C(c) = Y_c ^ W_c * C_u for a pivot column and C_u[x] for an inactive one, so
with W'_q = XOR of W_c over the pivot entries of list q the solve back-substitutes nothing and ph_store adds W'_q * C_u to the walk
of list q.  Here the planner's phase code runs emulated on the CPU (tests/emu/planner_emu.cpp) and the host's builder as it is
(tests/emu/out_view_emu.cpp): both images must be what pivslot / colslot / wt and the oracle's LT columns give independently, the
segmented planner run must leave the same bytes, and the emulated solve (tests/emu/solve_emu.cpp) with the job the planner wrote
must give the source's rows.

Two kinds of list are to be covered: one that names an inactive column (its slot holds the column's value: it adds nothing to W')
and one of pivots only.  The LT list of a SOURCE symbol is never of the second kind: its tuple names d1 >= 2 of the P permanently
inactive columns W .. L-1 (RFC 6330 5.3.5.3), and both planners leave every one of those inactive (asserted below: no pivot column
is >= W).  So the first kind is asserted on the receptions themselves, and the second on lists made for it: single pivots, pairs,
a pivot twice, a pivot with a parked column, through the host's builder and the emulated solve, against the oracle's intermediate
symbols."""
import ctypes as C

import numpy as np
import pytest

import nanorq_amd
from emu_support import Job, decode_setup, emu, emu_device_plan, lt_lists, pemu
from util import loss_pattern, payload, received_set

U32P = C.POINTER(C.c_uint32)
T, WB = 16, 16
_LIBS = {}


def _lib(name):
    if name not in _LIBS:
        from nanorq_amd import build as nbuild
        _LIBS[name] = C.CDLL(getattr(nbuild, "build_%s_emu" % name)())
    return _LIBS[name]


def _u16(buf, off, n):
    return np.frombuffer(buf, np.uint16, count=n, offset=off)


def _u32(buf, off, n):
    return np.frombuffer(buf, np.uint32, count=n, offset=off)


def _device_plan(K, kc, lost, rep_esis):
    """emu_plan with its job: (arena bytes up to total_bytes, header, lists (cptr, cols, rows), out_w)"""
    L_ = pemu()
    kcb = (C.c_uint8 * len(kc)).from_buffer_copy(kc)
    lost = np.ascontiguousarray(lost, np.uint32)
    rep_esis = np.ascontiguousarray(rep_esis, np.uint32)
    cap = L_.emu_plan_arena_bound(K, C.addressof(kcb), max(0, len(rep_esis) - len(lost)) + 24, len(lost) + 8)  # (= emu_device_plan's)
    arena = np.zeros(cap, np.uint8)
    job = Job()
    assert L_.emu_plan(K, 0, C.addressof(kcb), lost.ctypes.data_as(U32P), len(lost), rep_esis.ctypes.data_as(U32P), len(rep_esis),
                       len(rep_esis), arena.ctypes.data, cap, 140 * 1024, C.byref(job)) == 0
    hdr = nanorq_amd.plan_header(arena.tobytes()[:256])
    if hdr["status"] != 0:
        return None, hdr, None, 0
    base, n = arena.ctypes.data, job.nout
    assert job.plan == base and n == len(lost)
    cptr = _u32(arena, job.out_cptr - base, n + 1).copy()
    rows = _u32(arena, job.out_row - base, n).copy()
    cols = _u16(arena, job.out_slots - base, int(cptr[n])).copy()
    assert (hdr["off_out_cptr"], hdr["off_out_slots"]) == (job.out_cptr - base, job.out_slots - base)
    return arena.tobytes()[:hdr["total_bytes"]], hdr, (cptr, cols, rows), job.pad  # (pad: the record's last word, out_w)


def _host_lists(K, colslot, isis):
    """build_out_lists of out_lists.h: (cptr, cols, order)"""
    L_ = _lib("out_lists")
    L_.emu_out_lists.restype = C.c_uint32
    L_.emu_out_lists.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    isis = np.ascontiguousarray(isis, np.uint32)
    colslot = np.ascontiguousarray(colslot, np.uint16)
    n = len(isis)
    cptr, order, cols = np.zeros(n + 1, np.uint32), np.zeros(n, np.uint32), np.zeros(n * 64, np.uint16)
    m = L_.emu_out_lists(K, 0, colslot.ctypes.data, n, isis.ctypes.data, cptr.ctypes.data, cols.ctypes.data, len(cols), order.ctypes.data)
    assert m != 0xFFFFFFFF and m == cptr[n]
    return cptr, cols[:m].copy(), order


def _host_image(plan, cptr, cols, wpr):
    """build_out_w of out_lists.h: the image as [wpr, out_pad]"""
    L_ = _lib("out_view")
    L_.emu_out_w.restype = C.c_uint32
    L_.emu_out_w.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    n = len(cptr) - 1
    opad = (n + 63) & ~63
    planb = (C.c_uint8 * len(plan)).from_buffer_copy(plan)
    w = np.zeros(wpr * opad + 1, np.uint32)
    m = L_.emu_out_w(C.addressof(planb), n, cptr.ctypes.data, cols.ctypes.data, w.ctypes.data, len(w))
    assert m == wpr * opad
    return w[:m].reshape(wpr, opad)


def _expected_rows(orc, K, plan, hdr, rows):
    """W'_q of the list of source symbol rows[q], from pivslot / colslot / wt and the oracle's LT columns alone; also whether the
    list names an inactive column, and its slots"""
    colslot = _u16(plan, hdr["off_colslot"], hdr["L"])
    pivslot = _u16(plan, hdr["off_pivslot"], hdr["npiv"])
    uslot = set(int(s) for s in _u16(plan, hdr["off_uslot"], hdr["u"]))
    wpr = hdr["wpr"]
    wt = _u32(plan, hdr["off_wt"], wpr * hdr["npiv_pad"]).reshape(wpr, hdr["npiv_pad"])
    pivot_of = np.full(hdr["M"], -1, np.int64)
    pivot_of[pivslot] = np.arange(hdr["npiv"])
    assert not uslot & set(int(s) for s in pivslot)
    want = np.zeros((wpr, len(rows)), np.uint32)
    inact, slots = [], []
    for q, e in enumerate(rows):
        sl = [int(colslot[c]) for c in orc.lt_columns(K, int(e))]
        for s in sl:
            if pivot_of[s] >= 0:
                want[:, q] ^= wt[:, pivot_of[s]]
            else:
                assert s in uslot  # (a column is a pivot's or inactive)
        inact.append(any(s in uslot for s in sl))
        slots.append(sorted(sl))
    return want, inact, slots


def _check_image(image, want, n):
    assert image.shape[1] % 64 == 0 and image.shape[1] == (n + 63) & ~63
    assert np.array_equal(image[:, :n], want)
    assert not image[:, n:].any()


def _solve(plan, kc, rowsrc, work, rep, lists, rows, out_w, inter=None, out=None):
    """The emulated solve of one job; lost rows go into `work` (or the lists' symbols into `out`), intermediate symbols into `inter`
    when given."""
    planb = (C.c_uint8 * len(plan)).from_buffer_copy(plan)
    kcb = (C.c_uint8 * len(kc)).from_buffer_copy(kc)
    cptr, cols = lists
    rows = np.ascontiguousarray(rows, np.uint32)
    j = Job()
    j.plan = C.addressof(planb)
    j.rowsrc = rowsrc.ctypes.data
    j.src = work.ctypes.data
    j.rep = rep.ctypes.data
    j.inter = inter.ctypes.data if inter is not None else 0
    j.out = (work if out is None else out).ctypes.data
    j.out_cptr = cptr.ctypes.data
    j.out_slots = cols.ctypes.data
    j.out_row = rows.ctypes.data
    j.nout = len(rows)
    j.pad = out_w
    return emu().emu_solve(C.byref(j), T, WB, C.addressof(kcb))


@pytest.mark.parametrize("K", [100, 1000, 8192, 10000])
@pytest.mark.parametrize("p", [0.05, 0.10, 0.30])
def test_out_view_of_both_planners(orc, K, p):
    prm = orc.params(K)
    src = payload(K * T, seed=23).reshape(K, T)
    kc = nanorq_amd.host_kconst(K)
    done, with_inact = 0, 0
    for seed in (1, 2):
        lost = loss_pattern(K, p, seed)
        assert len(lost)
        esis = received_set(K, lost, 2)
        rep_esis = esis[esis >= K]
        plan, hdr, lists, out_w = _device_plan(K, kc, lost, rep_esis)
        if plan is None:
            continue  # (the oracle's verdict too: rank deficient)
        cptr, cols, rows = lists
        n, wpr = len(lost), hdr["wpr"]
        # the image against an independent computation, list by list in the plan's order
        assert wpr > 0 and out_w != 0 and out_w == hdr["off_wout"] and hdr["out_n"] == n
        assert hdr["out_pad"] % 64 == 0 and hdr["out_pad"] == (n + 63) & ~63
        assert hdr["total_bytes"] >= hdr["off_wout"] + 4 * wpr * hdr["out_pad"] and len(plan) == hdr["total_bytes"]
        assert hdr["off_wout"] >= hdr["off_wneed"] + 4 * wpr * hdr["need_pad"] > 0  # (a part of its own, behind the needed-pivot view)
        want, inact, slots = _expected_rows(orc, K, plan, hdr, rows)
        assert sorted(rows.tolist()) == lost.tolist()
        assert [sorted(int(s) for s in cols[cptr[q]:cptr[q + 1]]) for q in range(n)] == slots
        image = _u32(plan, hdr["off_wout"], wpr * hdr["out_pad"]).reshape(wpr, hdr["out_pad"])
        _check_image(image, want, n)
        with_inact += sum(inact)
        pivcol = _u16(plan, hdr["off_pivcol"], hdr["npiv"])
        assert sum(inact) == n and pivcol.max() < prm["W"]  # (see the head of the file: a source symbol's list is never of pivots only)
        # the segmented run (W transposed and the image filled afterwards) leaves the same plan bytes
        plan2, _ = emu_device_plan(K, kc, lost, rep_esis, split=True)
        assert plan2 == plan

        # the host's builder over the host planner's plan of the same reception: the same identity against that plan's wt
        isis, rowsrc = decode_setup(orc, K, lost, rep_esis)
        hplan = nanorq_amd.host_plan(K, isis, kc)
        hh = nanorq_amd.plan_header(hplan)
        assert hh["status"] == 0 and hh["off_wout"] == 0 and hh["off_needslot"] == 0
        hcptr, hcols, order = _host_lists(K, _u16(hplan, hh["off_colslot"], hh["L"]), lost)
        hwant, _, hslots = _expected_rows(orc, K, hplan, hh, lost[order])
        assert [sorted(int(s) for s in hcols[hcptr[q]:hcptr[q + 1]]) for q in range(n)] == hslots
        _check_image(_host_image(hplan, hcptr, hcols, hh["wpr"]), hwant, n)

        rep, ref_inter, _ = orc.encode_block(src, K, T, rep_esis, want_inter=True)
        # no intermediate symbols, the planner's own job: nothing is back-substituted, the lost rows are the source's
        work = src.copy()
        work[lost] = 0x5A
        assert _solve(plan, kc, rowsrc, work, rep, (cptr, cols), rows, out_w) == 1
        assert np.array_equal(work, src)
        # ... the same over the host's plan, lists and image (appended to the arena, as the host decode uploads them)
        himg = _host_image(hplan, hcptr, hcols, hh["wpr"])
        off = (len(hplan) + 15) & ~15
        work = src.copy()
        work[lost] = 0xA5
        assert _solve(hplan + bytes(off - len(hplan)) + himg.tobytes(), kc, rowsrc, work, rep, (hcptr, hcols), lost[order], off) == 1
        assert np.array_equal(work, src)
        # with intermediate symbols the image is left alone: every intermediate symbol is the oracle's, the lost rows too
        work = src.copy()
        work[lost] = 0x3C
        inter = np.zeros((prm["L"], T), np.uint8)
        assert _solve(plan, kc, rowsrc, work, rep, (cptr, cols), rows, out_w, inter) == 1
        assert np.array_equal(inter, ref_inter) and np.array_equal(work, src)
        # a job that brings its own lists, in row order, has out_w = 0: the needed-pivot view of the same plan serves it
        work = src.copy()
        work[lost] = 0xC3
        assert hdr["off_needslot"] != 0
        assert _solve(plan, kc, rowsrc, work, rep, lt_lists(orc, K, lost, plan), lost, 0) == 1
        assert np.array_equal(work, src)
        # lists of pivots only (and one of each mixture), made for it: the symbol is the XOR of the named columns' intermediate symbols
        pivslot, uslot = _u16(plan, hdr["off_pivslot"], hdr["npiv"]), _u16(plan, hdr["off_uslot"], hdr["u"])
        ucol = np.nonzero(~np.isin(np.arange(prm["L"]), pivcol))[0]
        colslot = _u16(plan, hdr["off_colslot"], hdr["L"])
        assert len(ucol) == hdr["u"] and sorted(colslot[ucol].tolist()) == sorted(uslot.tolist())
        ks = [0, hdr["npiv"] // 2, hdr["npiv"] - 1]
        made = [[int(pivcol[k])] for k in ks] + [[int(pivcol[ks[0]]), int(pivcol[ks[1]])], [int(pivcol[ks[2]])] * 2,
                                               [int(pivcol[ks[1]]), int(ucol[0])], [int(ucol[-1])]]
        mcptr = np.cumsum([0] + [len(m) for m in made]).astype(np.uint32)
        mcols = np.array([colslot[c] for m in made for c in m], np.uint16)
        mimg = _host_image(plan, mcptr, mcols, wpr)  # (the builder takes any plan with pivslot[] and wt[])
        assert mimg[:, :3].any() and not mimg[:, 4].any() and not mimg[:, 6].any()  # (a pivot twice cancels; a parked column adds nothing)
        assert np.array_equal(mimg[:, 5], mimg[:, 1]) and np.array_equal(mimg[:, 3], mimg[:, 0] ^ mimg[:, 1])
        off = (len(plan) + 15) & ~15
        got = np.full((len(made), T), 0x77, np.uint8)
        work = src.copy()
        assert _solve(plan + bytes(off - len(plan)) + mimg.tobytes(), kc, rowsrc, work, rep, (mcptr, mcols), np.arange(len(made)), off,
                      out=got) == 1
        for q, m in enumerate(made):
            assert np.array_equal(got[q], np.bitwise_xor.reduce(ref_inter[m], axis=0)), (q, m)
        done += 1
    assert done >= 1 and with_inact >= 1


def test_encode_plans_carry_no_out_view(orc):
    K = 1000
    kc = nanorq_amd.host_kconst(K)
    _, hdr = emu_device_plan(K, kc, [], [], encode=True)
    assert hdr["status"] == 0
    assert (hdr["off_wout"], hdr["out_pad"], hdr["out_n"], hdr["off_out_cptr"], hdr["off_out_slots"]) == (0, 0, 0, 0, 0)
