"""CPU tier: which view a device-planned decode without intermediate symbols gets -- the out view (plan.h off_wout, nrq_job out_w)
or, without it, the needed-pivot view (off_needslot / off_wneed) -- and that the second is whole when the first is withheld.

A plan gets no out view in two cases: its job carries PL_MODE_NO_OUTW (the option plan_no_out_view, tests: the planner emulation's
switch 0x800 of emu_plan_set_mode), or pl_final_b finds no room for the image behind the needed-pivot view.  In both the job's
out_w is 0 and the solve back-substitutes the needed pivots (solve_body.h ph_backsub).  Here the planner's phase code runs emulated
on the CPU (tests/emu/planner_emu.cpp) and the solve too (tests/emu/solve_emu.cpp), with the job record the planner wrote: its
lists in the planner's order (by length), not the row-ordered lists tests/test_need_view_emu.py makes for itself.

What "the same plan apart from the image" means below: every byte in front of the default plan's off_wout, except the header words
that describe the image (off_wout, out_pad, out_n, and off_out_cptr / off_out_slots, which pl_final_d sets with them for
pl_wt_fill) and total_bytes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import nanorq_amd
from emu_support import Job, decode_setup, emu, pemu
from nanorq_amd.binding import PLAN_FIELDS
from util import loss_pattern, payload, received_set

U32P = C.POINTER(C.c_uint32)
T, WB = 16, 16
NO_OUT_VIEW = 0x800   # emu_plan_set_mode: the job carries PL_MODE_NO_OUTW
SPLIT = 0x100         # ... the phase sequence in its two parts, W images filled afterwards (pl_wt_fill = nrq_wt_kernel)
PL_FAIL_CAPACITY = 2
IMAGE_WORDS = ("off_wout", "out_pad", "out_n", "off_out_cptr", "off_out_slots", "total_bytes")


def _u16(buf, off, n):
    return np.frombuffer(buf, np.uint16, count=n, offset=off)


def _u32(buf, off, n):
    return np.frombuffer(buf, np.uint32, count=n, offset=off)


def _full_cap(K, kc, lost, rep_esis):
    kcb = (C.c_uint8 * len(kc)).from_buffer_copy(kc)
    return pemu().emu_plan_arena_bound(K, C.addressof(kcb), max(0, len(rep_esis) - len(lost)) + 24, len(lost) + 8)  # (= emu_device_plan's)


def _plan(K, kc, lost, rep_esis, mode=0, cap=None):
    """emu_plan with its job record: (arena bytes up to total_bytes, header, (cptr, cols, rows) as the job names them or None, out_w).
    cap: the job's arena_cap (the buffer itself always has the full bound's bytes)."""
    L_ = pemu()
    kcb = (C.c_uint8 * len(kc)).from_buffer_copy(kc)
    lost = np.ascontiguousarray(lost, np.uint32)
    rep_esis = np.ascontiguousarray(rep_esis, np.uint32)
    full = _full_cap(K, kc, lost, rep_esis)
    arena = np.zeros(full, np.uint8)
    job = Job()
    L_.emu_plan_set_caps(0, 0)
    L_.emu_plan_set_mode(mode)
    try:
        rc = L_.emu_plan(K, 0, C.addressof(kcb), lost.ctypes.data_as(U32P), len(lost), rep_esis.ctypes.data_as(U32P), len(rep_esis),
                         len(rep_esis), arena.ctypes.data, full if cap is None else cap, 140 * 1024, C.byref(job))
    finally:
        L_.emu_plan_set_mode(0)
    assert rc == 0
    hdr = nanorq_amd.plan_header(arena.tobytes()[:256])
    if hdr["status"] != 0:
        return arena.tobytes()[:256], hdr, None, 0
    base, n = arena.ctypes.data, job.nout
    assert job.plan == base and n == len(lost) and hdr["total_bytes"] <= (full if cap is None else cap)
    cptr = _u32(arena, job.out_cptr - base, n + 1).copy()
    rows = _u32(arena, job.out_row - base, n).copy()
    cols = _u16(arena, job.out_slots - base, int(cptr[n])).copy()
    return arena.tobytes()[:hdr["total_bytes"]], hdr, (cptr, cols, rows), job.pad  # (pad: the record's last word, out_w)


def _solve(plan, kc, rowsrc, work, rep, lists, out_w):
    """The emulated solve of a job that wants no intermediate symbols, lists as the planner's job record names them."""
    planb = (C.c_uint8 * len(plan)).from_buffer_copy(plan)
    kcb = (C.c_uint8 * len(kc)).from_buffer_copy(kc)
    cptr, cols, rows = lists
    slots = np.concatenate([cols, np.zeros(64, np.uint16)])  # (what ph_store may read past a list: NRQ_STORE_SLACK)
    j = Job()
    j.plan = C.addressof(planb)
    j.rowsrc = rowsrc.ctypes.data
    j.src = work.ctypes.data
    j.rep = rep.ctypes.data
    j.inter = 0
    j.out = work.ctypes.data
    j.out_cptr = cptr.ctypes.data
    j.out_slots = slots.ctypes.data
    j.out_row = rows.ctypes.data
    j.nout = len(rows)
    j.pad = out_w
    return emu().emu_solve(C.byref(j), T, WB, C.addressof(kcb))


def _same_but_the_image(plan, hdr, ref, ref_hdr):
    """`plan` (without the image) against the default plan `ref`: see the head of the file"""
    end = ref_hdr["off_wout"]
    assert 0 < end <= len(plan) and hdr["total_bytes"] == len(plan) == end  # (the image was the last part: nothing else moved)
    a, b = np.frombuffer(plan, np.uint32, count=end // 4).copy(), np.frombuffer(ref, np.uint32, count=end // 4).copy()
    for f in IMAGE_WORDS:
        a[PLAN_FIELDS.index(f)] = b[PLAN_FIELDS.index(f)] = 0
    bad = np.nonzero(a != b)[0]
    assert bad.size == 0, ("first differing words (byte offsets)", (bad[:8] * 4).tolist(), {k: v for k, v in ref_hdr.items() if k.startswith("off_")})


def _need_view(plan, hdr):
    assert hdr["off_needslot"] != 0 and hdr["off_wneed"] != 0 and 0 < hdr["nneed"] <= hdr["need_pad"] and hdr["need_pad"] % 64 == 0
    return (hdr["nneed"], _u16(plan, hdr["off_needslot"], hdr["nneed"]).tolist(),
            _u32(plan, hdr["off_wneed"], hdr["wpr"] * hdr["need_pad"]).tolist())


def _reception(K, p, seed):
    lost = loss_pattern(K, p, seed)
    esis = received_set(K, lost, 2)
    return lost, esis[esis >= K]


@pytest.mark.parametrize("K", [100, 1000, 8192, 10000])
@pytest.mark.parametrize("p", [0.05, 0.10, 0.30])
def test_plan_with_and_without_the_out_view(orc, K, p):
    """The same reception planned by default and with the out view withheld: the flagged plan is the default one without its last
    part, its job has out_w == 0, the segmented run leaves the same bytes, and the emulated solve of the planner's own job record
    (needed-pivot view, lists by length) gives the source's rows."""
    src = payload(K * T, seed=29).reshape(K, T)
    kc = nanorq_amd.host_kconst(K)
    done = 0
    for seed in (1, 2):
        lost, rep_esis = _reception(K, p, seed)
        assert len(lost)
        ref, rh, _, ref_w = _plan(K, kc, lost, rep_esis)
        if rh["status"] != 0:
            continue  # (rank deficient: the oracle's verdict too, tests/test_out_view_emu.py)
        assert ref_w != 0 and ref_w == rh["off_wout"] and len(ref) == rh["total_bytes"]
        plan, hdr, lists, out_w = _plan(K, kc, lost, rep_esis, NO_OUT_VIEW)
        assert hdr["status"] == 0
        assert (hdr["off_wout"], hdr["out_pad"], hdr["out_n"]) == (0, 0, 0) and out_w == 0
        assert _need_view(plan, hdr) == _need_view(ref, rh)
        _same_but_the_image(plan, hdr, ref, rh)
        # bit 10 of the job's mode is not the segmented run's bit 8: pl_final_c has transposed W (pl_need_b has written wneed: above)
        wt = _u32(plan, hdr["off_wt"], hdr["wpr"] * hdr["npiv_pad"])
        assert wt.any() and np.array_equal(wt, _u32(ref, rh["off_wt"], rh["wpr"] * rh["npiv_pad"]))
        # the segmented run (W images by pl_wt_fill afterwards) leaves the same bytes
        plan2, hdr2, lists2, out_w2 = _plan(K, kc, lost, rep_esis, NO_OUT_VIEW | SPLIT)
        assert plan2 == plan and out_w2 == 0 and all(np.array_equal(x, y) for x, y in zip(lists, lists2))
        # the planner's job record: lists by length (not in row order once two lengths differ), every missing symbol once
        cptr, cols, rows = lists
        assert sorted(rows.tolist()) == lost.tolist()
        lens = np.diff(cptr.astype(np.int64))
        assert (lens[:-1] >= lens[1:]).all()
        rep, _, _ = orc.encode_block(src, K, T, rep_esis)
        _, rowsrc = decode_setup(orc, K, lost, rep_esis)
        work = src.copy()
        work[lost] = 0x5A
        assert _solve(plan, kc, rowsrc, work, rep, lists, 0) == 1
        assert np.array_equal(work, src)
        done += 1
    assert done >= 1


def _final_b_lines():
    """the source lines of pl_final_b (fail_site is the __LINE__ that raised PL_FAIL_CAPACITY)"""
    path = os.path.join(os.path.dirname(os.path.abspath(nanorq_amd.__file__)), "csrc", "planner_body.h")
    first = last = None
    with open(path) as f:
        for i, line in enumerate(f, 1):
            if re.search(r"\bvoid pl_final_b\(", line):
                first = i
            elif first and last is None and re.search(r"\bvoid pl_final_c\(", line):
                last = i
    assert first and last
    return first, last


@pytest.mark.parametrize("K,p", [(100, 0.10), (1000, 0.05), (1000, 0.30), (8192, 0.10)])
def test_room_rule_of_the_out_view(orc, K, p):
    """pl_final_b: the image comes last and only if it fits the arena (o <= cap and oend <= cap); without it the plan is good and the
    needed-pivot view serves; without room for that view the plan fails with PL_FAIL_CAPACITY, raised in pl_final_b.
    o and oend are the default plan's off_wout and total_bytes.  (The layout in front of o does not depend on arena_cap: every
    earlier use of it is a check that fails the plan -- asserted here by the capped plans' bytes being the default plan's.)"""
    src = payload(K * T, seed=31).reshape(K, T)
    kc = nanorq_amd.host_kconst(K)
    lost, rep_esis = _reception(K, p, 1)
    ref, rh, ref_lists, ref_w = _plan(K, kc, lost, rep_esis)
    assert rh["status"] == 0 and ref_w != 0
    o, oend = rh["off_wout"], rh["total_bytes"]
    assert o == (rh["off_wneed"] + 4 * rh["wpr"] * rh["npiv_pad"] + 15) & ~15  # (the end of the needed-pivot view's part: room for every pivot)
    assert oend == (o + 4 * rh["wpr"] * rh["out_pad"] + 15) & ~15 and oend < _full_cap(K, kc, lost, rep_esis)
    # exactly enough room: the image is there
    plan, hdr, lists, out_w = _plan(K, kc, lost, rep_esis, cap=oend)
    assert hdr["status"] == 0 and plan == ref and out_w == ref_w
    # 16 bytes short of it: a good plan without the image
    plan, hdr, lists, out_w = _plan(K, kc, lost, rep_esis, cap=oend - 16)
    assert hdr["status"] == 0 and (hdr["off_wout"], hdr["out_pad"], hdr["out_n"]) == (0, 0, 0) and out_w == 0
    assert _need_view(plan, hdr) == _need_view(ref, rh)
    _same_but_the_image(plan, hdr, ref, rh)
    assert all(np.array_equal(x, y) for x, y in zip(lists, ref_lists))
    rep, _, _ = orc.encode_block(src, K, T, rep_esis)
    _, rowsrc = decode_setup(orc, K, lost, rep_esis)
    work = src.copy()
    work[lost] = 0x5A
    assert _solve(plan, kc, rowsrc, work, rep, lists, 0) == 1
    assert np.array_equal(work, src)
    # the needed-pivot view itself ends exactly at the cap: still good
    plan, hdr, _, out_w = _plan(K, kc, lost, rep_esis, cap=o)
    assert hdr["status"] == 0 and hdr["off_wout"] == 0 and out_w == 0 and hdr["total_bytes"] == o
    # 16 bytes short of that: no plan, and pl_final_b says so
    _, hdr, _, _ = _plan(K, kc, lost, rep_esis, cap=o - 16)
    first, last = _final_b_lines()
    assert hdr["status"] == 1 and hdr["reserved0"] == PL_FAIL_CAPACITY and first < hdr["fail_site"] < last, hdr
