"""CPU tier: the needed-pivot view of device-planned decodes (plan.h off_needslot / off_wneed).

A decode that asks for no intermediate symbols reads only the slots named by the missing symbols' LT lists, so the GPU
planner lists the pivots whose slot is among them and the solve's back-substitution runs over those alone.  Here the
planner's phase code runs emulated on the CPU (tests/emu/planner_emu.cpp): the view must be exactly the set computed
independently from the plan's maps and the oracle's LT lists, its W image the matching columns of the full one, an
emulated solve that takes it must give the oracle's lost rows, and the full view must still give every intermediate
symbol."""
import ctypes as C

import numpy as np
import pytest

import nanorq_amd
from emu_support import Job, decode_setup, emu, emu_device_plan, emu_solve, lt_lists
from util import loss_pattern, payload, received_set


def _u16(plan, off, n):
    return np.frombuffer(plan, np.uint16, count=n, offset=off)


def _u32(plan, off, n):
    return np.frombuffer(plan, np.uint32, count=n, offset=off)


def _needed_pivots(orc, K, lost, plan, hdr):
    """Pivots k (ascending) whose slot occurs in a missing symbol's LT list, from pivslot / colslot and the oracle."""
    colslot = _u16(plan, hdr["off_colslot"], hdr["L"])
    pivslot = _u16(plan, hdr["off_pivslot"], hdr["npiv"])
    named = np.zeros(hdr["M"], bool)
    for e in lost:
        for col in orc.lt_columns(K, int(e)):
            named[colslot[col]] = True
    return np.nonzero(named[pivslot])[0]


def _solve_without_inter(plan, kc, rowsrc, work, rep, T, lists, lost, wb):
    """The emulated solve with a job that wants no intermediate symbols (job.inter = 0): lost rows go into `work`."""
    planb = (C.c_uint8 * len(plan)).from_buffer_copy(plan)
    kcb = (C.c_uint8 * len(kc)).from_buffer_copy(kc)
    cptr, cols = lists
    rows = np.ascontiguousarray(lost, np.uint32)
    j = Job()
    j.plan = C.addressof(planb)
    j.rowsrc = rowsrc.ctypes.data
    j.src = work.ctypes.data
    j.rep = rep.ctypes.data
    j.inter = 0
    j.out = work.ctypes.data
    j.out_cptr = cptr.ctypes.data
    j.out_slots = cols.ctypes.data
    j.out_row = rows.ctypes.data
    j.nout = len(rows)
    return emu().emu_solve(C.byref(j), T, wb, C.addressof(kcb))


@pytest.mark.parametrize("K", [100, 1000, 8192, 10000])
@pytest.mark.parametrize("p", [0.05, 0.10, 0.30])
def test_needed_pivots_match_the_lost_lists(orc, K, p):
    T, wb = 16, 16
    prm = orc.params(K)
    src = payload(K * T, seed=21).reshape(K, T)
    kc = nanorq_amd.host_kconst(K)
    done = 0
    for seed in range(1, 3):
        lost = loss_pattern(K, p, seed)
        if len(lost) == 0:
            continue
        esis = received_set(K, lost, 2)
        rep_esis = esis[esis >= K]
        plan, hdr = emu_device_plan(K, kc, lost, rep_esis)
        if hdr["status"] != 0:
            continue
        # the view: exactly the pivots the out lists name, ascending, and W's matching columns
        need = _needed_pivots(orc, K, lost, plan, hdr)
        assert hdr["off_needslot"] != 0 and hdr["off_wneed"] != 0
        assert hdr["nneed"] == len(need) and hdr["need_pad"] % 64 == 0 and hdr["nneed"] <= hdr["need_pad"]
        pivslot = _u16(plan, hdr["off_pivslot"], hdr["npiv"])
        assert np.array_equal(_u16(plan, hdr["off_needslot"], hdr["nneed"]), pivslot[need])
        wpr = hdr["wpr"]
        wt = _u32(plan, hdr["off_wt"], wpr * hdr["npiv_pad"]).reshape(wpr, hdr["npiv_pad"])
        wneed = _u32(plan, hdr["off_wneed"], wpr * hdr["need_pad"]).reshape(wpr, hdr["need_pad"])
        assert np.array_equal(wneed[:, :hdr["nneed"]], wt[:, need])
        assert not wneed[:, hdr["nneed"]:].any()
        assert hdr["total_bytes"] >= hdr["off_wneed"] + 4 * wpr * hdr["need_pad"]
        # the segmented run (big blocks on the GPU: W transposed afterwards, nrq_wt_kernel) builds the same plan, view included
        plan2, _ = emu_device_plan(K, kc, lost, rep_esis, split=True)
        assert plan2 == plan

        rep, ref_inter, _ = orc.encode_block(src, K, T, rep_esis, want_inter=True)
        _, rowsrc = decode_setup(orc, K, lost, rep_esis)
        lists = lt_lists(orc, K, lost, plan)
        # a job without intermediate symbols takes the view: the lost rows are the oracle's
        work = src.copy()
        work[lost] = 0x5A
        assert _solve_without_inter(plan, kc, rowsrc, work, rep, T, lists, lost, wb) == 1
        assert np.array_equal(work, src)
        # a job with them takes the full view: every intermediate symbol is the oracle's
        work = src.copy()
        work[lost] = 0x3C
        r, inter = emu_solve(plan, kc, rowsrc, work, rep, T, prm["L"], lists, lost, work, wb)
        assert r == 1 and np.array_equal(work, src) and np.array_equal(inter, ref_inter)
        done += 1
    assert done >= 1


def test_encode_plans_carry_no_view(orc):
    """An encode plan is shared by every call, whatever symbols it is asked for: it must keep the full view only."""
    K = 1000
    kc = nanorq_amd.host_kconst(K)
    _, hdr = emu_device_plan(K, kc, [], [], encode=True)
    assert hdr["status"] == 0
    assert hdr["off_needslot"] == 0 and hdr["off_wneed"] == 0 and hdr["nneed"] == 0


def test_host_plans_carry_no_view(orc):
    """Plans of the host planner take the full back-substitution (the header's view fields stay 0)."""
    K = 1000
    p = orc.params(K)
    kc = nanorq_amd.host_kconst(K)
    lost = loss_pattern(K, 0.1, 1)
    esis = received_set(K, lost, 2)
    isis, _ = decode_setup(orc, K, lost, esis[esis >= K])
    hdr = nanorq_amd.plan_header(nanorq_amd.host_plan(K, isis, kc))
    assert hdr["status"] == 0 and hdr["npiv"] + hdr["u"] == p["L"]
    assert hdr["off_needslot"] == 0 and hdr["nneed"] == 0
