"""The output lists of a solve job (nrq_job out_cptr / out_slots / out_row) as their two builders leave them: the device planner's
final phases (planner_body.h, emulated) and the host's build_out_lists (out_lists.h: encode calls, host-planned decodes).
Both put the lists in non-increasing length, equal lengths in the order the symbols were given in -- ph_store deals the lists to
its threads in the stored order -- and out_row[] goes with them."""
import ctypes as C

import numpy as np
import pytest

import nanorq_amd
from emu_support import Job, pemu
from util import loss_pattern

U32P = C.POINTER(C.c_uint32)
_OLEMU = None


def _olemu():
    """tests/emu/libout_lists_emu.so: build_out_lists of out_lists.h behind a C entry point"""
    global _OLEMU
    if _OLEMU is None:
        from nanorq_amd import build as nbuild
        _OLEMU = C.CDLL(nbuild.build_out_lists_emu())
    return _OLEMU


def _device_lists(K, kc, lost, rep_esis):
    """emu_plan's job: (header, colslot[], cptr, cols, rows) out of the arena"""
    L_ = pemu()
    kcb = (C.c_uint8 * len(kc)).from_buffer_copy(kc)
    lost = np.ascontiguousarray(lost, np.uint32)
    rep_esis = np.ascontiguousarray(rep_esis, np.uint32)
    cap = L_.emu_plan_arena_bound(K, C.addressof(kcb), 24, len(lost) + 8)
    arena = np.zeros(cap, np.uint8)
    job = Job()
    rc = L_.emu_plan(K, 0, C.addressof(kcb), lost.ctypes.data_as(U32P), len(lost), rep_esis.ctypes.data_as(U32P), len(rep_esis),
                     len(rep_esis), arena.ctypes.data, cap, 140 * 1024, C.byref(job))
    assert rc == 0
    hdr = nanorq_amd.plan_header(arena.tobytes()[:256])
    assert hdr["status"] == 0 and job.nout == len(lost)
    base = arena.ctypes.data
    n = job.nout
    cptr = np.frombuffer(arena, np.uint32, count=n + 1, offset=job.out_cptr - base).copy()
    rows = np.frombuffer(arena, np.uint32, count=n, offset=job.out_row - base).copy()
    cols = np.frombuffer(arena, np.uint16, count=int(cptr[n]), offset=job.out_slots - base).copy()
    colslot = np.frombuffer(arena, np.uint16, count=hdr["L"], offset=hdr["off_colslot"]).copy()
    return hdr, colslot, cptr, cols, rows


def _host_lists(K, colslot, isis):
    """build_out_lists: (cptr, cols, order)"""
    L_ = _olemu()
    L_.emu_out_lists.restype = C.c_uint32
    L_.emu_out_lists.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    isis = np.ascontiguousarray(isis, np.uint32)
    colslot = np.ascontiguousarray(colslot, np.uint16)
    n = len(isis)
    cptr, order, cols = np.zeros(n + 1, np.uint32), np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1) * 64, np.uint16)
    m = L_.emu_out_lists(K, 0, colslot.ctypes.data, n, isis.ctypes.data, cptr.ctypes.data, cols.ctypes.data, len(cols), order.ctypes.data)
    assert m != 0xFFFFFFFF and m == cptr[n]
    return cptr, cols[:m], order[:n]


def _pairs(cptr, cols, rows):
    return sorted((int(rows[i]), tuple(sorted(int(s) for s in cols[cptr[i]:cptr[i + 1]]))) for i in range(len(rows)))


def _direct(orc, K, colslot, isis, rows):
    """(destination row, sorted slot list) of every symbol, from the LT tuples and colslot[]"""
    return sorted((int(r), tuple(sorted(int(colslot[c]) for c in orc.lt_columns(K, int(x))))) for x, r in zip(isis, rows))


def _non_increasing(cptr):
    ln = np.diff(cptr.astype(np.int64))
    return bool(np.all(ln[1:] <= ln[:-1])), ln


def _stable(cptr, keys):
    """equal lengths in ascending order of `keys` (the order the symbols were given in)"""
    ln = np.diff(cptr.astype(np.int64))
    return all(ln[i] != ln[i + 1] or keys[i] < keys[i + 1] for i in range(len(ln) - 1))


@pytest.mark.parametrize("K,p,seed", [(10, 0.3, 1), (10, 0.6, 2), (100, 0.06, 1), (100, 0.4, 3), (1000, 0.05, 1), (1000, 0.1, 2),
                                      (1000, 0.5, 3)])
def test_decode_lists_of_both_planners(orc, K, p, seed):
    lost = loss_pattern(K, p, seed)
    assert len(lost)
    kc = nanorq_amd.host_kconst(K)
    rep_esis = np.arange(K, K + len(lost) + 2, dtype=np.uint32)
    hdr, colslot, cptr, cols, rows = _device_lists(K, kc, lost, rep_esis)
    want = _direct(orc, K, colslot, lost, lost)  # (the ISI of a source symbol is its ESI, its row in `out` too)
    assert _pairs(cptr, cols, rows) == want
    ok, ln = _non_increasing(cptr)
    assert ok, ln
    assert ln.min() >= 1 and ln.max() <= 33 and _stable(cptr, rows)
    # the host's builder over the same colslot[]: the same arrays, entry for entry
    hcptr, hcols, order = _host_lists(K, colslot, lost)
    hrows = lost[order]
    assert np.array_equal(hcptr, cptr) and np.array_equal(hcols, cols) and np.array_equal(hrows, rows)
    # ... and over the host planner's own plan (other slots, the same lengths: the same order)
    prm = orc.params(K)
    isis = np.arange(prm["Kp"], dtype=np.uint32)
    isis[lost] = rep_esis[:len(lost)] + (prm["Kp"] - K)
    isis = np.concatenate([isis, rep_esis[len(lost):] + (prm["Kp"] - K)])
    plan = nanorq_amd.host_plan(K, isis, kc)
    h2 = nanorq_amd.plan_header(plan)
    assert h2["status"] == 0
    colslot2 = np.frombuffer(plan, np.uint16, count=h2["L"], offset=h2["off_colslot"])
    cptr2, cols2, order2 = _host_lists(K, colslot2, lost)
    assert np.array_equal(order2, order) and np.array_equal(cptr2, cptr)
    assert _pairs(cptr2, cols2, lost[order2]) == _direct(orc, K, colslot2, lost, lost)


@pytest.mark.parametrize("K,nrep", [(10, 1), (10, 40), (100, 63), (1000, 769)])
def test_encode_lists_of_the_host_builder(orc, K, nrep):
    prm = orc.params(K)
    kc = nanorq_amd.host_kconst(K)
    plan = nanorq_amd.host_plan(K, np.arange(prm["Kp"], dtype=np.uint32), kc)
    hdr = nanorq_amd.plan_header(plan)
    assert hdr["status"] == 0
    colslot = np.frombuffer(plan, np.uint16, count=hdr["L"], offset=hdr["off_colslot"])
    isis = np.arange(K, K + nrep, dtype=np.uint32) + (prm["Kp"] - K)
    cptr, cols, order = _host_lists(K, colslot, isis)
    assert sorted(order.tolist()) == list(range(nrep))  # out_row[i] = order[i]: every row of `rep` once
    assert _pairs(cptr, cols, order) == _direct(orc, K, colslot, isis, np.arange(nrep))
    ok, ln = _non_increasing(cptr)
    assert ok and _stable(cptr, order), ln


def test_no_lists():
    cptr, cols, order = _host_lists(100, np.zeros(200, np.uint16), np.zeros(0, np.uint32))
    assert cptr.tolist() == [0] and len(cols) == 0 and len(order) == 0
