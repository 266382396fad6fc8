"""The device-resident object layout (nanorq_amd/csrc/obj_body.h) on the CPU: the body nrq_obj_layout_kernel runs, driven by
tests/emu/obj_emu.cpp, against a plain numpy model of the RFC 6330 section 4.4.1.2 layout.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

from nanorq_amd import build as nbuild

GUARD = 48
GFILL = 0xEE


@pytest.fixture(scope="module")
def emu():
    L = C.CDLL(nbuild.build_obj_emu())
    L.emu_obj_layout.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    L.emu_obj_layout.restype = C.c_int
    return L


def partition(I, J):
    IL, IS = -(-I // J), I // J
    JL = I - IS * J
    return (IL if JL else 0), IS, JL, J - JL


def layout(Kt, Z, T, N, Al):
    KL, KS, ZL, ZS = partition(Kt, Z)
    uL, uS, NL, NS = partition(T // Al, N)
    return dict(T=T, Z=Z, ZL=ZL, KL=KL, ZS=ZS, KS=KS, NL=NL, TL=uL * Al, NS=NS, TS=uS * Al)


def blocks(p):
    """(K, object offset) of every block"""
    out, off = [], 0
    for b in range(p["Z"]):
        K = p["KL"] if b < p["ZL"] else p["KS"]
        out.append((K, off))
        off += K * p["T"]
    return out


def subs(p):
    """(column, width) of every sub-block"""
    out, col = [], 0
    for j in range(p["NL"] + p["NS"]):
        w = p["TL"] if j < p["NL"] else p["TS"]
        out.append((col, w))
        col += w
    return out


def model_rows(p, obj, F):
    """the row images, back to back, of an object of F bytes (bytes past F read as zero)"""
    T = p["T"]
    total = sum(K for K, _ in blocks(p)) * T
    pad = np.zeros(total, np.uint8)
    pad[:F] = obj[:F]
    rows = np.zeros(total, np.uint8)
    for K, off in blocks(p):
        img = rows[off:off + K * T].reshape(K, T)
        for col, w in subs(p):
            img[:, col:col + w] = pad[off + K * col:off + K * (col + w)].reshape(K, w)
    return rows


def _prm(p):
    return np.array([p[k] for k in ("T", "Z", "ZL", "KL", "KS", "NL", "TL", "NS", "TS")], np.uint32)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def run(emu, p, obj, F, rows, to_obj, V=0, mask=None):
    m = np.full(8, 0xFFFFFFFF, np.uint32) if mask is None else mask
    rc = emu.emu_obj_layout(_ptr(_prm(p)), _ptr(obj), F, _ptr(rows), int(to_obj), _ptr(m), V)
    assert rc > 0, rc
    return rc


def _aligned(n, off=0):
    """n bytes at a 64-byte boundary + off"""
    raw = np.empty(n + 64 + off, np.uint8)
    s = (-raw.ctypes.data) % 64 + off
    return raw[s:s + n]


def f_cases(p):
    """F = Kt*T, Kt*T - 1, and an F that ends inside a middle sub-block of the last block"""
    (K, off), T = blocks(p)[-1], p["T"]
    Kt = off // T + K
    col, w = subs(p)[len(subs(p)) // 2]
    mid = off + K * col + (K * w) // 2 + 1
    return sorted({Kt * T, Kt * T - 1, mid})


GRID = []
for N in (1, 2, 3, 5):
    for Al in (1, 4, 8):
        for units in (13, 160):
            for Kt, Z in ((23, 4), (10, 3), (7, 7)):
                if N <= units:
                    GRID.append((Kt, Z, units * Al, N, Al))


def test_grid_has_two_classes_and_unequal_subblocks():
    ps = [layout(*g) for g in GRID]
    assert any(p["ZL"] and p["ZS"] for p in ps)
    assert any(p["NL"] and p["NS"] and p["TL"] != p["TS"] for p in ps)
    assert any(layout(*g)["TL"] == 432 and layout(*g)["TS"] == 424 for g in [(10, 3, 1280, 3, 8)])


@pytest.mark.parametrize("Kt,Z,T,N,Al", GRID)
def test_layout_matches_model(emu, Kt, Z, T, N, Al):
    p = layout(Kt, Z, T, N, Al)
    assert p["NL"] * p["TL"] + p["NS"] * p["TS"] == T
    total = Kt * T
    rng = np.random.default_rng(Kt * 1000 + T + N)
    for F in f_cases(p):
        src = rng.integers(0, 256, F + GUARD, dtype=np.uint8)   # bytes past F are garbage that must read as zero
        want = model_rows(p, src, F)
        for obj_off in (0, 1):
            obj = _aligned(F + GUARD, obj_off)
            obj[:] = src
            for V in (0, 1):   # the library's width, and bytes
                rows = _aligned(total + GUARD)
                rows[:] = GFILL
                used = run(emu, p, obj, F, rows, 0, V)
                assert np.array_equal(rows[:total], want), (F, obj_off, used)
                assert (rows[total:] == GFILL).all()
                # rows -> object: the bytes before F come back, nothing at or past F is written
                out = _aligned(F + GUARD, obj_off)
                out[:] = GFILL
                run(emu, p, out, F, rows, 1, V)
                assert np.array_equal(out[:F], src[:F]), (F, obj_off, used)
                assert (out[F:] == GFILL).all(), (F, obj_off, used)


@pytest.mark.parametrize("Kt,Z,T,N,Al", [(23, 4, 1280, 3, 8), (10, 3, 52, 5, 4), (7, 7, 13, 2, 1)])
def test_masked_blocks_left_untouched(emu, Kt, Z, T, N, Al):
    """rows -> object writes only the blocks whose mask bit is set"""
    p = layout(Kt, Z, T, N, Al)
    F = f_cases(p)[1]
    rng = np.random.default_rng(3)
    src = rng.integers(0, 256, F, dtype=np.uint8)
    rows = _aligned(Kt * T)
    rows[:] = model_rows(p, src, F)
    mask = np.zeros(8, np.uint32)
    pick = [b for b in range(Z) if b % 2 == 0]
    for b in pick:
        mask[b >> 5] |= np.uint32(1 << (b & 31))
    out = _aligned(F + GUARD)
    out[:] = GFILL
    run(emu, p, out, F, rows, 1, 0, mask)
    for b, (K, off) in enumerate(blocks(p)):
        lo, hi = min(off, F), min(off + K * T, F)
        if b in pick:
            assert np.array_equal(out[lo:hi], src[lo:hi]), b
        else:
            assert (out[lo:hi] == GFILL).all(), b
    assert (out[F:] == GFILL).all()


def test_width_choice(emu):
    """16-byte row pieces where T, TL and TS allow them, else 8, 4, 2 or 1; a width wider than fits is refused"""
    cases = [((10, 3, 1280, 1, 8), 16), ((10, 3, 1280, 4, 8), 16), ((10, 3, 1280, 3, 8), 8), ((10, 3, 52, 1, 4), 4),
             ((10, 3, 13, 2, 1), 1), ((10, 3, 1284, 2, 4), 4), ((10, 3, 1282, 1, 2), 2)]
    for g, V in cases:
        p = layout(*g)
        F = g[0] * g[2]
        obj = _aligned(F)
        rows = _aligned(F)
        assert run(emu, p, obj, F, rows, 0) == V, (g, p)
        assert emu.emu_obj_layout(_ptr(_prm(p)), _ptr(obj), F, _ptr(rows), 0, None, 2 * V if V < 16 else 32) == -1
