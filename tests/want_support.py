"""Test support for the want listing (nrq_rx_want / nrq_orx_want): a numpy model written from the words of include/nanorq_hip.h,
the CPU emulation of the listing (nanorq_amd/csrc/want_emu.cpp over want_body.h) over the emulated receptions of
rx_support.EmuRx, and the receptions both tiers list -- the CPU tier through the emulation, the GPU tier on the device."""
import ctypes as C

import numpy as np

import nanorq_amd
from nanorq_amd import build as nbuild
from rx_support import _p, tag

WANT_SOURCE = 1

_EMU = None


def emu_lib():
    global _EMU
    if _EMU is None:
        L = C.CDLL(nbuild.build_want_emu())
        vp, u32 = C.c_void_p, C.c_uint32
        L.emu_rx_want.argtypes = [vp, vp, vp, vp, u32, u32, u32, vp, u32, vp]
        _EMU = L
    return _EMU


POISON_WORDS = 64  # words of all ZEROS behind a seen bitmap handed to the emulation: a read past the bitmap shows as a wanted ESI
GUARD = 0xDEADBEEF


def host_want(sbn0, K, max_esi, rep_cap, seen, gaps, nrep, extra=0, source=False, esi_from=0):
    """The list as the header states it.  seen: per block a bool array over the ESIs 0 .. max_esi; gaps: missing source symbols
    per block; nrep: repair symbols booked per block."""
    out = [np.zeros(0, np.uint32)]
    for b in range(len(gaps)):
        g = int(gaps[b])
        if g == 0:  # complete: nothing, in either mode
            continue
        bits = np.asarray(seen[b], bool)
        assert len(bits) == max_esi + 1
        if source:  # the g source ESIs < K whose seen bit is clear, ascending
            es = np.flatnonzero(~bits[:K])
            assert len(es) == g
        else:
            r = min(int(nrep[b]), rep_cap)
            need = min(max(g + extra - r, 0), rep_cap - r)
            lo = max(K, esi_from)
            es = (lo + np.flatnonzero(~bits[lo:max_esi + 1]))[:need] if lo <= max_esi else np.zeros(0, np.int64)
        out.append((((sbn0 + b) << 24) | es).astype(np.uint32))
    return np.concatenate(out)


def model_books(mod):
    """(seen, gaps, nrep) of a rx_support.ModelRx, in host_want's form"""
    seen = np.zeros((mod.nblk, mod.max_esi + 1), bool)
    for b in range(mod.nblk):
        seen[b, sorted(mod.seen[b])] = True
    return seen, [len(m) for m in mod.missing], [len(r) for r in mod.reps]


def model_want(mod, extra=0, source=False, esi_from=0):
    return host_want(mod.sbn0, mod.K, mod.max_esi, mod.rep_cap, *model_books(mod), extra=extra, source=source, esi_from=esi_from)


def emu_rx_want(rx, flags=0, extra=0, esi_from=0, cap=None, count_only=False):
    """the want listing of one emulated reception (rx_support.EmuRx) -> (rc, n, tags [cap]); cap None: exactly the count (asked
    for first, with a NULL list).  Four guard words lie behind the list, POISON_WORDS zero words behind the bitmap."""
    prm = np.array([rx.K, rx.nblk, rx.sbn0, rx.max_esi, rx.rep_cap], np.uint32)
    seen = np.concatenate([rx.seen, np.zeros(POISON_WORDS, np.uint32)])
    n = C.c_uint32(0)
    rc = emu_lib().emu_rx_want(_p(prm), _p(seen), _p(rx.gaps), _p(rx.nrep), flags, extra, esi_from, None, 0, C.byref(n))
    if count_only or rc != 0:
        return rc, n.value, np.zeros(0, np.uint32)
    if cap is None:
        cap = n.value
    out = np.full(cap + 4, GUARD, np.uint32)
    rc = emu_lib().emu_rx_want(_p(prm), _p(seen), _p(rx.gaps), _p(rx.nrep), flags, extra, esi_from, _p(out), cap, C.byref(n))
    assert (out[cap:] == GUARD).all(), "guard words"
    return rc, n.value, out[:cap]


# ------------------------------------------------------------------------------------------------ the receptions listed ----
NBLK, SBN0 = 3, 5
BIG = 1 << 24  # the largest extra the call takes


class Case:
    """A reception (nblk = 3 at sbn0 = 5), the stream of tags it ingests, in order, and the queries (source, extra, esi_from) put
    to it."""

    def __init__(self, name, K, rep_cap, stream, queries, max_esi=0):
        self.name, self.K, self.rep_cap, self.queries = name, K, rep_cap, queries
        self.Kp = nanorq_amd.params(K)["Kp"]
        self.max_esi = max_esi or 2 * self.Kp
        self.stream = np.array([tag(SBN0 + b, e) for b, e in stream], np.uint32)

    def __repr__(self):
        return self.name


def _blk(b, esis):
    return [(b, int(e)) for e in esis]


def _one_word():
    """K = 10, max_esi = 20: one seen word per block.  Block 0 complete (with a repair symbol in before it completed), block 1
    untouched, block 2 with every repair row used (a fifth repair symbol got FULL)"""
    s = _blk(0, [11]) + _blk(0, range(10)) + _blk(2, [0, 2, 3, 5, 7, 8]) + _blk(2, [11, 14, 20, 12, 13])
    q = [(True, 0, 0)] + [(False, x, 0) for x in (0, 1, 2, BIG)] + [(False, 2, f) for f in (12, 19, 20, 21)]
    return Case("one_word", 10, 4, s, q)


def _free_rows():
    """rep_cap = 4.  Block 0: 3 missing, repair ESI 12 in (the list skips it); block 1: 1 missing, 2 repair symbols in (a surplus of
    1: wants nothing until extra is 2); block 2: 5 missing, 3 repair rows used (g + extra - r = 5 at extra 3: one free row, lists 1)"""
    s = _blk(0, [0, 1, 2, 3, 5, 7, 9]) + _blk(0, [12]) + _blk(1, range(1, 10)) + _blk(1, [10, 11]) + \
        _blk(2, [0, 1, 2, 3, 4]) + _blk(2, [10, 15, 16])
    return Case("free_rows", 10, 4, s, [(True, 0, 0)] + [(False, x, 0) for x in (0, 1, 2, 3)])


def _boundary(K):
    """lo = K on bit 31 / 0 / 1 of a seen word; esi_from inside a word, on a word boundary, at max_esi and above it"""
    rng = np.random.default_rng(K)
    Kp = nanorq_amd.params(K)["Kp"]
    max_esi = 2 * Kp
    s = []
    for b in range(NBLK):
        s += _blk(b, np.flatnonzero(rng.random(K) >= 0.3))
        s += _blk(b, rng.choice(np.arange(K, max_esi + 1), 6, replace=False))
    s += _blk(1, [K, max_esi])  # (DUP if the draw had them: the books are the same)
    wb = (K // 32 + 1) * 32  # the first word boundary above K
    q = [(True, 0, 0)] + [(False, x, 0) for x in (0, 2, 40)] + \
        [(False, 40, f) for f in (K - 1, K, K + 3, wb, max_esi - 1, max_esi, max_esi + 1, (1 << 24) - 1, 0xFFFFFFFF)]
    return Case("boundary_K%d" % K, K, 48, s, q)


def _short_range(K):
    """max_esi = K': the repair range holds K' - K + 1 ESIs, far fewer than are needed"""
    Kp = nanorq_amd.params(K)["Kp"]
    s = _blk(0, range(2, K)) + _blk(1, range(0, K, 2)) + (_blk(1, [Kp]) if Kp > K else [])
    return Case("short_range_K%d" % K, K, 100, s, [(True, 0, 0), (False, 0, 0), (False, 1000, 0), (False, 1000, Kp), (False, 1000, Kp + 1)], max_esi=Kp)


def _rounds_source():
    """K = 8200: 257 seen words per block, two fill rounds.  Block 0 has every 3rd symbol, block 1 nothing, block 2 the other two
    thirds"""
    K = 8200
    e = np.arange(K)
    s = _blk(0, e[e % 3 == 0]) + _blk(2, e[e % 3 != 0]) + _blk(2, [K + 4])
    return Case("rounds_source", K, 4, s, [(True, 0, 0), (False, 0, 0), (False, 2, 0)])


def _rounds_repair():
    """K = 10, rep_cap = 9000, extra = 8600: thousands of repair ESIs, the list crosses 256 seen words.  Block 0: 2 missing, every
    7th repair ESI below 3000 in; block 1 untouched; block 2 complete"""
    s = _blk(0, range(2, 10)) + _blk(0, range(10, 3000, 7)) + _blk(2, range(10))
    return Case("rounds_repair", 10, 9000, s, [(False, 8600, 0), (False, 8600, 5000), (False, 8600, 8191), (False, BIG, 0), (True, 0, 0)],
                max_esi=20000)


# (built on first use, not on import: a Case asks the library for K', and loading the library while pytest collects would open the
# HIP runtime before torch has found the device)
_BUILDERS = {"one_word": _one_word, "free_rows": _free_rows, "boundary_K31": lambda: _boundary(31), "boundary_K32": lambda: _boundary(32),
             "boundary_K33": lambda: _boundary(33), "short_range_K10": lambda: _short_range(10), "short_range_K31": lambda: _short_range(31),
             "rounds_source": _rounds_source, "rounds_repair": _rounds_repair}
CASE_NAMES = list(_BUILDERS)
_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = _BUILDERS[name]()
        assert _CASES[name].name == name
    return _CASES[name]
