"""Test support for held symbols (NRQ_TX_HELD, nrq_rx_held): the CPU emulation of the held emit and of the held listing
(nanorq_amd/csrc/held_emu.cpp over emit_body.h and held_body.h), driven from the emulated receptions of rx_support.EmuRx."""
import ctypes as C

import numpy as np

from nanorq_amd import build as nbuild
from relay_support import mask_words
from tx_support import FILL, _p

TX_HELD = 2

_EMU = None


def emu_lib():
    global _EMU
    if _EMU is None:
        L = C.CDLL(nbuild.build_held_emu())
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        L.emu_emit_held.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, u32, u32, vp, u64, vp]
        L.emu_rx_held.argtypes = [vp, vp, vp, vp, vp, u32, vp]
        _EMU = L
    return _EMU


POISON_WORDS = 64  # words of all ones behind a seen bitmap handed to the emulation: a read past the bitmap shows as "held"


def emu_emit_held(rxs, Kps, inters, span, ready, tags, inline, stride):
    """The held emit over a relay's table: segment g reads the emulated reception rxs[g] (rx_support.EmuRx; K' = Kps[g]) and the
    intermediate symbols inters[g] ([nblk, L, T]); ready: bool per block of the span -> (packets [n, stride], results [n])"""
    nseg, T = len(rxs), rxs[0].T
    prm = np.array([[r.K, Kp, T, r.nblk, r.sbn0] for r, Kp in zip(rxs, Kps)], np.uint32)
    srcs = [np.ascontiguousarray(r.src.reshape(r.nblk, -1)) for r in rxs]
    inters = [np.ascontiguousarray(a, np.uint8) for a in inters]
    seens = [np.concatenate([r.seen, np.full(POISON_WORDS, 0xFFFFFFFF, np.uint32)]) for r in rxs]
    reps = [np.ascontiguousarray(r.rep.reshape(r.nblk, -1)) for r in rxs]

    def per_seg(ctype, vals):
        return (ctype * nseg)(*vals)
    tags = np.ascontiguousarray(tags, np.uint32)
    n = len(tags)
    res = np.full(n, 77, np.int32)
    pkts = np.full((n, stride), FILL, np.uint8)
    rc = emu_lib().emu_emit_held(
        _p(prm), nseg, _p(np.array(span, np.uint32)),
        per_seg(C.c_void_p, [a.ctypes.data for a in srcs]), per_seg(C.c_uint64, [a.shape[1] for a in srcs]),
        per_seg(C.c_void_p, [a.ctypes.data for a in inters]), per_seg(C.c_uint64, [a.shape[1] * T for a in inters]),
        _p(mask_words(ready)),
        per_seg(C.c_void_p, [a.ctypes.data for a in seens]), per_seg(C.c_uint32, [r.bm_words for r in rxs]),
        per_seg(C.c_void_p, [r.rep_esi.ctypes.data for r in rxs]), per_seg(C.c_void_p, [r.nrep.ctypes.data for r in rxs]),
        per_seg(C.c_uint32, [r.rep_cap for r in rxs]),
        per_seg(C.c_void_p, [a.ctypes.data for a in reps]), per_seg(C.c_uint64, [a.shape[1] for a in reps]),
        _p(tags), n, int(inline), _p(pkts), stride, _p(res))
    assert rc == 0, rc
    return pkts, res


def emu_rx_held(rx, cap=None):
    """the held listing of one emulated reception -> (rc, n, tags [cap]); cap None: exactly the count (asked for first)"""
    prm = np.array([rx.K, rx.nblk, rx.sbn0, rx.max_esi, rx.rep_cap], np.uint32)
    n = C.c_uint32(0)
    rc = emu_lib().emu_rx_held(_p(prm), _p(rx.seen), _p(rx.nrep), _p(rx.rep_esi), None, 0, C.byref(n))
    assert rc == 0
    if cap is None:
        cap = n.value
    out = np.full(cap + 4, 0xDEADBEEF, np.uint32)  # (four guard words behind the list)
    rc = emu_lib().emu_rx_held(_p(prm), _p(rx.seen), _p(rx.nrep), _p(rx.rep_esi), _p(out), cap, C.byref(n))
    assert (out[cap:] == 0xDEADBEEF).all()
    return rc, n.value, out[:cap]


def host_held(sbn0, K, seen_src, rep_lists):
    """the list as the header states it, built on the host: per block the seen source ESIs (bool [K]) ascending, then its repair
    ESIs in arrival order"""
    out = []
    for b, (seen, reps) in enumerate(zip(seen_src, rep_lists)):
        sbn = np.uint32((sbn0 + b) << 24)
        out.append(sbn | np.flatnonzero(np.asarray(seen)[:K]).astype(np.uint32))
        out.append(sbn | np.asarray(reps, np.uint32))
    return np.concatenate(out).astype(np.uint32) if out else np.zeros(0, np.uint32)
