"""Test support for relays (nrq_rx_relay / nrq_orx_relay): the CPU emulation of the emit over a table WITH a ready mask
(emu_emit_table_ready of nanorq_amd/csrc/emit_emu.cpp), and lossy receptions of one block list built from the oracle."""
import ctypes as C

import numpy as np

import tx_support
from tx_support import FILL, _p

NOT_READY = -2  # NRQ_TX_NOT_READY
FOREIGN = -1

_DECLARED = False


def _lib():
    global _DECLARED
    L = tx_support.emu_lib()
    if not _DECLARED:
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        L.emu_emit_table_ready.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp, u32, vp, u32, vp, u64, vp, vp, vp]
        _DECLARED = True
    return L


def mask_words(ready):
    """bool per block of the span -> the 8 words of tx_src::ready"""
    bits = np.zeros(256, np.uint8)
    bits[:len(ready)] = np.asarray(ready, bool)
    return np.packbits(bits, bitorder="little").view(np.uint32).copy()


def emu_emit_table_ready(segs, span, T, inline, stride, ready, tags=None, rng=None):
    """tx_support.emu_emit_table with a ready mask (bool per block of the span)"""
    srcs = [np.ascontiguousarray(s[3].reshape(s[3].shape[0], -1), np.uint8) for s in segs]
    inters = [np.ascontiguousarray(s[4], np.uint8) for s in segs]
    prm = np.array([[K, Kp, T, src.shape[0], sbn0] for (K, Kp, sbn0, _, _), src in zip(segs, srcs)], np.uint32)
    nseg = len(segs)

    def per_seg(ctype, vals):
        return (ctype * nseg)(*vals)
    sbn0, Z, ZL = span
    if tags is not None:
        tags = np.ascontiguousarray(tags, np.uint32)
        n = len(tags)
        out = np.full(n, 77, np.int32)
        res, tags_out, range_ = out, None, None
    else:
        esi0, nL, nS, _ = rng
        n = ZL * nL + (Z - ZL) * nS
        out = np.zeros(n, np.uint32)
        res, tags_out, range_ = None, out, np.array(rng, np.uint32)
    pkts = np.full((n, stride), FILL, np.uint8)
    rc = _lib().emu_emit_table_ready(_p(prm), nseg, _p(np.array(span, np.uint32)),
                                     per_seg(C.c_void_p, [a.ctypes.data for a in srcs]), per_seg(C.c_uint64, [a.shape[1] for a in srcs]),
                                     per_seg(C.c_void_p, [a.ctypes.data for a in inters]),
                                     per_seg(C.c_uint64, [a.shape[1] * T for a in inters]), _p(tags), n if tags is not None else 0,
                                     _p(range_), int(inline), _p(pkts), stride, _p(res), _p(tags_out), _p(mask_words(ready)))
    assert rc == 0, rc
    return pkts, out
