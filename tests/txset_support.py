"""Test support for sender sets (nrq_txset_*): the CPU emulation of the set's emit kernels (nanorq_amd/csrc/txset_emu.cpp over
emit_set_body.h) on tables of host arrays, and keyed tag lists over the member mixes of rxset_support."""
import ctypes as C

import numpy as np

import nanorq_amd
from nanorq_amd import build as nbuild
from held_support import POISON_WORDS
from tx_support import FILL, random_tags, tag

FOREIGN, NOT_READY = -1, -2
UNKNOWN_KEY = 0x7E57AB1E  # no mix uses it

_EMU = None


def emu_lib():
    global _EMU
    if _EMU is None:
        L = C.CDLL(nbuild.build_txset_emu())
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        L.emu_txset_emit.argtypes = [u32, vp, vp, vp, vp, vp, u32, u32, u32, vp, u64, vp, vp]
        _EMU = L
    return _EMU


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class Seg:
    """One table segment: nblk blocks of (K, K', T) from SBN sbn0 under `key`.  src [nblk, K, T] (or [nblk, >= K*T]), inter
    [nblk, L, T]; rx: the emulated reception (rx_support.EmuRx) a relay's segment reads, else None; ready: bool per block."""

    def __init__(self, key, K, Kp, T, sbn0, src, inter, rx=None, ready=None):
        self.key, self.K, self.Kp, self.T, self.sbn0 = key, K, Kp, T, sbn0
        self.nblk = src.shape[0]
        self.src = np.ascontiguousarray(src.reshape(self.nblk, -1), np.uint8)
        self.inter = np.ascontiguousarray(inter, np.uint8)
        self.rx = rx
        self.ready = np.ones(self.nblk, bool) if ready is None else np.asarray(ready, bool)


def table_order(segs):
    """the segments in the order of the set's table: sorted by (key, first SBN)"""
    return sorted(segs, key=lambda s: (s.key, s.sbn0))


def global_blocks(segs, keys, tags):
    """the set's global block of every (key, tag), len(blocks) for a packet of no member -- worked out here, not by the emulation"""
    segs = table_order(segs)
    nb = sum(s.nblk for s in segs)
    keys = np.zeros(len(tags), np.uint32) if keys is None else np.asarray(keys, np.uint32)
    sbn = np.asarray(tags, np.uint32) >> 24
    out = np.full(len(tags), nb, np.int64)
    g0 = 0
    for s in segs:
        hit = (keys == s.key) & (sbn >= s.sbn0) & (sbn < s.sbn0 + s.nblk)
        out[hit] = g0 + sbn[hit].astype(np.int64) - s.sbn0
        g0 += s.nblk
    return out, nb


def emu_txset_emit(segs, keys, tags, hdr, stride, held=False):
    """The emulated set emit -> (packets [n, stride], results [n], work order [n]).  hdr: 0, 4 (tag inline) or 8 (key and tag)."""
    segs = table_order(segs)
    tags = np.ascontiguousarray(tags, np.uint32)
    ks = None if keys is None else np.ascontiguousarray(keys, np.uint32)
    n = len(tags)
    prm = np.zeros((max(1, len(segs)), 8), np.uint32)
    ptr = np.zeros((max(1, len(segs)), 9), np.uint64)
    keep = []
    bits = []
    for g, s in enumerate(segs):
        prm[g, :6] = (s.K, s.Kp, s.T, s.nblk, s.sbn0, s.key)
        ptr[g, :4] = (s.src.ctypes.data, s.src.shape[1], s.inter.ctypes.data, s.inter.shape[1] * s.T)
        if s.rx is not None:
            r = s.rx
            seen = np.concatenate([r.seen, np.full(POISON_WORDS, 0xFFFFFFFF, np.uint32)])  # a read past the bitmap shows as "held"
            rep = np.ascontiguousarray(r.rep.reshape(r.nblk, -1))
            keep += [seen, rep]
            prm[g, 6:] = (r.bm_words, r.rep_cap)
            ptr[g, 4:] = (seen.ctypes.data, r.rep_esi.ctypes.data, r.nrep.ctypes.data, rep.ctypes.data, rep.shape[1])
        bits.append(s.ready)
    bits = np.concatenate(bits) if bits else np.zeros(0, bool)
    ready = np.zeros(32, np.uint32)
    for g in np.flatnonzero(bits):
        ready[g >> 5] |= np.uint32(1 << (g & 31))
    pkts = np.full((n, stride), FILL, np.uint8)
    res = np.full(n, 77, np.int32)
    order = np.full(max(1, n), 0xFFFFFFFF, np.uint32)
    rc = emu_lib().emu_txset_emit(len(segs), _p(prm), _p(ptr), _p(ready), _p(ks), _p(tags), n, hdr, int(held), _p(pkts), stride, _p(res),
                                  _p(order))
    assert rc == 0, rc
    return pkts, res, order[:n]


def mix_segs(rng, mix, T):
    """a sender Seg with random rows per member (key, K, nblk, sbn0) of a mix of rxset_support"""
    out = []
    for key, K, nblk, sbn0 in mix:
        Kp = nanorq_amd.params(K)["Kp"]
        L = nanorq_amd.params(Kp)["L"]
        out.append(Seg(key, K, Kp, T, sbn0, rng.integers(0, 256, (nblk, K, T), dtype=np.uint8),
                       rng.integers(0, 256, (nblk, L, T), dtype=np.uint8)))
    return out


def keyed_tags(rng, segs, n, objects=()):
    """(keys, tags) of exactly n packets: random_tags per segment under its key (with SBNs next to it: foreign ones), packets of an
    unknown key, and for objects (key, Z) SBNs >= Z under the object's key; shuffled"""
    ks, ts = [], []
    per = max(1, n // max(1, len(segs)))
    for s in segs:
        t = random_tags(rng, s.K, s.nblk, s.sbn0, per)
        ts.append(t)
        ks.append(np.full(len(t), s.key, np.uint32))
    t = random_tags(rng, segs[0].K, segs[0].nblk, segs[0].sbn0, max(2, n // 16))
    ts.append(t)
    ks.append(np.full(len(t), UNKNOWN_KEY, np.uint32))
    for key, Z in objects:
        t = np.array([tag(min(255, Z + i), 3 + i) for i in range(3) if Z + i < 256], np.uint32)
        ts.append(t)
        ks.append(np.full(len(t), key, np.uint32))
    keys, tags = np.concatenate(ks), np.concatenate(ts)
    while len(tags) < n:  # (top up with the first segment's)
        t = random_tags(rng, segs[0].K, segs[0].nblk, segs[0].sbn0, n - len(tags))
        tags = np.concatenate([tags, t])
        keys = np.concatenate([keys, np.full(len(t), segs[0].key, np.uint32)])
    perm = rng.permutation(len(tags))[:n]
    return keys[perm].astype(np.uint32), tags[perm].astype(np.uint32)


def be32(a):
    a = np.ascontiguousarray(a, np.uint32)
    return a.astype(">u4").view(np.uint8).reshape(len(a), 4)


__all__ = ["Seg", "FILL", "FOREIGN", "NOT_READY", "UNKNOWN_KEY", "emu_txset_emit", "global_blocks", "table_order", "mix_segs", "keyed_tags",
           "be32", "tag"]
