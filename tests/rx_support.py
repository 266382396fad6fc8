"""Test support for the device-resident receiver (nrq_rx_*): the CPU emulation of its ingest kernels
(tests/emu/ingest_emu.cpp over nanorq_amd/csrc/ingest_body.h), a plain Python model of the rules, and packet builders."""
import ctypes as C

import numpy as np

from nanorq_amd import build as nbuild

ERR, ADDED, IGN, DUP, FULL = -1, 0, 1, 2, 3
UNTOUCHED = 77  # result entries of packets outside a reception keep what they held

_EMU = None


def emu_lib():
    global _EMU
    if _EMU is None:
        L = C.CDLL(nbuild.build_ingest_emu())
        vp, u64 = C.c_void_p, C.c_uint64
        L.emu_rx_add.argtypes = [vp, vp, u64, vp, u64, vp, vp, vp, vp, vp, vp, vp, u64, vp, C.c_uint32, vp]
        _EMU = L
    return _EMU


def tag(sbn, esi):
    return (int(sbn) << 24) | int(esi)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class EmuRx:
    """The reception's state in numpy arrays, advanced by the emulated kernels."""

    def __init__(self, K, T, nblk, rep_cap, sbn0=0, max_esi=0, Kp=None):
        if not max_esi:
            max_esi = 2 * Kp
        self.K, self.T, self.nblk, self.rep_cap, self.sbn0, self.max_esi = K, T, nblk, rep_cap, sbn0, max_esi
        self.m1 = max_esi + 1
        self.bm_words = max_esi // 32 + 1
        self.src = np.zeros((nblk, K, T), np.uint8)
        self.rep = np.zeros((nblk, rep_cap, T), np.uint8)
        self.first = np.full(nblk * self.m1, 0xFFFFFFFF, np.uint32)
        self.seen = np.zeros(nblk * self.bm_words, np.uint32)
        self.gaps = np.full(nblk, K, np.uint32)
        self.nrep = np.zeros(nblk, np.uint32)
        self.rep_esi = np.zeros(nblk * rep_cap, np.uint32)
        self.live = np.zeros(nblk, np.uint32)

    def add(self, pkts, tags=None, results=None):
        """pkts: [n, stride] uint8; tags: [n] uint32 or None (inline FEC Payload IDs).  Returns the result codes."""
        pkts = np.ascontiguousarray(pkts, np.uint8)
        n = pkts.shape[0]
        res = np.full(n, UNTOUCHED, np.int32) if results is None else results
        tg = None if tags is None else np.ascontiguousarray(tags, np.uint32)
        prm = np.array([self.K, self.T, self.nblk, self.sbn0, self.max_esi, self.rep_cap], np.uint32)
        rc = emu_lib().emu_rx_add(_p(prm), _p(self.src), self.K * self.T, _p(self.rep), self.rep_cap * self.T, _p(self.first), _p(self.seen),
                             _p(self.gaps), _p(self.nrep), _p(self.rep_esi), _p(self.live), _p(pkts), pkts.shape[1], _p(tg), n, _p(res))
        assert rc == 0, "a packet's destination row was left unwritten"
        return res

    def seen_bits(self, b):
        w = self.seen[b * self.bm_words:(b + 1) * self.bm_words]
        return np.unpackbits(w.view(np.uint8), bitorder="little")[:self.m1].astype(bool)

    def lost(self, b):
        return np.flatnonzero(~self.seen_bits(b)[:self.K]).astype(np.uint32)

    def rep_list(self, b):
        return self.rep_esi[b * self.rep_cap: b * self.rep_cap + int(self.nrep[b])].copy()

    def mark_complete(self, b):
        """what a successful decode does to the books (nrq_ing_mark_kernel)"""
        for e in range(self.K):
            self.seen[b * self.bm_words + e // 32] |= np.uint32(1 << (e % 32))
        self.gaps[b] = 0


class ModelRx:
    """The rules, one packet after the other (nanorq_decoder_add_symbol plus rep_cap)."""

    def __init__(self, K, T, nblk, rep_cap, sbn0=0, max_esi=0, Kp=None):
        self.K, self.T, self.nblk, self.rep_cap, self.sbn0 = K, T, nblk, rep_cap, sbn0
        self.max_esi = max_esi or 2 * Kp
        self.seen = [set() for _ in range(nblk)]
        self.missing = [set(range(K)) for _ in range(nblk)]
        self.reps = [[] for _ in range(nblk)]
        self.src = np.zeros((nblk, K, T), np.uint8)
        self.rep = np.zeros((nblk, rep_cap, T), np.uint8)

    def add(self, payloads, tags, results=None):
        n = len(tags)
        res = np.full(n, UNTOUCHED, np.int32) if results is None else results
        for k in range(n):
            t = int(tags[k])
            sbn, esi = t >> 24, t & 0xFFFFFF
            if not (self.sbn0 <= sbn < self.sbn0 + self.nblk):
                continue
            b = sbn - self.sbn0
            if esi > self.max_esi:
                r = ERR
            elif not self.missing[b]:
                r = IGN
            elif esi in self.seen[b]:
                r = DUP
            elif esi < self.K:
                r = ADDED
                self.src[b, esi] = payloads[k]
                self.missing[b].discard(esi)
                self.seen[b].add(esi)
            elif len(self.reps[b]) >= self.rep_cap:
                r = FULL
            else:
                r = ADDED
                self.rep[b, len(self.reps[b])] = payloads[k]
                self.reps[b].append(esi)
                self.seen[b].add(esi)
            res[k] = r
        return res

    def lost(self, b):
        return np.array(sorted(self.missing[b]), np.uint32)

    def mark_complete(self, b):
        self.seen[b] |= set(range(self.K))
        self.missing[b] = set()


def inline_packets(payloads, tags, stride=None):
    """packets with the RFC 6330 section 3.2 FEC Payload ID in front: [n, stride] uint8"""
    payloads = np.ascontiguousarray(payloads, np.uint8)
    n, T = payloads.shape
    stride = stride or T + 4
    out = np.zeros((n, stride), np.uint8)
    out[:, :4] = np.ascontiguousarray(tags, np.uint32).astype(">u4").view(np.uint8).reshape(n, 4)
    out[:, 4:4 + T] = payloads
    return out


def random_stream(rng, K, nblk, sbn0, max_esi, n, sbn_span=0, dup=0.1, over=0.02):
    """tags of a messy reception: every block's source and some repair ESIs, shuffled, with duplicates, ESIs above max_esi and
    (sbn_span > 0) SBNs of neighbouring blocks outside the reception"""
    tags = []
    lo, hi = max(0, sbn0 - sbn_span), min(256, sbn0 + nblk + sbn_span)
    for _ in range(n):
        sbn = int(rng.integers(lo, hi))
        u = rng.random()
        if u < over:
            esi = int(rng.integers(max_esi + 1, max_esi + 40))
        elif u < 0.6:
            esi = int(rng.integers(0, K))
        else:
            esi = int(rng.integers(K, min(max_esi + 1, K + 3 * K // 10 + 8)))
        tags.append(tag(sbn, esi))
    tags = np.array(tags, np.uint32)
    nd = int(len(tags) * dup)
    if nd:
        extra = tags[rng.integers(0, len(tags), nd)]
        tags = np.concatenate([tags, extra])
        rng.shuffle(tags)
    return tags


def payloads_for(tags, T, salt=0):
    """deterministic payload bytes of each tag (equal tags carry equal bytes, as real duplicates do)"""
    t = np.asarray(tags, np.uint64)
    j = np.arange(T, dtype=np.uint64)
    x = (t[:, None] * np.uint64(2654435761) + j[None, :] * np.uint64(40503) + np.uint64(salt)) >> np.uint64(7)
    return (x & np.uint64(0xFF)).astype(np.uint8)
