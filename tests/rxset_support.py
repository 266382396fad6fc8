"""Test support for reception sets (nrq_rxset_*): the CPU emulation of the set's ingest kernels (nanorq_amd/csrc/rxset_emu.cpp over
ingest_set_body.h) on the state arrays of rx_support.EmuRx members, member mixes, and keyed packet streams."""
import ctypes as C

import numpy as np

from nanorq_amd import build as nbuild
from rx_support import ERR, IGN, UNTOUCHED, EmuRx, ModelRx, payloads_for, random_stream, tag

_EMU = None
UNKNOWN_KEY = 0x7E57AB1E  # no mix below uses it


def emu_lib():
    global _EMU
    if _EMU is None:
        L = C.CDLL(nbuild.build_rxset_emu())
        vp = C.c_void_p
        L.emu_rxset_add.argtypes = [C.c_uint32, vp, vp, vp, C.c_uint64, vp, vp, C.c_uint32, C.c_uint32, vp]
        _EMU = L
    return _EMU


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class EmuSet:
    """The emulated set over EmuRx members: add() advances the members' own arrays, so a member's own add() between two set calls
    works on the same books."""

    def __init__(self):
        self.members = []  # (key, EmuRx, objZ)

    def attach(self, key, emu, objZ=0):
        self.members.append((key, emu, objZ))

    def add(self, pkts, keys=None, tags=None, key_inline=False, results=None):
        """pkts [n, stride] uint8; keys / tags [n] uint32 or None.  Returns the result codes; raises if the poison check trips."""
        pkts = np.ascontiguousarray(pkts, np.uint8)
        n = pkts.shape[0]
        res = np.full(n, UNTOUCHED, np.int32) if results is None else results
        ks = None if keys is None else np.ascontiguousarray(keys, np.uint32)
        tg = None if tags is None else np.ascontiguousarray(tags, np.uint32)
        prm = np.array([[e.K, e.T, e.nblk, e.sbn0, e.max_esi, e.rep_cap, k, z] for k, e, z in self.members], np.uint32).reshape(-1, 8)
        ptr = np.array([[a.ctypes.data for a in (e.src, e.rep, e.first, e.seen, e.gaps, e.nrep, e.rep_esi, e.live)]
                        for _, e, _ in self.members], np.uint64).reshape(-1, 8)
        rc = emu_lib().emu_rxset_add(len(self.members), _p(prm), _p(ptr), _p(pkts), pkts.shape[1], _p(ks), _p(tg), int(key_inline), n, _p(res))
        assert rc != -1, "a packet's destination row was left unwritten by the classify pass"
        assert rc == 0, rc
        return res


# (key, K, nblk, sbn0): two block classes of one key, the same SBNs under another key, a reception at the top of the SBN range
MIX4 = [(5, 10, 3, 0), (5, 100, 5, 3), (9, 100, 4, 0), (0, 26, 2, 250)]
# six members, 360 blocks: block counters beyond 256
MIX360 = [(1, 10, 60, 0), (1, 10, 60, 60), (1, 10, 60, 120), (1, 10, 60, 180), (2, 10, 60, 0), (2, 10, 60, 60)]


def rep_cap_of(K, small):
    """repair rows per block: `small` leaves some blocks of a random_stream overflowing (FULL)"""
    return 2 if small else K // 2 + 12


def keyed_stream(rng, mix, kps, n, unknown=0.05, sbn_span=2, exact=False):
    """(keys, tags) of about n packets (exact: of n): a random_stream per member (duplicates, ESIs above max_esi, neighbouring SBNs), tagged with
    the member's key, merged and shuffled, with packets of an unknown key mixed in"""
    ks, ts = [], []
    blocks = sum(m[2] for m in mix)
    for (key, K, nblk, sbn0), Kp in zip(mix, kps):
        t = random_stream(rng, K, nblk, sbn0, 2 * Kp, max(1, n * nblk // blocks), sbn_span=sbn_span)
        ts.append(t)
        ks.append(np.full(len(t), key, np.uint32))
    nu = int(n * unknown)
    if nu:
        _, K, nblk, sbn0 = mix[0]
        ts.append(random_stream(rng, K, nblk, sbn0, 2 * kps[0], nu, dup=0))
        ks.append(np.full(nu, UNKNOWN_KEY, np.uint32))
    keys, tags = np.concatenate(ks), np.concatenate(ts)
    perm = rng.permutation(len(tags))
    if exact:
        assert len(perm) >= n
        perm = perm[:n]
    return keys[perm], tags[perm]


def keyed_payloads(keys, tags, T):
    """deterministic payload bytes of each (key, tag): equal keys and tags carry equal bytes"""
    out = payloads_for(tags, T)
    return out ^ (np.asarray(keys, np.uint32).astype(np.uint64) * np.uint64(37) + np.uint64(11)).astype(np.uint8)[:, None]


def packets(payloads, keys, tags, carrier, stride_extra=0):
    """The four carriers -> (pkts [n, stride], keys or None, tags or None, inline, key_inline).
    "arrays": keys and tags beside bare payloads; "nokeys": tags only (every key 0); "inline": FEC Payload ID in the packet, keys
    beside; "keyinline": key and FEC Payload ID in the packet."""
    payloads = np.ascontiguousarray(payloads, np.uint8)
    n, T = payloads.shape
    be = lambda a: np.ascontiguousarray(a, np.uint32).astype(">u4").view(np.uint8).reshape(n, 4)
    hdr = {"arrays": 0, "nokeys": 0, "inline": 4, "keyinline": 8}[carrier]
    pk = np.zeros((n, hdr + T + stride_extra), np.uint8)
    pk[:, hdr:hdr + T] = payloads
    if carrier == "inline":
        pk[:, :4] = be(tags)
    elif carrier == "keyinline":
        pk[:, :4] = be(keys)
        pk[:, 4:8] = be(tags)
    return (pk, None if carrier in ("nokeys", "keyinline") else keys, None if hdr else tags, hdr > 0, carrier == "keyinline")


def expected_codes(members, keys, tags, payloads, objects=()):
    """The oracle: each member (key, rx with .add(payloads, tags)) fed exactly the packets that carry its key, in packet
    order; its codes land in those packets' entries.  objects: (key, Z, max_esi) of attached objects (the SBN >= Z rule)."""
    exp = np.full(len(tags), UNTOUCHED, np.int32)
    for key, rx in members:
        sel = np.flatnonzero(keys == key)
        if not len(sel):
            continue
        r = rx.add(payloads[sel], tags[sel])
        hit = r != UNTOUCHED
        assert (exp[sel[hit]] == UNTOUCHED).all()
        exp[sel[hit]] = r[hit]
    for key, Z, max_esi in objects:
        sel = np.flatnonzero((keys == key) & ((tags >> 24) >= Z))
        exp[sel] = np.where((tags[sel] & 0xFFFFFF) > max_esi, ERR, IGN)
    return exp


__all__ = ["EmuSet", "EmuRx", "ModelRx", "MIX4", "MIX360", "UNKNOWN_KEY", "UNTOUCHED", "keyed_stream", "keyed_payloads", "packets",
           "expected_codes", "rep_cap_of", "tag"]
