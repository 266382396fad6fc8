"""Test support for a reception set's want and held listings with keys (nrq_rxset_want / nrq_rxset_held): the CPU emulation of
the listing (nanorq_amd/csrc/rxset_want_emu.cpp over want_set_body.h) on the state arrays of rx_support.EmuRx members, and a numpy
model written from the words of include/nanorq_hip.h: in rxset_decode_support.block_order, want_support.host_want per member's
block (and a held list built from the books in the same style), with the member's key repeated."""
import ctypes as C

import numpy as np

from nanorq_amd import build as nbuild
from rxset_decode_support import block_order
from want_support import GUARD, POISON_WORDS, WANT_SOURCE, host_want

_EMU = None
NGUARD = 4  # guard words behind the tags, the keys and the counts


def emu_lib():
    global _EMU
    if _EMU is None:
        L = C.CDLL(nbuild.build_rxset_want_emu())
        vp, u32 = C.c_void_p, C.c_uint32
        L.emu_rxset_want.argtypes = [u32, vp, vp, u32, u32, u32, vp, vp, u32, vp, vp]
        L.emu_rxset_held.argtypes = [u32, vp, vp, vp, vp, u32, vp, vp]
        _EMU = L
    return _EMU


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _table(members):
    """(prm, ptr, keep): the members as emu_rxset_add describes them, every seen bitmap a copy with POISON_WORDS zero words behind
    it (a read past the bitmap shows up as a wanted ESI); `keep` holds the copies alive"""
    prm = np.array([[e.K, e.T, e.nblk, e.sbn0, e.max_esi, e.rep_cap, k, z] for k, e, z in members], np.uint32).reshape(-1, 8)
    keep = [np.concatenate([e.seen, np.zeros(POISON_WORDS, np.uint32)]) for _, e, _ in members]
    ptr = np.array([[a.ctypes.data for a in (e.src, e.rep, e.first, s, e.gaps, e.nrep, e.rep_esi, e.live)]
                    for (_, e, _), s in zip(members, keep)], np.uint64).reshape(-1, 8)
    return prm, ptr, keep


def emu_list(members, what, flags=0, extra=0, esi_from=0, cap=None, with_keys=True, with_tags=True, raw_keys_only=False):
    """The emulated listing (`what`: "want" / "held") over [(key, EmuRx, objZ)] in any order -> (rc, n, counts [nb], keys [cap],
    tags [cap]).  cap None: exactly the total (asked for first, with NULL lists).  NGUARD guard words lie behind the tags, the keys
    and the counts; asserts that they are intact.  raw_keys_only: keys given without tags (the call refuses that)."""
    prm, ptr, keep = _table(members)
    nmem, nb = len(members), sum(e.nblk for _, e, _ in members)
    L = emu_lib()

    def call(keys, tags, cap, cnt, n):
        if what == "want":
            return L.emu_rxset_want(nmem, _p(prm), _p(ptr), flags, extra, esi_from, _p(keys), _p(tags), cap, _p(cnt), C.byref(n))
        return L.emu_rxset_held(nmem, _p(prm), _p(ptr), _p(keys), _p(tags), cap, _p(cnt), C.byref(n))

    n = C.c_uint32(0xFFFFFFFF)
    cnt = np.full(nb + NGUARD, GUARD, np.uint32)
    if raw_keys_only:
        keys = np.full(8 + NGUARD, GUARD, np.uint32)
        rc = call(keys, None, 8, cnt, n)
        assert (keys == GUARD).all()
        return rc, n.value, cnt[:nb], keys[:0], keys[:0]
    rc = call(None, None, 0, cnt, n)
    assert rc not in (-2, -3), rc
    assert (cnt[nb:] == GUARD).all(), "guard words behind the counts"
    if rc != 0 or not with_tags:
        return rc, n.value, cnt[:nb].copy(), np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    if cap is None:
        cap = n.value
    tags = np.full(cap + NGUARD, GUARD, np.uint32)
    keys = np.full(cap + NGUARD, GUARD, np.uint32) if with_keys else None
    cnt2 = np.full(nb + NGUARD, GUARD, np.uint32)
    n2 = C.c_uint32(0xFFFFFFFF)
    rc = call(keys, tags, cap, cnt2, n2)
    assert rc != -3, "a listing pass wrote behind the counts"
    assert (tags[cap:] == GUARD).all() and (cnt2[nb:] == GUARD).all() and (keys is None or (keys[cap:] == GUARD).all()), "guard words"
    assert n2.value == n.value and np.array_equal(cnt2[:nb], cnt[:nb])  # (the count call and the fill call agree)
    assert all(not s[-POISON_WORDS:].any() for s in keep)
    return rc, n2.value, cnt2[:nb].copy(), (keys[:cap] if with_keys else None), tags[:cap]


# ------------------------------------------------------------------------------------------------ the model: the header ----
def _books(e, b):
    """(seen bits [max_esi + 1], gaps, nrep) of block b of an EmuRx"""
    return e.seen_bits(b), int(e.gaps[b]), int(e.nrep[b])


def model_want(members, extra=0, source=False, esi_from=0):
    """(keys, tags, counts per block) of the set, from the header's words; members = [(key, EmuRx, objZ)]"""
    keys, tags, cnt = [np.zeros(0, np.uint32)], [np.zeros(0, np.uint32)], []
    for key, e, b in block_order([(k, e) for k, e, _ in members]):
        bits, g, nr = _books(e, b)
        t = host_want(e.sbn0 + b, e.K, e.max_esi, e.rep_cap, [bits], [g], [nr], extra=extra, source=source, esi_from=esi_from)
        tags.append(t)
        keys.append(np.full(len(t), key, np.uint32))
        cnt.append(len(t))
    return np.concatenate(keys), np.concatenate(tags), np.array(cnt, np.uint32)


def host_held(sbn, K, rep_cap, bits, nrep, rep_esi):
    """A block's held list as the header states it: the seen source ESIs ascending, then the repair ESIs in arrival order (the
    repair rows in use: min(nrep, rep_cap))"""
    es = np.concatenate([np.flatnonzero(np.asarray(bits, bool)[:K]), np.asarray(rep_esi[:min(int(nrep), rep_cap)], np.int64)])
    return ((sbn << 24) | es).astype(np.uint32)


def model_held(members):
    keys, tags, cnt = [np.zeros(0, np.uint32)], [np.zeros(0, np.uint32)], []
    for key, e, b in block_order([(k, e) for k, e, _ in members]):
        bits, _, nr = _books(e, b)
        t = host_held(e.sbn0 + b, e.K, e.rep_cap, bits, nr, e.rep_esi[b * e.rep_cap:(b + 1) * e.rep_cap])
        tags.append(t)
        keys.append(np.full(len(t), key, np.uint32))
        cnt.append(len(t))
    return np.concatenate(keys), np.concatenate(tags), np.array(cnt, np.uint32)


def check_want(members, extra=0, source=False, esi_from=0):
    """the emulated want listing of the set equals the model's: total, counts, keys, tags -> the model's (keys, tags, counts)"""
    mk, mt, mc = model_want(members, extra=extra, source=source, esi_from=esi_from)
    rc, n, cnt, keys, tags = emu_list(members, "want", WANT_SOURCE if source else 0, extra, esi_from)
    what = (source, extra, esi_from)
    assert rc == 0 and n == len(mt) == int(mc.sum()), (what, rc, n, len(mt))
    assert np.array_equal(cnt, mc), what
    assert np.array_equal(tags, mt), what
    assert np.array_equal(keys, mk), what
    return mk, mt, mc


def check_held(members):
    mk, mt, mc = model_held(members)
    rc, n, cnt, keys, tags = emu_list(members, "held")
    assert rc == 0 and n == len(mt) == int(mc.sum()), (rc, n, len(mt))
    assert np.array_equal(cnt, mc) and np.array_equal(tags, mt) and np.array_equal(keys, mk)
    return mk, mt, mc


QUERIES = [(True, 0, 0), (False, 0, 0), (False, 2, 0), (False, 2, 15)]  # (source, extra, esi_from): what the mixes are asked
