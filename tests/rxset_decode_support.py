"""Test support for a reception set's counts, lists and decode (nrq_rxset_blocks / _counts / _lists / _decode): the CPU emulation
of the listing passes (nanorq_amd/csrc/rxset_lists_emu.cpp over lists_set_body.h) on the state arrays of rx_support.EmuRx members,
numpy models written from the header's words, and rxset_plan.h's grouping behind ctypes."""
import ctypes as C

import numpy as np

from nanorq_amd import build as nbuild

_EMU = None
CHUNK = 256  # RXSET_CHUNK_BLOCKS
NONE = 0xFFFFFFFF


def emu_lib():
    global _EMU
    if _EMU is None:
        L = C.CDLL(nbuild.build_rxset_lists_emu())
        vp, u32 = C.c_void_p, C.c_uint32
        L.emu_rxset_lists_words.argtypes = [u32, vp]
        L.emu_rxset_lists_words.restype = C.c_uint64
        L.emu_rxset_lists.argtypes = [u32, vp, vp, vp, vp, vp, vp]
        L.emu_rxset_plan.argtypes = [vp, u32, vp, vp, vp, u32, vp, vp, vp, u32]
        _EMU = L
    return _EMU


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def block_order(members):
    """[(key, member, block in the member)] in the set's block order; members = [(key, rx with .sbn0 / .nblk)]"""
    out = []
    for key, rx in sorted(members, key=lambda m: (m[0], m[1].sbn0)):
        out += [(key, rx, b) for b in range(rx.nblk)]
    return out


def emu_lists(members):
    """The emulated listing passes over [(key, EmuRx, objZ)] in any order -> (keys, sbns, (gaps, nrep) of the counts pass, gaps of
    the lists pass, offsets [nb + 1], list words).  Raises when a guard word behind the buffer was overwritten."""
    nmem = len(members)
    prm = np.array([[e.K, e.T, e.nblk, e.sbn0, e.max_esi, e.rep_cap, k, z] for k, e, z in members], np.uint32).reshape(-1, 8)
    ptr = np.array([[a.ctypes.data for a in (e.src, e.rep, e.first, e.seen, e.gaps, e.nrep, e.rep_esi, e.live)]
                    for _, e, _ in members], np.uint64).reshape(-1, 8)
    nb = sum(e.nblk for _, e, _ in members)
    words = int(emu_lib().emu_rxset_lists_words(nmem, _p(prm)))
    assert words == 1 + sum(e.nblk * (e.K + e.rep_cap + 2) for _, e, _ in members)
    keys, sbns, counts = np.zeros(nb, np.uint32), np.zeros(nb, np.uint32), np.zeros(2 * nb, np.uint32)
    buf = np.zeros(words, np.uint32)
    rc = emu_lib().emu_rxset_lists(nmem, _p(prm), _p(ptr), _p(keys), _p(sbns), _p(counts), _p(buf))
    assert rc != -3, "a listing pass wrote behind the list buffer"
    assert rc == nb, rc
    off = buf[nb:2 * nb + 1].copy()
    return keys, sbns, (counts[:nb].copy(), counts[nb:].copy()), buf[:nb].copy(), off, buf[2 * nb + 1:2 * nb + 1 + int(off[nb])].copy()


def model_block_list(e, b):
    """a block's list from the header's words: rep_esi[b][:nrep], then the ESIs < K whose seen bit is clear, ascending"""
    rep = e.rep_esi[b * e.rep_cap:b * e.rep_cap + int(e.nrep[b])]
    w = e.seen[b * e.bm_words:(b + 1) * e.bm_words]
    bits = np.unpackbits(w.view(np.uint8), bitorder="little")[:e.K]
    return np.concatenate([rep, np.flatnonzero(bits == 0)]).astype(np.uint32)


def selected(ng, nr, K, max_esi):
    """the three clauses of nrq_rx_decode's rule, in numpy (int64: no wrap)"""
    ng, nr, K, max_esi = (np.asarray(a, np.int64) for a in (ng, nr, K, max_esi))
    return (ng != 0) & (nr >= ng) & (nr - ng <= max_esi - K)


def plan(mem, member, ng, nr):
    """rxset_plan(): mem [nmem][4] = (K, K', max_esi, has_relay).  -> (chunk_of [nb], pos_of [nb], chunks [n][4] = (K, K', has_relay, blocks))"""
    mem = np.ascontiguousarray(mem, np.uint32).reshape(-1, 4)
    member, ng, nr = (np.ascontiguousarray(a, np.uint32) for a in (member, ng, nr))
    nb = len(member)
    chunk_of, pos_of = np.zeros(max(nb, 1), np.uint32), np.zeros(max(nb, 1), np.uint32)
    cp = np.zeros((max(nb, 1), 4), np.uint32)
    n = emu_lib().emu_rxset_plan(_p(mem), len(mem), _p(member), _p(ng), _p(nr), nb, _p(chunk_of), _p(pos_of), _p(cp), len(cp))
    assert n >= 0, n
    return chunk_of[:nb], pos_of[:nb], cp[:n]


def predicted_chunks(groups):
    """decode calls for {group: selected blocks}"""
    return sum((n + CHUNK - 1) // CHUNK for n in groups.values())
