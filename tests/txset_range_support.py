"""Test support for the range mode of a sender set (nrq_txset_count_all / _emit_all / _emit_all_syms): a plain numpy statement of
the packet map -- written from the contract in include/nanorq_hip.h, not derived from the emulation or the library -- the CPU
emulation of the map pass (nanorq_amd/csrc/txset_range_emu.cpp over emit_set_range_body.h), and the tables and call lists the
CPU tier and the GPU tier share."""
import ctypes as C
import itertools

import numpy as np

from nanorq_amd import build as nbuild
from rxset_support import MIX4, MIX360

# an object's three-segment table (class L, class S, a staged last block; Z = 6) beside a sender
OBJ3 = [(0, 11, 2, 0), (0, 10, 3, 2), (0, 10, 1, 5), (4, 10, 2, 6)]
# 64 segments of one block each, K cycling over 10, 11, 26, 100, under 16 keys
SEG64 = [(i // 4, (10, 11, 26, 100)[i % 4], 1, i % 4) for i in range(64)]
TABLES = {"mix4": MIX4, "mix360": MIX360, "obj3": OBJ3, "seg64": SEG64}

# (order, source, rep0, nrep, G): every combination the issue names
CALLS = [(order, source, rep0, nrep, G) for order, source, (rep0, nrep), G in
         itertools.product((0, 1), (0, 1), ((0, 0), (0, 5), (7, 5)), (1, 4, 64))]

_EMU = None


def emu_lib():
    global _EMU
    if _EMU is None:
        L = C.CDLL(nbuild.build_txset_range_emu())
        vp, u32 = C.c_void_p, C.c_uint32
        L.emu_txset_range.argtypes = [u32, vp, vp, u32, vp, vp, vp, vp, vp]
        _EMU = L
    return _EMU


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def blocks_of(mix):
    """(key, SBN, K) of every block in the set's block order: members (key, K, nblk, sbn0) sorted by (key, first SBN), a member's
    blocks in SBN order"""
    out = []
    for key, K, nblk, sbn0 in sorted(mix, key=lambda m: (m[0], m[3])):
        out += [(key, sbn0 + b, K) for b in range(nblk)]
    return out


def cut(K, source, rep0, nrep, G):
    """a block's packet list [(first ESI, count)]: the source run [0, K) cut into packets of G from its start (only with source),
    then the repair run [K + rep0, K + rep0 + nrep) cut the same way"""
    runs = ([(0, K)] if source else []) + [(K + rep0, K + rep0 + nrep)]
    out = []
    for lo, hi in runs:
        e = lo
        while e < hi:
            out.append((e, min(G, hi - e)))
            e += G
    return out


def range_ref(mix, order, source, rep0, nrep, G):
    """the map as numpy arrays -> (keys, first tags, counts, packets per block).  Order 0: block after block; order 1: round j holds
    packet j of every block that has one, in block order -- a stable sort of the block-major list by (j, block)."""
    keys, tags, cnts, g_of, j_of, lens = [], [], [], [], [], []
    for g, (key, sbn, K) in enumerate(blocks_of(mix)):
        pk = cut(K, source, rep0, nrep, G)
        lens.append(len(pk))
        for j, (e, c) in enumerate(pk):
            keys.append(key)
            tags.append((sbn << 24) | e)
            cnts.append(c)
            g_of.append(g)
            j_of.append(j)
    keys, tags, cnts = np.array(keys, np.uint32), np.array(tags, np.uint32), np.array(cnts, np.uint8)
    if order:
        perm = np.lexsort((np.array(g_of, np.int64), np.array(j_of, np.int64)))
        keys, tags, cnts = keys[perm], tags[perm], cnts[perm]
    return keys, tags, cnts, np.array(lens, np.uint32)


def emu_range(mix, order, source, rep0, nrep, G, n):
    """the emulated map pass over the table of `mix` -> (keys, tags, counts, segments, work order), each [n]"""
    rows = sorted(mix, key=lambda m: (m[0], m[3]))
    prm = np.zeros((max(1, len(rows)), 8), np.uint32)
    for i, (key, K, nblk, sbn0) in enumerate(rows):
        prm[i, :6] = (K, 0, 0, nblk, sbn0, key)
    call = np.array([source, rep0, nrep, G, order], np.uint32)
    m = max(1, n)
    keys, tags, seg, worder = (np.full(m, 0xFFFFFFFF, np.uint32) for _ in range(4))
    nsym = np.full(m, 0xFF, np.uint8)
    rc = emu_lib().emu_txset_range(len(rows), _p(prm), _p(call), n, _p(keys), _p(tags), _p(nsym), _p(seg), _p(worder))
    assert rc == 0, rc
    return keys[:n], tags[:n], nsym[:n], seg[:n], worder[:n]


def global_block(mix, keys, tags):
    """the set's global block of every (key, tag) of the map"""
    index = {(key, sbn): g for g, (key, sbn, _) in enumerate(blocks_of(mix))}
    return np.array([index[(int(k), int(t) >> 24)] for k, t in zip(keys, tags)], np.int64)
