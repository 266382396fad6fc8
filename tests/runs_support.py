"""Test support for the want and held listings as runs (nrq_rx_want_syms / nrq_rx_held_syms) and the held emit of packets of several
symbols (NRQ_TX_HELD in nrq_tx_emit_syms): the reference model -- the packetisation of include/nanorq_hip.h in ten lines of Python,
applied to the one-symbol lists of want_support.model_want / held_support.host_held -- and the CPU emulation
(nanorq_amd/csrc/runs_emu.cpp over runs_body.h) over the emulated receptions of rx_support.EmuRx."""
import ctypes as C

import numpy as np

import nanorq_amd
import syms_support as S
from nanorq_amd import build as nbuild
from relay_support import mask_words
from rx_support import EmuRx, ModelRx, payloads_for, tag
from tx_support import FILL, _p

ESI = 0xFFFFFF
GS = (1, 2, 5, 16, 64)
GUARD = 0xDEADBEEF
GUARD_B = 0xA5
POISON_WORDS = 64

_EMU = None


def emu_lib():
    global _EMU
    if _EMU is None:
        L = C.CDLL(nbuild.build_runs_emu())
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        L.emu_rx_want_syms.argtypes = [vp, vp, vp, vp, u32, u32, u32, u32, vp, vp, u32, vp, vp]
        L.emu_rx_held_syms.argtypes = [vp, vp, vp, vp, u32, vp, vp, u32, vp, vp]
        L.emu_emit_held_syms.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, u32, u32, u32, vp, u64, vp]
        _EMU = L
    return _EMU


def packetise(L, G, K_of):
    """The packetisation of a one-symbol listing L at G -> (first tags uint32 [n], counts uint8 [n]).  K_of(sbn) -> the K of that
    block: a run is a maximal stretch of consecutive tags (one block, consecutive ESIs in list order) that lies on one side of K;
    every run is cut into packets of G from its start, the last one short."""
    L = [int(t) for t in L]
    tags, cnt, i = [], [], 0
    while i < len(L):
        j, K = i, K_of(L[i] >> 24)
        while j + 1 < len(L) and L[j + 1] == L[j] + 1 and L[j + 1] >> 24 == L[i] >> 24 and ((L[j] & ESI) < K) == ((L[j + 1] & ESI) < K):
            j += 1
        for s in range(i, j + 1, G):
            tags.append(L[s])
            cnt.append(min(G, j + 1 - s))
        i = j + 1
    return np.array(tags, np.uint32), np.array(cnt, np.uint8)


def expanded(tags, nsym, G):
    """the one-symbol tag list a packet list stands for (syms_support.expansion, as tags)"""
    _, sbn, esi = S.expansion(tags, [int(c) for c in nsym], G)
    return ((sbn << 24) | esi).astype(np.uint32)


def _outputs(cap):
    return np.full(cap + 4, GUARD, np.uint32), np.full(cap + 16, GUARD_B, np.uint8)


def _listing(call, cap, count_only, only=None):
    """the two-step use of a listing: the counts (NULL outputs), then the packets into buffers with guards behind them
    -> (rc, npkt, nsym, tags [cap], counts [cap])"""
    npkt, nsym = C.c_uint32(0), C.c_uint32(0)
    rc = call(None, None, 0, C.byref(npkt), C.byref(nsym))
    if count_only or rc != 0:
        return rc, npkt.value, nsym.value, np.zeros(0, np.uint32), np.zeros(0, np.uint8)
    if cap is None:
        cap = npkt.value
    tg, ns = _outputs(cap)
    n2, s2 = C.c_uint32(0), C.c_uint32(0)
    rc = call(None if only == "nsym" else _p(tg), None if only == "tags" else _p(ns), cap, C.byref(n2), C.byref(s2))
    assert (tg[cap:] == GUARD).all() and (ns[cap:] == GUARD_B).all(), "guards behind the outputs"
    if rc == 0 or only is None:
        assert (n2.value, s2.value) == (npkt.value, nsym.value)
    return rc, n2.value, s2.value, tg[:cap], ns[:cap]


def emu_want_syms(rx, G, flags=0, extra=0, esi_from=0, cap=None, count_only=False, only=None):
    """the want listing in packets of one emulated reception; POISON_WORDS zero words lie behind the bitmap (a read past it shows
    as a wanted ESI), guard words and bytes behind both outputs"""
    prm = np.array([rx.K, rx.nblk, rx.sbn0, rx.max_esi, rx.rep_cap], np.uint32)
    seen = np.concatenate([rx.seen, np.zeros(POISON_WORDS, np.uint32)])

    def call(tg, ns, cap, npkt, nsym):
        return emu_lib().emu_rx_want_syms(_p(prm), _p(seen), _p(rx.gaps), _p(rx.nrep), flags, extra, esi_from, G, tg, ns, cap, npkt, nsym)
    return _listing(call, cap, count_only, only)


def emu_held_syms(rx, G, cap=None, count_only=False, only=None):
    """the held listing in packets of one emulated reception; POISON_WORDS words of all ones lie behind the bitmap (a read past it
    shows as a held ESI)"""
    prm = np.array([rx.K, rx.nblk, rx.sbn0, rx.max_esi, rx.rep_cap], np.uint32)
    seen = np.concatenate([rx.seen, np.full(POISON_WORDS, 0xFFFFFFFF, np.uint32)])

    def call(tg, ns, cap, npkt, nsym):
        return emu_lib().emu_rx_held_syms(_p(prm), _p(seen), _p(rx.nrep), _p(rx.rep_esi), G, tg, ns, cap, npkt, nsym)
    return _listing(call, cap, count_only, only)


def emu_emit_held_syms(rxs, Kps, inters, span, ready, tags, nsym, G, inline, stride):
    """The held emit of packets of up to G symbols over a relay's table, as held_support.emu_emit_held: segment g reads the emulated
    reception rxs[g] and the intermediate symbols inters[g]; nsym None: the sender's rule -> (packets [n, stride], results [n])"""
    nseg, T = len(rxs), rxs[0].T
    prm = np.array([[r.K, Kp, T, r.nblk, r.sbn0] for r, Kp in zip(rxs, Kps)], np.uint32)
    srcs = [np.ascontiguousarray(r.src.reshape(r.nblk, -1)) for r in rxs]
    inters = [np.ascontiguousarray(a, np.uint8) for a in inters]
    seens = [np.concatenate([r.seen, np.full(POISON_WORDS, 0xFFFFFFFF, np.uint32)]) for r in rxs]
    reps = [np.ascontiguousarray(r.rep.reshape(r.nblk, -1)) for r in rxs]

    def per_seg(ctype, vals):
        return (ctype * nseg)(*vals)
    tags = np.ascontiguousarray(tags, np.uint32)
    ns = None if nsym is None else np.ascontiguousarray(nsym, np.uint8)
    n = len(tags)
    res = np.full(n, 77, np.int32)
    pkts = np.full((n, stride), FILL, np.uint8)
    rc = emu_lib().emu_emit_held_syms(
        _p(prm), nseg, _p(np.array(span, np.uint32)),
        per_seg(C.c_void_p, [a.ctypes.data for a in srcs]), per_seg(C.c_uint64, [a.shape[1] for a in srcs]),
        per_seg(C.c_void_p, [a.ctypes.data for a in inters]), per_seg(C.c_uint64, [a.shape[1] * T for a in inters]),
        _p(mask_words(ready)),
        per_seg(C.c_void_p, [a.ctypes.data for a in seens]), per_seg(C.c_uint32, [r.bm_words for r in rxs]),
        per_seg(C.c_void_p, [r.rep_esi.ctypes.data for r in rxs]), per_seg(C.c_void_p, [r.nrep.ctypes.data for r in rxs]),
        per_seg(C.c_uint32, [r.rep_cap for r in rxs]),
        per_seg(C.c_void_p, [a.ctypes.data for a in reps]), per_seg(C.c_uint64, [a.shape[1] for a in reps]),
        _p(tags), _p(ns), n, G, int(inline), _p(pkts), stride, _p(res))
    assert rc == 0, rc
    return pkts, res


# ---- the reception whose repair runs cross a round of rows ----
R600 = dict(K=10, T=16, nblk=3, rep_cap=600, sbn0=2)


def r600_stream():
    """Block 0: repair ESIs 10 .. 539 arriving ascending (one run over 530 rows: it crosses row 256, and 256 % 5 = 1); block 1: the
    same ESIs descending (530 runs of one); block 2: source ESIs 0 .. 8 and repair ESI 10, then 11, 12 (nothing joins K - 1 to K:
    there is no symbol 9)"""
    s0 = R600["sbn0"]
    return np.array([tag(s0, e) for e in range(10, 540)] + [tag(s0 + 1, e) for e in range(539, 9, -1)] +
                    [tag(s0 + 2, e) for e in range(9)] + [tag(s0 + 2, e) for e in (10, 11, 12)], np.uint32)


def r600_filled():
    """-> (EmuRx, ModelRx) after the stream, in two calls"""
    p = R600
    Kp = nanorq_amd.params(p["K"])["Kp"]
    emu = EmuRx(p["K"], p["T"], p["nblk"], p["rep_cap"], sbn0=p["sbn0"], max_esi=1000, Kp=Kp)
    mod = ModelRx(p["K"], p["T"], p["nblk"], p["rep_cap"], sbn0=p["sbn0"], max_esi=1000, Kp=Kp)
    for part in np.array_split(r600_stream(), 2):
        pay = payloads_for(part, p["T"])
        assert np.array_equal(emu.add(pay, tags=part), mod.add(pay, part))
    return emu, mod


def model_held(mod):
    """held_support.host_held of a rx_support.ModelRx"""
    from held_support import host_held
    return host_held(mod.sbn0, mod.K, [[e in mod.seen[b] for e in range(mod.K)] for b in range(mod.nblk)], mod.reps)


# ---- the relay in three states and the packet list of the held emit tests (CPU tier and GPU tier) ----
HI = (1 << 24) - 1
FOREIGN, NOT_READY, BAD_RANGE = -1, -2, -3
K3, NB3, S3, MAXE3 = 100, 3, 9, 1000
LOST3 = [[1, 17, 60, 99], [0, 5, 44], [2, 3, 70, 71, 72]]


def mixed_stream(G):
    """what the three blocks receive, in arrival order (block 0 becomes ready, block 1 complete but not ready, block 2 stays
    partial): per block the source ESIs it keeps, then its repair ESIs.  Block 2's repair arrivals: a run in arrival order, a run of
    consecutive ESIs arriving DESCENDING, and three stretches of G ESIs with the first, a middle and the last one missing."""
    K = K3
    asc = list(range(K + 5, K + 5 + G + 3))
    desc = list(range(K + 80 + G - 1, K + 80 - 1, -1))
    holes = [e for base, hole in ((K + 300, 0), (K + 400, G // 2), (K + 500, G - 1)) for e in range(base, base + G) if e != base + hole]
    reps = [[K + 3, K + 40, K + 9, K + 1, K + 77, K + 6], [K + 12, K + 13, K + 2, K + 31, K + 8], asc + desc + holes]
    return [[e for e in range(K) if e not in LOST3[b]] + reps[b] for b in range(NB3)]


def mixed_packets(G):
    """(first tag, count or None for the sender's rule) over the three blocks: every row of the table of include/nanorq_hip.h"""
    K, t = K3, lambda b, e: tag(S3 + b, e)
    c2 = min(2, G)
    pk = [(t(2, 4), G), (t(2, 4), None), (t(2, K + 5), G), (t(2, K + 6), c2), (t(2, K + 5 + G), 3), (t(2, K + 80), G), (t(2, K + 81), G - 1),  # held
          (t(2, 3), c2), (t(2, 69), 2), (t(2, K + 300), G), (t(2, K + 400), G), (t(2, K + 500), G), (t(2, K + 9), G),
          (t(2, K + 4), 2), (t(2, K + 700), 1),                                                                 # a symbol missing
          (t(1, 0), G), (t(1, 0), None), (t(1, K - c2), c2), (t(1, K - 1), None), (t(1, K + 12), 2), (t(1, K + 2), 2), (t(1, K + 13), 1),
          (t(0, 0), G), (t(0, K - 3), None), (t(0, K + 7), G), (t(0, K + 7), None),                             # the ready block
          (t(3, 1), 1), (tag(S3 - 1, 1), 1),                                                                    # foreign SBNs
          (t(0, 5), 0), (t(0, 5), G + 1), (t(0, K - 1), 2), (t(0, HI), 2),                                      # BAD_RANGE, ready
          (t(2, 5), 0), (t(2, 5), G + 1), (t(2, K - 1), 2), (t(2, HI), 2), (t(1, K - 1), 2)]                    # BAD_RANGE, not ready
    return [(a, c) for a, c in pk if c is None or c <= 255]


def table(tags, counts, G, held_of, ready):
    """the result of every packet by the table of include/nanorq_hip.h; held_of(b) -> the set of ESIs block b holds"""
    out = []
    for tg, c in zip(tags, counts):
        b, e = (int(tg) >> 24) - S3, int(tg) & HI
        if not 0 <= b < NB3:
            out.append(FOREIGN)
        elif c == 0 or c > G or (e < K3 and e + c > K3) or e + c - 1 > HI:
            out.append(BAD_RANGE)
        elif ready[b] or all(e + i in held_of(b) for i in range(c)):
            out.append(0)
        else:
            out.append(NOT_READY)
    return np.array(out, np.int32)


def from_one_symbol(one, tags, counts, res, G, T, inline, stride):
    """the packets a list must give, laid out from the one-symbol packets `one` ([m, T]) of the expansion of its written packets"""
    hdr = 4 if inline else 0
    want = np.full((len(tags), stride), FILL, np.uint8)
    q = 0
    for k, (tg, c) in enumerate(zip(tags, counts)):
        if res[k] != 0:
            continue
        if inline:
            want[k, :4] = np.frombuffer(int(tg).to_bytes(4, "big"), np.uint8)
        want[k, hdr:hdr + c * T] = one[q:q + c].reshape(-1)
        q += c
    assert q == len(one)
    return want


def counts_of(packets, G):
    return [S.rule(K3, int(a) & HI, G) if c is None else c for a, c in packets]
