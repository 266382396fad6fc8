"""Test support for a reception set's want and held listings as runs (nrq_rxset_want_syms / nrq_rxset_held_syms) and a sender
set's held emit of packets of several symbols (NRQ_TX_HELD in nrq_txset_emit_syms): the CPU emulation
(nanorq_amd/csrc/rxset_runs_emu.cpp over runs_set_body.h) on the state arrays of rx_support.EmuRx members and txset_support.Seg
segments, the reference -- runs_support.packetise of the one-symbol set listing with each block's own member's K -- and the mixed
member table both tiers emit from."""
import ctypes as C

import numpy as np

import nanorq_amd
import runs_support as U
import txset_support as XS
from nanorq_amd import build as nbuild
from rx_support import EmuRx, ModelRx, payloads_for, tag
from rxset_decode_support import block_order
from tx_support import FILL

GUARD, GUARD_B, NGUARD, NGUARD_B = U.GUARD, U.GUARD_B, 4, 16
POISON_WORDS = U.POISON_WORDS
HI = U.HI
FOREIGN, NOT_READY, BAD_RANGE = U.FOREIGN, U.NOT_READY, U.BAD_RANGE

_EMU = None


def emu_lib():
    global _EMU
    if _EMU is None:
        L = C.CDLL(nbuild.build_rxset_runs_emu())
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        L.emu_rxset_want_syms.argtypes = [u32, vp, vp, u32, u32, u32, u32, vp, vp, vp, u32, vp, vp, vp]
        L.emu_rxset_held_syms.argtypes = [u32, vp, vp, u32, vp, vp, vp, u32, vp, vp, vp]
        L.emu_txset_emit_held_syms.argtypes = [u32, vp, vp, vp, vp, vp, vp, u32, u32, u32, vp, u64, vp, vp]
        _EMU = L
    return _EMU


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _table(members, poison):
    """(prm, ptr, keep): the members [(key, EmuRx, objZ)] as emu_rxset_add describes them, every seen bitmap a copy with
    POISON_WORDS words of `poison` behind it (zeros show a read past the bitmap as a wanted ESI, ones as a held one)"""
    prm = np.array([[e.K, e.T, e.nblk, e.sbn0, e.max_esi, e.rep_cap, k, z] for k, e, z in members], np.uint32).reshape(-1, 8)
    keep = [np.concatenate([e.seen, np.full(POISON_WORDS, poison, np.uint32)]) for _, e, _ in members]
    ptr = np.array([[a.ctypes.data for a in (e.src, e.rep, e.first, s, e.gaps, e.nrep, e.rep_esi, e.live)]
                    for (_, e, _), s in zip(members, keep)], np.uint64).reshape(-1, 8)
    return prm, ptr, keep


class Listing:
    """what one emulated call left: rc, npkt, nsym, cnt [nb], keys / tags / ns [cap] (None where not given)"""

    def __init__(self, rc, npkt, nsym, cnt, keys, tags, ns):
        self.rc, self.npkt, self.nsym, self.cnt, self.keys, self.tags, self.ns = rc, npkt, nsym, cnt, keys, tags, ns


def emu_list_syms(members, what, G, flags=0, extra=0, esi_from=0, cap=None, count_only=False, with_keys=True, give=("tags", "nsym"),
                  no_npkt=False):
    """The emulated listing in packets (`what`: "want" / "held") over [(key, EmuRx, objZ)] in any order -> Listing.  cap None:
    exactly the packet total (asked for first, with NULL lists).  Guard words and bytes lie behind the keys, the tags, the counts
    and the per-block counts; asserts that they are intact and that the count call and the fill call agree.  give: which of the
    two lists the fill call is handed (both, or one: refused); no_npkt: the packet total's pointer is NULL (refused)."""
    prm, ptr, keep = _table(members, 0 if what == "want" else 0xFFFFFFFF)
    nmem, nb = len(members), sum(e.nblk for _, e, _ in members)
    L = emu_lib()

    def call(keys, tags, ns, cap, cnt, npkt, nsym):
        np_ = None if no_npkt else C.byref(npkt)
        if what == "want":
            return L.emu_rxset_want_syms(nmem, _p(prm), _p(ptr), flags, extra, esi_from, G, _p(keys), _p(tags), _p(ns), cap, _p(cnt), np_, C.byref(nsym))
        return L.emu_rxset_held_syms(nmem, _p(prm), _p(ptr), G, _p(keys), _p(tags), _p(ns), cap, _p(cnt), np_, C.byref(nsym))

    npkt, nsym = C.c_uint32(0xFFFFFFFF), C.c_uint32(0xFFFFFFFF)
    cnt = np.full(nb + NGUARD, GUARD, np.uint32)
    rc = call(None, None, None, 0, cnt, npkt, nsym)
    assert rc not in (-2, -3, -4), rc
    assert (cnt[nb:] == GUARD).all(), "guard words behind the per-block counts"
    if rc != 0 or count_only:
        return Listing(rc, npkt.value, nsym.value, cnt[:nb].copy(), None, None, None)
    if cap is None:
        cap = npkt.value
    tags = np.full(cap + NGUARD, GUARD, np.uint32)
    keys = np.full(cap + NGUARD, GUARD, np.uint32)
    ns = np.full(cap + NGUARD_B, GUARD_B, np.uint8)
    cnt2 = np.full(nb + NGUARD, GUARD, np.uint32)
    n2, s2 = C.c_uint32(0xFFFFFFFF), C.c_uint32(0xFFFFFFFF)
    rc = call(keys if with_keys else None, tags if "tags" in give else None, ns if "nsym" in give else None, cap, cnt2, n2, s2)
    assert rc not in (-2, -3, -4), rc
    assert (tags[cap:] == GUARD).all() and (keys[cap:] == GUARD).all() and (ns[cap:] == GUARD_B).all() and (cnt2[nb:] == GUARD).all(), "guards"
    if not with_keys:
        assert (keys == GUARD).all()
    if len(give) == 2:
        assert (n2.value, s2.value) == (npkt.value, nsym.value) and np.array_equal(cnt2[:nb], cnt[:nb])
    poison = 0 if what == "want" else 0xFFFFFFFF
    assert all((s[-POISON_WORDS:] == poison).all() for s in keep)
    return Listing(rc, n2.value, s2.value, cnt2[:nb].copy(), keys[:cap] if with_keys else None, tags[:cap], ns[:cap])


# ------------------------------------------------------------------------------------- the reference: the header's words ----
def reference(members, one_keys, one_tags, one_cnt, G):
    """the packetisation of a one-symbol set listing (keys, tags, tags per block, in block order) with each block's own member's K
    -> (keys [n], first tags [n], counts [n], packets per block [nb])"""
    ks, ts, ns, cnt = [np.zeros(0, np.uint32)], [np.zeros(0, np.uint32)], [np.zeros(0, np.uint8)], []
    at = 0
    for (key, e, b), c in zip(block_order([(k, e) for k, e, _ in members]), one_cnt):
        c = int(c)
        assert (one_keys[at:at + c] == key).all() and ((one_tags[at:at + c] >> 24) == e.sbn0 + b).all()
        t, n = U.packetise(one_tags[at:at + c], G, lambda sbn, K=e.K: K)
        ts.append(t)
        ns.append(n)
        ks.append(np.full(len(t), key, np.uint32))
        cnt.append(len(t))
        at += c
    assert at == len(one_tags)
    return np.concatenate(ks), np.concatenate(ts), np.concatenate(ns), np.array(cnt, np.uint32)


def check_listing(got, ref, L, G):
    """a listing (keys, tags, counts, per-block counts, npkt, nsym) equals the reference of the one-symbol list L, word for word"""
    keys, tags, ns, cnt, npkt, nsym = got
    rk, rt, rn, rc = ref
    assert npkt == len(rt) == int(np.sum(cnt)) and nsym == len(L), (npkt, len(rt), nsym, len(L))
    assert np.array_equal(cnt, rc)
    assert np.array_equal(tags, rt) and np.array_equal(ns, rn) and np.array_equal(keys, rk)
    assert np.array_equal(U.expanded(tags, ns, G), L)
    if G == 1:
        assert np.array_equal(tags, L) and (ns == 1).all()


# ------------------------------------------------------------------------------------------------ the held set emit ----
def emu_txset_emit_held_syms(segs, keys, tags, nsym, G, hdr, stride):
    """The emulated set emit with NRQ_TX_HELD of packets of several symbols over txset_support.Seg segments (rx: the emulated
    reception a relay's segment reads; a read past its bitmap shows as "held") -> (packets [n, stride], results [n], order [n])."""
    segs = XS.table_order(segs)
    tags = np.ascontiguousarray(tags, np.uint32)
    ks = None if keys is None else np.ascontiguousarray(keys, np.uint32)
    ns = None if nsym is None else np.ascontiguousarray(nsym, np.uint8)
    n = len(tags)
    prm = np.zeros((max(1, len(segs)), 8), np.uint32)
    ptr = np.zeros((max(1, len(segs)), 9), np.uint64)
    keep, bits = [], []
    for g, s in enumerate(segs):
        prm[g, :6] = (s.K, s.Kp, s.T, s.nblk, s.sbn0, s.key)
        ptr[g, :4] = (s.src.ctypes.data, s.src.shape[1], s.inter.ctypes.data, s.inter.shape[1] * s.T)
        if s.rx is not None:
            r = s.rx
            seen = np.concatenate([r.seen, np.full(POISON_WORDS, 0xFFFFFFFF, np.uint32)])
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
    rc = emu_lib().emu_txset_emit_held_syms(len(segs), _p(prm), _p(ptr), _p(ready), _p(ks), _p(tags), _p(ns), n, G, hdr, _p(pkts), stride,
                                            _p(res), _p(order))
    assert rc == 0, rc
    return pkts, res, order[:n]


# The mixed member table: the relay of runs_support (K3 = 100, three blocks from SBN S3: ready / complete but not ready / partial)
# under KEY_R, a plain sender under KEY_S and an object's relay of two block classes under KEY_O.
KEY_R, KEY_S, KEY_O, KEY_NONE = 0x52, 7, 0x1001, XS.UNKNOWN_KEY
KS, NBS, SBNS = 26, 2, U.S3          # the sender: the relay's first SBNs under another key
KOL, KOS, ZL, ZS = 31, 30, 1, 2      # the object: one block of K = 31, two of K = 30
FAR = 64 + 9                         # block 2's repair rows in front of its runs: the runs lie beyond row 64 of the list
REP_CAP3 = 5 * 64 + 8 + FAR          # (runs_support's mixed stream at G = 64 books 320 repair rows)


def far_stream(G):
    """runs_support.mixed_stream with FAR single repair symbols (ESIs K3 + 600, + 602, ...: no two consecutive) arriving at block
    2 in front of its other repair symbols, so that every held repair packet's rows lie beyond the first trip of 64"""
    st = U.mixed_stream(G)
    src, rep = [e for e in st[2] if e < U.K3], [e for e in st[2] if e >= U.K3]
    return [st[0], st[1], src + [U.K3 + 600 + 2 * i for i in range(FAR)] + rep]


class Mixed:
    """the member table at symbol size T and packet size G: segs (txset_support.Seg, table order), the emulated receptions and
    their models, and for each segment what its blocks hold"""

    def __init__(self, T, G, seed=0, relay=None, sender=None):
        """relay (emu, mod, inter) and sender (src, inter): these two members as a device holds them (the GPU tier, where blocks
        0 and 1 are decoded and their rows are therefore real symbols of far_stream(G)); None: made here over arbitrary rows"""
        rng = np.random.default_rng(1000 * T + G + seed)
        self.T, self.G = T, G
        p = nanorq_amd.params
        Kp = p(U.K3)["Kp"]
        self.streams, self.obj_streams = [], []
        if relay is None:
            self.emu = EmuRx(U.K3, T, U.NB3, REP_CAP3, sbn0=U.S3, max_esi=U.MAXE3, Kp=Kp)
            self.mod = ModelRx(U.K3, T, U.NB3, REP_CAP3, sbn0=U.S3, max_esi=U.MAXE3, Kp=Kp)
            for b, es in enumerate(far_stream(G)):
                tg = np.array([tag(U.S3 + b, e) for e in es], np.uint32)
                pay = payloads_for(tg, T, salt=G)
                self.streams.append((np.full(len(tg), KEY_R, np.uint32), tg, pay))
                assert np.array_equal(self.emu.add(pay, tags=tg), self.mod.add(pay, tg))
            self.fixed = [rng.integers(0, 256, (len(U.LOST3[b]), T), dtype=np.uint8) for b in (0, 1)]
            for b in (0, 1):  # decoded: the lost rows recovered
                self.emu.src[b, U.LOST3[b]] = self.fixed[b]
                self.emu.mark_complete(b)
                self.mod.mark_complete(b)
            self.inter = rng.integers(0, 256, (U.NB3, p(Kp)["L"], T), dtype=np.uint8)
        else:
            self.emu, self.mod, self.inter = relay
        relay = XS.Seg(KEY_R, U.K3, Kp, T, U.S3, self.emu.src, self.inter, rx=self.emu, ready=[True, False, False])
        KpS = p(KS)["Kp"]
        if sender is None:
            sender = (rng.integers(0, 256, (NBS, KS, T), dtype=np.uint8), rng.integers(0, 256, (NBS, p(KpS)["L"], T), dtype=np.uint8))
        sender = XS.Seg(KEY_S, KS, KpS, T, SBNS, *sender)
        # the object's relay: class L (SBN 0) partial, class S (SBNs 1, 2) partial and untouched
        self.obj = []
        osegs = []
        for K, nblk, sbn0, lost, reps in ((KOL, ZL, 0, [[3, 4, 30]], [[KOL + 1, KOL + 2, KOL + 3, KOL + 9]]),
                                          (KOS, ZS, ZL, [[0, 29], list(range(KOS))], [[KOS + 5, KOS + 4], []])):
            KpO = p(K)["Kp"]
            e = EmuRx(K, T, nblk, 12, sbn0=sbn0, max_esi=2 * p(KOL)["Kp"], Kp=KpO)
            m = ModelRx(K, T, nblk, 12, sbn0=sbn0, max_esi=2 * p(KOL)["Kp"], Kp=KpO)
            for b in range(nblk):
                tg = np.array([tag(sbn0 + b, x) for x in [x for x in range(K) if x not in lost[b]] + reps[b]], np.uint32)
                if len(tg):
                    pay = payloads_for(tg, T, salt=G + 1)
                    self.streams.append((np.full(len(tg), KEY_O, np.uint32), tg, pay))
                    self.obj_streams.append((tg, pay))
                    assert np.array_equal(e.add(pay, tags=tg), m.add(pay, tg))
            self.obj.append((e, m))
            osegs.append(XS.Seg(KEY_O, K, KpO, T, sbn0, e.src, rng.integers(0, 256, (nblk, p(KpO)["L"], T), dtype=np.uint8), rx=e,
                                ready=[False] * nblk))
        self.segs = XS.table_order([relay, sender] + osegs)
        self.relay, self.sender, self.osegs = relay, sender, osegs

    def packets(self):
        """(keys, first tags, counts) interleaved over the members so that one wave holds packets of several segments: the relay's
        runs_support.mixed_packets (every row of the header's table), the same first tags under the sender's key and under an
        unknown key, and the object's held lists with a packet across each class's K and one of an SBN >= Z"""
        G = self.G
        mp = U.mixed_packets(G)
        rel = [(KEY_R, a, c) for a, c in zip([a for a, _ in mp], U.counts_of(mp, G))]
        c2 = min(2, G)
        snd = [(KEY_S, tag(SBNS, 0), min(G, KS)), (KEY_S, tag(SBNS + 1, KS - c2), c2), (KEY_S, tag(SBNS + 1, KS + 3), G), (KEY_S, tag(SBNS, KS - 1), 2),
               (KEY_S, tag(SBNS, 5), 0), (KEY_S, tag(SBNS + NBS, 1), 1), (KEY_S, tag(SBNS, HI), 2), (KEY_S, tag(SBNS + 1, 2), 1)]
        obj = []
        for e, _ in self.obj:
            _, _, _, tg, ns = U.emu_held_syms(e, G)
            obj += [(KEY_O, int(a), int(c)) for a, c in zip(tg, ns)]
        obj += [(KEY_O, tag(0, KOL - 1), 2), (KEY_O, tag(1, KOS - 1), 2), (KEY_O, tag(0, 3), 1), (KEY_O, tag(2, 0), min(G, KOS)), (KEY_O, tag(ZL + ZS, 0), 1),
                (KEY_O, tag(0, KOL + 2), min(G, 3)), (KEY_O, tag(1, KOS + 4), c2), (KEY_O, tag(0, 0), c2)]
        none = [(KEY_NONE, tag(U.S3, 1), 1), (KEY_NONE, tag(U.S3 + 2, 4), G)]
        out, rows = [], [rel, snd, obj, none]
        while any(rows):
            for r in rows:
                if r:
                    out.append(r.pop(0))
        return (np.array([k for k, _, _ in out], np.uint32), np.array([a for _, a, _ in out], np.uint32), np.array([c for _, _, c in out], np.uint8))

    def results(self, keys, tags, counts):
        """the result of every packet by the table of include/nanorq_hip.h, member by member (runs_support.table for the relay)"""
        G = self.G
        out = np.full(len(tags), FOREIGN, np.int32)
        rel = np.flatnonzero(keys == KEY_R)
        out[rel] = U.table(tags[rel], [int(c) for c in counts[rel]], G, lambda b: self.mod.seen[b], [True, False, False])
        for k in np.flatnonzero((keys == KEY_S) | (keys == KEY_O)):
            sbn, e, c = int(tags[k]) >> 24, int(tags[k]) & HI, int(counts[k])
            if keys[k] == KEY_S:
                if not SBNS <= sbn < SBNS + NBS:
                    continue
                K, held, ready = KS, set(), True
            else:
                if sbn >= ZL + ZS:
                    continue
                (em, mod), b = (self.obj[0], sbn) if sbn < ZL else (self.obj[1], sbn - ZL)
                K, held, ready = em.K, mod.seen[b], False
            if c == 0 or c > G or (e < K and e + c > K) or e + c - 1 > HI:
                out[k] = BAD_RANGE
            elif ready or all(e + i in held for i in range(c)):
                out[k] = 0
            else:
                out[k] = NOT_READY
        return out

    def expected(self, keys, tags, counts, res, hdr, stride):
        """the packets a list must give: runs_support.from_one_symbol of the one-symbol held set emit's packets of the expansion of
        its written packets, the key word in front when it is inline"""
        G, T = self.G, self.T
        ok = res == 0
        one_tags = U.expanded(tags[ok], counts[ok], G)
        one_keys = np.repeat(keys[ok], counts[ok].astype(np.int64))
        one, one_res, _ = XS.emu_txset_emit(self.segs, one_keys, one_tags, 0, T, held=True)
        assert (one_res == 0).all()
        body = U.from_one_symbol(one, tags, [int(c) for c in counts], res, G, T, hdr > 0, stride - (4 if hdr == 8 else 0))
        if hdr != 8:
            return body
        want = np.full((len(tags), stride), FILL, np.uint8)
        want[:, 4:] = body
        want[ok, :4] = XS.be32(keys[ok])
        return want


# the five payload paths of sys_emit_path as (T, hdr, stride kind): 16-byte aligned with hdr 0 / 4 / 8, a stride that is a multiple
# of 4 only, an odd T
PATH_ROWS = [(16, 0, "r16", "TX_V16"), (16, 4, "r16", "TX_V16_SHIFT"), (16, 8, "r16", "TXS_V16_KEY"), (16, 4, "pad4", "TX_DWORD"), (5, 8, "tight", "TX_BYTE")]


def stride_of(T, G, hdr, kind):
    s = G * T + hdr
    return {"tight": s, "pad4": (s + 3) // 4 * 4 + 4, "r16": (s + 15) // 16 * 16}[kind]


# ---------------------------------------------------------- the loop of the GPU tier: its members, losses and seed ----
LOOP = [(0x21, 10, 4, 0), (0x21, 32, 3, 4), (5, 100, 3, 0), (0x7000, 257, 2, 1)]  # (key, K, nblk, sbn0): members of different K
LOOP_LOSS = (0.25, 0.2, 0.15, 0.1)
LOOP_SEED = 1  # chosen on the CPU: oracle_rounds(LOOP_SEED) == 1 -- the host planner solves every block of these losses from
#                exactly its gaps' worth of repair symbols K .. K + g - 1, so the bound of 3 rounds holds by the reference alone
#                (asserted in test_rxset_runs_emu.py)


def loop_losses(seed):
    """the source ESIs every block of LOOP loses: {(member, block): sorted list}"""
    rng = np.random.default_rng(seed)
    return {(m, b): np.flatnonzero(rng.random(K) < LOOP_LOSS[m]).tolist() for m, (_, K, nblk, _) in enumerate(LOOP) for b in range(nblk)}


def oracle_rounds(seed):
    """Rounds the loop needs by the host planner alone: round j asks with extra = j - 1, so a block with g gaps has received the
    repair ESIs K .. K + g + j - 2 (nrq_rx_want's list: the lowest unseen ones) when round j decodes; solvable iff the plan's
    status is 0."""
    from emu_support import decode_setup
    from forced_inact_support import header

    class P:
        params = staticmethod(nanorq_amd.params)
    worst = 1
    for (m, b), lost in loop_losses(seed).items():
        K = LOOP[m][1]
        if not lost:
            continue
        for j in range(1, 9):
            isis, _ = decode_setup(P, K, lost, np.arange(K, K + len(lost) + j - 1))
            if header(K, isis)["status"] == 0:
                break
        worst = max(worst, j)
    return worst
