"""Test support for the sets' packets of several symbols (nrq_rxset_add_syms, nrq_txset_emit_syms): the CPU emulation of their
kernels (nanorq_amd/csrc/syms_set_emu.cpp over syms_set_body.h), the exported path and word rules, keyed packets of several
symbols in the three header forms, and the case list the CPU tier and the GPU tier share."""
import ctypes as C

import numpy as np

import nanorq_amd
from nanorq_amd import build as nbuild
import rx_support as R
import rxset_support as RS
import syms_support as S
import txset_support as XS
from tx_support import FILL

UNKNOWN_KEY = RS.UNKNOWN_KEY
ESI_MAX = S.ESI_MAX
PATHS = {0: "TX_V16", 1: "TX_V16_SHIFT", 2: "TX_DWORD", 3: "TX_BYTE", 4: "TXS_V16_KEY"}

_EMU = None


def emu_lib():
    global _EMU
    if _EMU is None:
        L = C.CDLL(nbuild.build_syms_set_emu())
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        L.emu_sys_emit_path.argtypes = [u64, u32]
        L.emu_sys_copy_word.argtypes = [u64]
        L.emu_sys_copy_word.restype = u32
        L.emu_sys_rxset_add.argtypes = [u32, vp, vp, vp, u64, vp, vp, u32, vp, u32, u32, vp]
        L.emu_sys_txset_emit.argtypes = [u32, vp, vp, vp, vp, vp, vp, u32, u32, u32, vp, u64, vp, vp]
        _EMU = L
    return _EMU


_p = RS._p
be32 = XS.be32


def emit_path(out_ptr, stride, T, hdr, rows=()):
    """the set emit's payload path by the exported rule (rows: (address, stride) pairs of every row table)"""
    al = int(out_ptr) | int(stride) | int(T)
    for addr, step in rows:
        al |= int(addr) | int(step)
    return PATHS[emu_lib().emu_sys_emit_path(al, hdr)]


def copy_word(pkt_ptr, stride, hdr, T, rows=()):
    """the set ingest's copy word (16 / 4 / 1 bytes) by the exported rule"""
    al = int(pkt_ptr) | int(stride) | int(hdr) | int(T)
    for addr, step in rows:
        al |= int(addr) | int(step)
    return int(emu_lib().emu_sys_copy_word(al))


# ---- ingest ----
class EmuSetSyms(RS.EmuSet):
    """EmuSet with the emulated ingest of packets of several symbols"""

    def add_syms(self, pkts, G, keys=None, tags=None, key_inline=False, nsym=None, results=None):
        pkts = np.ascontiguousarray(pkts, np.uint8)
        n = pkts.shape[0]
        res = np.full(n * G, R.UNTOUCHED, np.int32) if results is None else results
        ks = None if keys is None else np.ascontiguousarray(keys, np.uint32)
        tg = None if tags is None else np.ascontiguousarray(tags, np.uint32)
        ns = None if nsym is None else np.ascontiguousarray(nsym, np.uint8)
        prm = np.array([[e.K, e.T, e.nblk, e.sbn0, e.max_esi, e.rep_cap, k, z] for k, e, z in self.members], np.uint32).reshape(-1, 8)
        ptr = np.array([[a.ctypes.data for a in (e.src, e.rep, e.first, e.seen, e.gaps, e.nrep, e.rep_esi, e.live)]
                        for _, e, _ in self.members], np.uint64).reshape(-1, 8)
        rc = emu_lib().emu_sys_rxset_add(len(self.members), _p(prm), _p(ptr), _p(pkts), pkts.shape[1], _p(ks), _p(tg), int(key_inline),
                                         _p(ns), n, G, _p(res))
        assert rc != -1, "a slot's destination row was left unwritten by the classify pass"
        assert rc == 0, rc
        return res


def keyed_symbol_bytes(key, tag, T, salt=0):
    """deterministic payload of the symbol `tag` under `key` (equal keys and tags carry equal bytes, as real duplicates do)"""
    return RS.keyed_payloads(np.array([key], np.uint32), np.array([tag], np.uint32), T)[0] ^ np.uint8(salt)


def build_packets(keys, tags, counts, G, T, hdr, stride, salt=0, fill=0x5A):
    """keyed packets of several symbols [n, stride]: hdr = 0 (bare runs), 4 (FEC Payload ID) or 8 (key, FEC Payload ID); a
    malformed packet (count 0 or above G) still has G symbols' bytes"""
    n = len(tags)
    out = np.full((n, stride), fill, np.uint8)
    for k in range(n):
        c = int(counts[k]) if 1 <= int(counts[k]) <= G else G
        t = int(tags[k])
        for i in range(c):
            sym = R.tag(t >> 24, min((t & ESI_MAX) + i, ESI_MAX))
            out[k, hdr + i * T: hdr + (i + 1) * T] = keyed_symbol_bytes(int(keys[k]), sym, T, salt)
    if hdr == 8:
        out[:, :4] = be32(keys)
    if hdr:
        out[:, hdr - 4:hdr] = be32(tags)
    return out


def carrier(keys, tags, hdr):
    """how the set call is given the packets of header form hdr -> dict(keys, tags, inline / key_inline)"""
    return {0: dict(keys=keys, tags=tags), 4: dict(keys=keys, tags=None), 8: dict(keys=None, tags=None)}[hdr]


def member_view(pkts, sel, hdr):
    """the packets `sel` as a single member's own add_syms takes them: (pkts, inline) -- behind the key when it is inline"""
    return (np.ascontiguousarray(pkts[sel][:, 4:]) if hdr == 8 else pkts[sel]), hdr > 0


# the members of the shared ingest case: (name, key, K, nblk, sbn0, objZ, small rep_cap)
OBJ_KEY, OBJ_Z, OBJ_KS = 7, 3, (103, 102, 102)
MEMBERS = [("a", 5, 100, 2, 0, 0, False),   # two members with the same SBN span under different keys ...
           ("b", 9, 100, 2, 0, 0, True),    # ... this one with few repair rows (NRQ_RX_FULL)
           ("c", 5, 10, 2, 4, 0, False),    # one key with two spans
           ("oL", OBJ_KEY, 103, 1, 0, OBJ_Z, False),  # an object of two block classes: 103 / 102 / 102 symbols
           ("oS", OBJ_KEY, 102, 2, 1, OBJ_Z, False)]


def obj_max_esi():
    """the object's max_esi: twice the K' of its larger class (asked of the library when a test runs, not at import: a GPU test
    process brings torch's runtime up before the library is loaded)"""
    return 2 * nanorq_amd.params(OBJ_KS[0])["Kp"]


def member_params(spec):
    name, key, K, nblk, sbn0, objZ, small = spec
    Kp = nanorq_amd.params(K)["Kp"]
    return dict(K=K, nblk=nblk, sbn0=sbn0, Kp=Kp, rep_cap=3 if small else 24, max_esi=obj_max_esi() if objZ else 2 * Kp)


def ingest_calls(G, T, given, ncalls=2, seed=0):
    """The shared case list: per call (keys, first tags, counts or None).  Call 0 starts with the edge packets -- duplicates inside
    one call, the same SBN under two keys, given counts across K, runs past max_esi and past 2^24 - 1, counts of 0 and G + 1, unknown
    keys, SBN >= Z of the object -- and has a live repair packet at index 85, whose slots are 255..257 at G = 3 (the ING_TILE edge);
    the rest are messy streams per member (random_stream: duplicates, ESIs above max_esi, neighbouring SBNs), shuffled."""
    rng = np.random.default_rng(1000 * G + T + seed)
    calls = []
    for call in range(ncalls):
        ks, ts = [], []
        for spec in MEMBERS:
            p = member_params(spec)
            t = R.random_stream(rng, p["K"], p["nblk"], p["sbn0"], p["max_esi"], 40, sbn_span=1)
            ts.append(t)
            ks.append(np.full(len(t), spec[1], np.uint32))
        t = R.random_stream(rng, 100, 2, 0, 202, 8, dup=0)
        ts.append(t)
        ks.append(np.full(len(t), UNKNOWN_KEY, np.uint32))
        keys, tags = np.concatenate(ks), np.concatenate(ts)
        perm = rng.permutation(len(tags))
        keys, tags = keys[perm], tags[perm]
        nsym = rng.integers(1, G + 1, len(tags)).astype(np.uint8)
        if call == 0:
            edge = [(5, R.tag(0, 10), 4), (5, R.tag(0, 12), 4),             # overlapping packets: duplicates inside one call
                    (9, R.tag(0, 10), 4),                                   # the same SBN and ESIs under the other key
                    (5, R.tag(1, 98), 4), (5, R.tag(4, 8), 3),              # given counts across K (K = 100, K = 10)
                    (9, R.tag(1, 2 * 101 - 1), 4),                          # runs past max_esi
                    (5, R.tag(1, ESI_MAX - 1), 3),                          # runs past 2^24 - 1
                    (5, R.tag(0, 20), 0), (5, R.tag(0, 30), G + 1),         # malformed counts
                    (UNKNOWN_KEY, R.tag(0, 5), 0), (UNKNOWN_KEY, R.tag(0, 40), G),      # no member: untouched whatever the count
                    (5, R.tag(3, 1), 2),                                    # a key that is no object's, SBN between its spans
                    (OBJ_KEY, R.tag(OBJ_Z, 5), G), (OBJ_KEY, R.tag(200, obj_max_esi() - 1), 3),   # SBN >= Z: IGN, and ERR past max_esi
                    (OBJ_KEY, R.tag(OBJ_Z, 1), 0), (OBJ_KEY, R.tag(OBJ_Z + 1, 1), G + 1),       # SBN >= Z, malformed
                    (OBJ_KEY, R.tag(0, 100), G), (OBJ_KEY, R.tag(2, 100), G),               # both block classes
                    (9, R.tag(0, 120), G), (9, R.tag(0, 120 + G), G), (9, R.tag(0, 121), G)]  # more repair symbols than rows: FULL
            ek = np.array([e[0] for e in edge], np.uint32)
            et = np.array([e[1] for e in edge], np.uint32)
            en = np.array([e[2] if e[2] in (0, G + 1) else min(e[2], G) for e in edge], np.uint8)
            keys, tags, nsym = np.concatenate([ek, keys]), np.concatenate([et, tags]), np.concatenate([en, nsym])
            assert len(tags) > 86
            keys[85], tags[85], nsym[85] = 5, R.tag(0, 150), min(3, G)  # (ESIs no random_stream of K = 100 reaches: new to the block)
        calls.append((keys, tags, nsym if given else None))
    return calls


def foreign_codes(keys, tags, nsym, G, exp):
    """the SBN >= Z rule of the attached object (nrq_orx_add_syms), slot by slot, into exp [n * G]"""
    for k in np.flatnonzero((keys == OBJ_KEY) & ((tags >> 24) >= OBJ_Z)):
        c = int(nsym[k]) if nsym is not None else G
        if c == 0 or c > G:
            exp[k * G] = R.ERR
            continue
        e = int(tags[k]) & ESI_MAX
        for i in range(c):
            exp[k * G + i] = R.ERR if e + i > obj_max_esi() else R.IGN
    return exp


# ---- emit ----
def emu_txset_emit_syms(segs, keys, tags, nsym, G, hdr, stride):
    """The emulated set emit of packets of several symbols over sender / relay segments (txset_support.Seg; ready bits as there)
    -> (packets [n, stride], results [n], work order [n])."""
    segs = XS.table_order(segs)
    tags = np.ascontiguousarray(tags, np.uint32)
    ks = None if keys is None else np.ascontiguousarray(keys, np.uint32)
    ns = None if nsym is None else np.ascontiguousarray(nsym, np.uint8)
    n = len(tags)
    prm = np.zeros((max(1, len(segs)), 8), np.uint32)
    ptr = np.zeros((max(1, len(segs)), 9), np.uint64)
    for g, s in enumerate(segs):
        prm[g, :6] = (s.K, s.Kp, s.T, s.nblk, s.sbn0, s.key)
        ptr[g, :4] = (s.src.ctypes.data, s.src.shape[1], s.inter.ctypes.data, s.inter.shape[1] * s.T)
    bits = np.concatenate([s.ready for s in segs]) if segs else np.zeros(0, bool)
    ready = np.zeros(32, np.uint32)
    for g in np.flatnonzero(bits):
        ready[g >> 5] |= np.uint32(1 << (g & 31))
    pkts = np.full((n, stride), FILL, np.uint8)
    res = np.full(n, 77, np.int32)
    order = np.full(max(1, n), 0xFFFFFFFF, np.uint32)
    rc = emu_lib().emu_sys_txset_emit(len(segs), _p(prm), _p(ptr), _p(ready), _p(ks), _p(tags), _p(ns), n, G, hdr, _p(pkts), stride, _p(res),
                                      _p(order))
    assert rc == 0, rc
    return pkts, res, order[:n]


def member_emit_syms(seg, tags, nsym, G, hdr, stride):
    """what the member's own emulated emit_syms (syms_support.emu_emit_table) writes for `tags`, laid out in the set's header form:
    -> (packets [n, stride] with FILL where nothing is written, results).  hdr = 8: the key in front of the member's inline form."""
    inline = hdr > 0
    ready = np.zeros(8, np.uint32)
    for b in np.flatnonzero(seg.ready):
        ready[b >> 5] |= np.uint32(1 << (b & 31))
    pk, res = S.emu_emit_table([(seg.K, seg.Kp, seg.sbn0, seg.src, seg.inter.reshape(seg.nblk, -1, seg.T))], (seg.sbn0, seg.nblk, seg.nblk),
                               seg.T, G, inline, stride - (4 if hdr == 8 else 0), tags=tags, nsym=nsym, ready=ready)
    if hdr != 8:
        return pk, res
    out = np.full((len(tags), stride), FILL, np.uint8)
    out[:, 4:] = pk
    out[res == 0, :4] = np.frombuffer(int(seg.key).to_bytes(4, "big"), np.uint8)
    return out, res


def emit_cases(segs, G, rng, extra=70):
    """(keys, first tags, counts or None for the rule) of a set emit: per segment the list of test_gpu_syms._list_cases -- full and
    short packets, every result code -- plus packets of an unknown key; more than one wave at any G"""
    HI = ESI_MAX
    cases = []
    for s in segs:
        K, nblk, sbn0, c2 = s.K, s.nblk, s.sbn0, min(2, G)
        own = [(R.tag(sbn0, 0), None), (R.tag(sbn0, max(0, K - (G + 1) // 2)), None), (R.tag(sbn0 + nblk - 1, K - 1), None),
               (R.tag(sbn0 + nblk - 1, K), None), (R.tag(sbn0, min(50, K - 1)), 1), (R.tag(sbn0, K - c2), c2),
               (R.tag(sbn0 + nblk - 1, K + 3), G), (R.tag(sbn0, HI - G + 1), G),
               (R.tag(sbn0, 5), 0), (R.tag(sbn0, 5), G + 1), (R.tag(sbn0, K - 1), 2), (R.tag(sbn0, HI), 2),
               (R.tag(sbn0 + nblk, 1), 1)]
        cases += [(s.key, t, c) for t, c in own]
    cases += [(UNKNOWN_KEY, R.tag(segs[0].sbn0, 1), 1), (UNKNOWN_KEY, R.tag(segs[0].sbn0, 2), None)]
    for _ in range(extra):
        s = segs[int(rng.integers(0, len(segs)))]
        b = int(rng.integers(0, s.nblk))
        if rng.random() < 0.5:
            e = int(rng.integers(0, s.K))
            c = int(rng.integers(1, min(G, s.K - e) + 1))
        else:
            e = int(rng.integers(s.K, s.K + 40 - G + 1)) if G <= 40 else s.K
            c = int(rng.integers(1, G + 1))
        cases.append((s.key, R.tag(s.sbn0 + b, e), c))
    return cases


def case_arrays(segs, cases, G, given):
    """(keys, tags, nsym or None) of a case list; given: the rule's counts are written out"""
    keys = np.array([c[0] for c in cases], np.uint32)
    tags = np.array([c[1] for c in cases], np.uint32)
    if not given:
        return keys, tags, None

    def K_of(key, sbn):
        for s in segs:
            if s.key == key and s.sbn0 <= sbn < s.sbn0 + s.nblk:
                return s.K
        return 1 << 30
    nsym = np.array([S.rule(K_of(k, int(t) >> 24), int(t) & ESI_MAX, G) if c is None else c for k, t, c in cases], np.uint8)
    return keys, tags, nsym


def expected_emit(segs, keys, tags, nsym, G, hdr, stride):
    """the set's packets and results from each member's own emulated emit_syms over the packets of its (key, SBN span)"""
    n = len(tags)
    out = np.full((n, stride), FILL, np.uint8)
    res = np.full(n, -1, np.int32)
    sbn = tags >> 24
    for s in segs:
        sel = np.flatnonzero((keys == s.key) & (sbn >= s.sbn0) & (sbn < s.sbn0 + s.nblk))
        if not len(sel):
            continue
        pk, r = member_emit_syms(s, tags[sel], None if nsym is None else nsym[sel], G, hdr, stride)
        out[sel], res[sel] = pk, r
    return out, res
