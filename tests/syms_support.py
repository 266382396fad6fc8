"""Test support for packets of several symbols (nrq_*_syms): the CPU emulation of their kernels (nanorq_amd/csrc/syms_emu.cpp over
syms_body.h), the exported count / range / path rules, and plain Python restatements of the slot maps -- the expansion of a packet
list into one-symbol packets, which the existing one-symbol models and emulations (rx_support, tx_support) then judge."""
import ctypes as C

import numpy as np

from nanorq_amd import build as nbuild
import rx_support as R
import tx_support as X

BAD_RANGE = -3
G_MAX = 64
ESI_MAX = 0xFFFFFF
PATHS = {0: "TX_V16", 1: "TX_V16_SHIFT", 2: "TX_DWORD", 3: "TX_BYTE"}

_EMU = None


def emu_lib():
    global _EMU
    if _EMU is None:
        L = C.CDLL(nbuild.build_syms_emu())
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        L.emu_sy_rule.argtypes = [u32, u32, u32]
        L.emu_sy_rule.restype = u32
        L.emu_sy_pkt_count.argtypes = [u32, u32, u32, u32]
        L.emu_sy_pkt_count.restype = u32
        L.emu_sy_range_pkt.argtypes = [u32, u32, u32, u32, u32, vp, vp]
        L.emu_sy_range_pkt.restype = None
        L.emu_sy_range_index.argtypes = [u32, u32, u32, u32, u32]
        L.emu_sy_range_index.restype = u32
        L.emu_sy_emit_path.argtypes = [u64, u32]
        L.emu_sy_copy_word.argtypes = [u64]
        L.emu_sy_copy_word.restype = u32
        L.emu_sy_emit_table.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp, vp, u32, u32, vp, u32, vp, u64, vp, vp, vp, vp, vp, vp]
        L.emu_sy_rx_add.argtypes = [vp, vp, u64, vp, u64, vp, vp, vp, vp, vp, vp, vp, u64, vp, vp, u32, u32, vp]
        _EMU = L
    return _EMU


_p = X._p


# ---- plain restatements ----
def rule(K, e, G):
    return min(G, K - e) if e < K else G


def range_packets(K, esi0, n, G):
    """[(first ESI, count)] of one block: the source run, then the repair run, each cut into packets of G"""
    out = []
    for lo, hi in ((esi0, min(K, esi0 + n)), (max(K, esi0), esi0 + n)):
        e = lo
        while e < hi:
            out.append((e, min(G, hi - e)))
            e += G
    return out


def range_list(blocks, sbn0, esi0, ns, G, interleave):
    """blocks: K per block (SBN order), ns: ESIs per block -> (first tags, counts) in packet order"""
    per = [range_packets(K, esi0, n, G) for K, n in zip(blocks, ns)]
    order = []
    if interleave:
        for j in range(max(len(p) for p in per) if per else 0):
            order += [(b, j) for b in range(len(per)) if j < len(per[b])]
    else:
        order = [(b, j) for b in range(len(per)) for j in range(len(per[b]))]
    tags = np.array([R.tag(sbn0 + b, per[b][j][0]) for b, j in order], np.uint32)
    cnt = np.array([per[b][j][1] for b, j in order], np.uint8)
    return tags, cnt


def rx_counts(tags, nsym, G, K_of):
    """the count a receiver takes for each packet (0: malformed); K_of(sbn) -> K or None outside"""
    out = []
    for k, t in enumerate(np.asarray(tags, np.uint32)):
        if nsym is not None:
            c = int(nsym[k])
            out.append(c if 1 <= c <= G else 0)
        else:
            K = K_of(int(t) >> 24)
            out.append(rule(K, int(t) & ESI_MAX, G) if K is not None else G)
    return out


def expansion(tags, counts, G):
    """-> (slots [m], sbn [m], esi [m]) of the one-symbol packets in slot order; the ESI is computed in ESI space (it may pass
    2^24 - 1: such a symbol does not exist)"""
    slots, sbn, esi = [], [], []
    for k, t in enumerate(np.asarray(tags, np.uint32)):
        for i in range(counts[k]):
            slots.append(k * G + i)
            sbn.append(int(t) >> 24)
            esi.append((int(t) & ESI_MAX) + i)
    return np.array(slots, np.int64), np.array(sbn, np.int64), np.array(esi, np.int64)


def model_add(model, pkts, tags, nsym, G, hdr, results, K_of=None):
    """ModelRx over the expansion of (pkts [n, stride], first tags, counts): results [n * G] updated in place.  A malformed count
    gives slot k * G ERR (inside the reception); a symbol past 2^24 - 1 is ERR."""
    K_of = K_of or (lambda sbn: model.K if model.sbn0 <= sbn < model.sbn0 + model.nblk else None)
    T = model.T
    cnt = rx_counts(tags, nsym, G, K_of)
    for k, t in enumerate(np.asarray(tags, np.uint32)):
        if cnt[k] == 0 and K_of(int(t) >> 24) is not None:
            results[k * G] = R.ERR
    slots, sbn, esi = expansion(tags, cnt, G)
    for s, b, e in zip(slots, sbn, esi):
        if K_of(int(b)) is None:
            continue
        if e > ESI_MAX:
            results[s] = R.ERR
            continue
        k, i = divmod(int(s), G)
        one = np.full(1, R.UNTOUCHED, np.int32)
        model.add([pkts[k, hdr + i * T: hdr + (i + 1) * T]], [R.tag(b, e)], one)
        results[s] = one[0]
    return results


class EmuRxSyms(R.EmuRx):
    """EmuRx with the emulated ingest of packets of several symbols"""

    def add_syms(self, pkts, G, tags=None, nsym=None, results=None):
        pkts = np.ascontiguousarray(pkts, np.uint8)
        n = pkts.shape[0]
        res = np.full(n * G, R.UNTOUCHED, np.int32) if results is None else results
        tg = None if tags is None else np.ascontiguousarray(tags, np.uint32)
        ns = None if nsym is None else np.ascontiguousarray(nsym, np.uint8)
        prm = np.array([self.K, self.T, self.nblk, self.sbn0, self.max_esi, self.rep_cap], np.uint32)
        rc = emu_lib().emu_sy_rx_add(_p(prm), _p(self.src), self.K * self.T, _p(self.rep), self.rep_cap * self.T, _p(self.first),
                                     _p(self.seen), _p(self.gaps), _p(self.nrep), _p(self.rep_esi), _p(self.live), _p(pkts), pkts.shape[1],
                                     _p(tg), _p(ns), n, G, _p(res))
        assert rc == 0, "a slot's destination row was left unwritten"
        return res


def pack(payloads, tags, G, T, hdr, stride, fill=0):
    """packets [n, stride] from per-packet payload runs (payloads[k]: [c_k * T] bytes) with the inline header when hdr = 4"""
    n = len(tags)
    out = np.full((n, stride), fill, np.uint8)
    for k in range(n):
        if hdr:
            out[k, :4] = np.frombuffer(int(tags[k]).to_bytes(4, "big"), np.uint8)
        out[k, hdr:hdr + len(payloads[k])] = payloads[k]
    return out


def emu_emit_table(segs, span, T, G, inline, stride, tags=None, nsym=None, rng=None, ready=None, maps_only=False):
    """The emulated emit from a table of segments (as tx_support.emu_emit_table): a list of first tags (tags, nsym or None) ->
    (packets, results); or range mode rng = (esi0, eL, eS, interleave) -> (packets, first tags, counts, back) where back[k] is packet
    k's index found again from its block and first ESI.  maps_only: no rows are needed (segs' arrays may be None)."""
    L = emu_lib()
    nseg = len(segs)
    if maps_only:
        prm = np.array([[K, Kp, T, nb, sbn0] for (K, Kp, sbn0, nb, _) in segs], np.uint32)
        srcs = inters = None
    else:
        srcs = [np.ascontiguousarray(s[3].reshape(s[3].shape[0], -1), np.uint8) for s in segs]
        inters = [np.ascontiguousarray(s[4], np.uint8) for s in segs]
        prm = np.array([[K, Kp, T, src.shape[0], sbn0] for (K, Kp, sbn0, _, _), src in zip(segs, srcs)], np.uint32)

    def per_seg(ctype, vals):
        return (ctype * nseg)(*vals)
    sp = np.array(span, np.uint32)
    rd = None if ready is None else np.ascontiguousarray(ready, np.uint32)
    a_src = per_seg(C.c_void_p, [a.ctypes.data for a in srcs]) if srcs else None
    a_ss = per_seg(C.c_uint64, [a.shape[1] for a in srcs]) if srcs else None
    a_in = per_seg(C.c_void_p, [a.ctypes.data for a in inters]) if srcs else None
    a_is = per_seg(C.c_uint64, [a.shape[1] * T for a in inters]) if srcs else None
    if tags is not None:
        tags = np.ascontiguousarray(tags, np.uint32)
        ns = None if nsym is None else np.ascontiguousarray(nsym, np.uint8)
        n = len(tags)
        res = np.full(n, 77, np.int32)
        pkts = np.full((n, stride), X.FILL, np.uint8)
        rc = L.emu_sy_emit_table(_p(prm), nseg, _p(sp), a_src, a_ss, a_in, a_is, _p(tags), _p(ns), n, G, None, int(inline), _p(pkts), stride,
                                 _p(res), None, None, None, None, _p(rd))
        assert rc == 0, rc
        return pkts, res
    r4 = np.array(rng, np.uint32)
    npkt = np.zeros(1, np.uint32)
    # a first pass for the packet count, the maps and the way back
    cap = int(sum(s[3] if maps_only else s[3].shape[0] for s in segs)) * (int(max(rng[1], rng[2])) + 2)
    t_out, c_out, back = np.zeros(cap, np.uint32), np.zeros(cap, np.uint8), np.zeros(cap, np.uint32)
    rc = L.emu_sy_emit_table(_p(prm), nseg, _p(sp), a_src, a_ss, a_in, a_is, None, None, 0, G, _p(r4), int(inline), None, stride, None,
                             _p(t_out), _p(c_out), _p(back), _p(npkt), _p(rd))
    assert rc == 0, rc
    n = int(npkt[0])
    if maps_only:
        return None, t_out[:n], c_out[:n], back[:n]
    pkts = np.full((n, stride), X.FILL, np.uint8)
    t2, c2 = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint8)
    rc = L.emu_sy_emit_table(_p(prm), nseg, _p(sp), a_src, a_ss, a_in, a_is, None, None, 0, G, _p(r4), int(inline), _p(pkts), stride, None,
                             _p(t2), _p(c2), None, None, _p(rd))
    assert rc == 0, rc
    assert np.array_equal(t2[:n], t_out[:n]) and np.array_equal(c2[:n], c_out[:n])
    return pkts, t_out[:n], c_out[:n], back[:n]


def expanded_emit(K, Kp, T, src, inter, tags, counts, G, inline, stride, sbn0=0):
    """what the one-symbol emulation (tx_support.emu_emit) writes for the expansion, laid out as packets of several symbols:
    -> packets [n, stride] (FILL where nothing is written).  counts[k] = 0: the packet stays untouched."""
    hdr = 4 if inline else 0
    n = len(tags)
    out = np.full((n, stride), X.FILL, np.uint8)
    slots, sbn, esi = expansion(tags, counts, G)
    if len(slots) == 0:
        return out
    one_tags = np.array([R.tag(b, e) for b, e in zip(sbn, esi)], np.uint32)
    one, res = X.emu_emit(K, Kp, T, src, inter, one_tags, inline, T + hdr, sbn0=sbn0)
    assert (res == 0).all()
    for q, s in enumerate(slots):
        k, i = divmod(int(s), G)
        if i == 0 and hdr:
            out[k, :4] = one[q, :4]
        out[k, hdr + i * T: hdr + (i + 1) * T] = one[q, hdr:hdr + T]
    return out


def emit_path(out_ptr, stride, T, inline, rows=()):
    """the emit's payload path by the exported rule (rows: (address, stride) pairs of every row table)"""
    al = int(out_ptr) | int(stride) | int(T)
    for addr, step in rows:
        al |= int(addr) | int(step)
    return PATHS[emu_lib().emu_sy_emit_path(al, 1 if inline else 0)]


def copy_word(pkt_ptr, stride, hdr, T, rows=()):
    """the ingest copy's word (16 / 4 / 1 bytes) by the exported rule"""
    al = int(pkt_ptr) | int(stride) | int(hdr) | int(T)
    for addr, step in rows:
        al |= int(addr) | int(step)
    return int(emu_lib().emu_sy_copy_word(al))
