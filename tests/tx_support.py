"""Test support for the device-resident senders (nrq_tx_*, nrq_otx_*): the CPU emulation of their emit kernel
(nanorq_amd/csrc/emit_emu.cpp over emit_body.h), the packets the oracle says a transmission must produce, and tag
lists."""
import ctypes as C

import numpy as np

import nanorq_amd
from nanorq_amd import build as nbuild

FILL = 0xA5  # bytes of an output buffer before an emit: packets left untouched keep them

_EMU = None


def emu_lib():
    global _EMU
    if _EMU is None:
        L = C.CDLL(nbuild.build_emit_emu())
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        L.emu_tx_emit.argtypes = [vp, vp, u64, vp, u64, vp, u32, u32, vp, u64, vp]
        L.emu_tx_emit_range.argtypes = [vp, vp, u64, vp, u64, u32, u32, u32, u32, vp, u64, vp]
        L.emu_emit_table.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp, u32, vp, u32, vp, u64, vp, vp]
        _EMU = L
    return _EMU


def tag(sbn, esi):
    return (int(sbn) << 24) | int(esi)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _prm(K, Kp, T, nblk, sbn0):
    return np.array([K, Kp, T, nblk, sbn0], np.uint32)


def emu_emit(K, Kp, T, src, inter, tags, inline, stride, sbn0=0, pkts=None):
    """src [nblk, K*T or more] uint8, inter [nblk, L, T] uint8 -> (packets [n, stride], results [n])"""
    nblk = src.shape[0]
    src = np.ascontiguousarray(src.reshape(nblk, -1), np.uint8)
    inter = np.ascontiguousarray(inter, np.uint8)
    tags = np.ascontiguousarray(tags, np.uint32)
    n = len(tags)
    pkts = np.full((n, stride), FILL, np.uint8) if pkts is None else pkts
    res = np.full(n, 77, np.int32)
    rc = emu_lib().emu_tx_emit(_p(_prm(K, Kp, T, nblk, sbn0)), _p(src), src.shape[1], _p(inter), inter.shape[1] * T, _p(tags), n,
                               int(inline), _p(pkts), stride, _p(res))
    assert rc == 0, rc
    return pkts, res


def emu_emit_range(K, Kp, T, src, inter, esi0, n, interleave, inline, stride, sbn0=0):
    """-> (packets [n*nblk, stride], tags [n*nblk])"""
    nblk = src.shape[0]
    src = np.ascontiguousarray(src.reshape(nblk, -1), np.uint8)
    inter = np.ascontiguousarray(inter, np.uint8)
    pkts = np.full((n * nblk, stride), FILL, np.uint8)
    tags = np.zeros(n * nblk, np.uint32)
    rc = emu_lib().emu_tx_emit_range(_p(_prm(K, Kp, T, nblk, sbn0)), _p(src), src.shape[1], _p(inter), inter.shape[1] * T, esi0, n,
                                     int(interleave), int(inline), _p(pkts), stride, _p(tags))
    assert rc == 0, rc
    return pkts, tags


def emu_emit_table(segs, span, T, inline, stride, tags=None, rng=None):
    """The emit from a table of segments, each (K, Kp, sbn0, src [nblk, K*T or more], inter [nblk, L, T]), over the span
    (sbn0, Z, ZL): a tag list (tags) or range mode (rng = (esi0, nL, nS, interleave)) -> (packets [n, stride], results [n] or the
    tags [n] range mode wrote)"""
    srcs = [np.ascontiguousarray(s[3].reshape(s[3].shape[0], -1), np.uint8) for s in segs]
    inters = [np.ascontiguousarray(s[4], np.uint8) for s in segs]
    prm = np.array([[K, Kp, T, src.shape[0], sbn0] for (K, Kp, sbn0, _, _), src in zip(segs, srcs)], np.uint32)
    nseg = len(segs)

    def per_seg(ctype, vals):
        return (ctype * nseg)(*vals)
    sbn0, Z, ZL = span
    if tags is not None:
        tags = np.ascontiguousarray(tags, np.uint32)
        n = len(tags)
        out = np.full(n, 77, np.int32)
        res, tags_out, range_ = out, None, None
    else:
        esi0, nL, nS, _ = rng
        n = ZL * nL + (Z - ZL) * nS
        out = np.zeros(n, np.uint32)
        res, tags_out, range_ = None, out, np.array(rng, np.uint32)
    pkts = np.full((n, stride), FILL, np.uint8)
    rc = emu_lib().emu_emit_table(_p(prm), nseg, _p(np.array(span, np.uint32)),
                                  per_seg(C.c_void_p, [a.ctypes.data for a in srcs]), per_seg(C.c_uint64, [a.shape[1] for a in srcs]),
                                  per_seg(C.c_void_p, [a.ctypes.data for a in inters]),
                                  per_seg(C.c_uint64, [a.shape[1] * T for a in inters]), _p(tags), n if tags is not None else 0,
                                  _p(range_), int(inline), _p(pkts), stride, _p(res), _p(tags_out))
    assert rc == 0, rc
    return pkts, out


def range_tags(nblk, sbn0, esi0, n, interleave):
    """the tag list emit_range(esi0, n) stands for"""
    k = np.arange(n * nblk, dtype=np.uint64)
    if interleave:
        b, i = k % nblk, k // nblk
    else:
        b, i = k // n, k % n
    return (((b + sbn0) << np.uint64(24)) | (i + esi0)).astype(np.uint32)


def oracle_blocks(orc, src, K, T, Kp, repair_esis):
    """per block: (inter [L, T], {esi: repair payload}) from the oracle; repair_esis: per block a list of ESIs >= K"""
    out = []
    for b in range(src.shape[0]):
        esis = np.unique(np.asarray(repair_esis[b], np.uint32))
        rep, inter, _ = orc.encode_block(src[b].reshape(-1)[:K * T], K, T, esis, want_inter=True, Kp=Kp)
        out.append((inter, {int(e): rep[q] for q, e in enumerate(esis)}))
    return out


def expected_payload(src, blocks, K, T, b, esi):
    return src[b].reshape(-1)[esi * T:(esi + 1) * T] if esi < K else blocks[b][1][esi]


def check_packets(pkts, tags, src, blocks, K, T, nblk, sbn0, inline, results=None):
    """every packet of the transmission against the oracle (header big-endian SBN|ESI when inline; bytes past the packet keep
    FILL); foreign packets untouched with result -1"""
    off = 4 if inline else 0
    for k, t in enumerate(np.asarray(tags, np.uint32)):
        sbn, esi = int(t) >> 24, int(t) & 0xFFFFFF
        b = sbn - sbn0
        if not 0 <= b < nblk:
            assert (pkts[k] == FILL).all(), k
            if results is not None:
                assert results[k] == -1, k
            continue
        if results is not None:
            assert results[k] == 0, k
        if inline:
            assert bytes(pkts[k, :4]) == int(t).to_bytes(4, "big"), k
        assert np.array_equal(pkts[k, off:off + T], expected_payload(src, blocks, K, T, b, esi)), (k, sbn, esi)
        assert (pkts[k, off + T:] == FILL).all(), k


def random_tags(rng, K, nblk, sbn0, n, foreign=True):
    """source ESIs, repair ESIs just above K, ESIs just below 2^24 and (foreign) SBNs next to the transmission, shuffled"""
    out = []
    lo, hi = (max(0, sbn0 - 1), min(256, sbn0 + nblk + 1)) if foreign else (sbn0, sbn0 + nblk)
    for _ in range(n):
        u = rng.random()
        if u < 0.4:
            esi = int(rng.integers(0, K))
        elif u < 0.8:
            esi = int(rng.integers(K, K + 40))
        else:
            esi = int(rng.integers((1 << 24) - 30, 1 << 24))
        out.append(tag(int(rng.integers(lo, hi)), esi))
    return np.array(out, np.uint32)


def params_L(Kp):
    return nanorq_amd.params(Kp)["L"]


def emit_mode(out_ptr, stride, T, hdr, rows=()):
    """The payload path an emit takes, by the rule of tx_launch / nrq_txset_emit restated: OR the packet buffer's address, its
    stride, T and every row table's address and stride (rows: (address, stride) pairs -- the source rows, the intermediate
    symbols at inter_ptr with stride L * T, for a held emit the receptions' repair rows); all 16-byte aligned: the 16-byte form of
    the header (hdr = 0, 4 or 8 bytes), 4-byte aligned: dwords, else bytes.  There is no statistic for the mode: a test asserts
    this on what it hands to the call, so that a case cannot pass on another path than the one it is listed for."""
    al = int(out_ptr) | int(stride) | int(T)
    for addr, step in rows:
        al |= int(addr) | int(step)
    if al % 16 == 0:
        return {0: "TX_V16", 4: "TX_V16_SHIFT", 8: "TXS_V16_KEY"}[hdr]
    return "TX_DWORD" if al % 4 == 0 else "TX_BYTE"


def copy_forms(pkt_ptr, pkt_stride, payload_off, n, T, row_ptrs):
    """The forms nrq_ing_copy_kernel takes over n packets, by its rule restated: per packet the payload's address (packet k at
    pkt_ptr + k * pkt_stride, the payload payload_off bytes in), the row's address and T ORed; 16-byte aligned: "v16", 4-byte
    aligned: "dword", else "byte".  row_ptrs: the addresses of the row tables a packet may land in (rows lie T bytes apart, so a
    row is as aligned as its table and T allow).  Returns the set of forms."""
    d = int(T)
    for p in row_ptrs:
        d |= int(p)
    out = set()
    for k in range(min(n, 16)):  # (the low four bits of k * stride repeat after 16 packets)
        al = (int(pkt_ptr) + k * int(pkt_stride) + payload_off) | d
        out.add("v16" if al % 16 == 0 else "dword" if al % 4 == 0 else "byte")
    return out
