"""-m gpu tier: guard bands round the caller's buffers of nrq_encode_blocks / nrq_decode_blocks.

Every buffer the other GPU tests hand the library comes from nrq_dev_alloc, whose pool rounds to 4 KiB and reuses larger blocks: a
write a few bytes past `rep` or `inter` lands in slack and nobody sees it.  Here a case makes ONE allocation and carves `src`,
`rep` and `inter` out of it at their exact byte sizes, with 64 KiB bands of a known pattern before, between and behind them; the
block strides are exact (K*T, nrep*T, L*T), so the last row of block b abuts the first row of block b + 1.  After the call and a
sync every byte outside the three arrays is as it was, every byte of `src` a call must not write too, and every block equals the
oracle (repair and intermediate symbols; recovered rows; an undecodable block untouched).  An overrun lands in the test's own
bands: nothing faults.

Base offsets 0 and 1 / 4 / 8 bytes behind a 16-byte boundary: rows on 16-byte boundaries with T a multiple of 16 take the
aligned-only mover instance, everything else the byte-wise one -- stats()["movers_aligned"] must say which ran.  Both contexts of
gpu_support, strip widths 16 / 12 / 8 / 4 / 2 (option max_wb), a dozen shapes per width: single bytes, a partial last strip, a
partial last line group, block counts either side of the rule that maps work by block octets (8, 16, 65 by octets -- 65 leaves
an octet with one block --, the others round-robin), nrep 0 / 1 / many with and without the intermediate symbols, and two
launches with more work slots than workgroups (work slots of several strips, strip-less portions, both staging sets)."""
import numpy as np
import pytest

import nanorq_amd
from util import loss_pattern, payload, received_set, undecodable

pytestmark = pytest.mark.gpu

BAND = 64 << 10
# (K, T, nblk, nrep, want_inter)
ENCODES = [(10, 1, 1, 0, True), (10, 17, 7, 1, False), (101, 15, 8, 40, True), (101, 16, 9, 3, True), (257, 31, 33, 7, False),
           (257, 64, 8, 40, True), (101, 129, 7, 1, True), (257, 200, 9, 17, False), (10, 272, 65, 33, True), (1024, 272, 2, 9, True),
           (3100, 64, 2, 9, True),
           # more work slots than the device has workgroups: one staged element per strip (the smallest output staging stride) in slots
           # of several strips whose last has strip-less portions; the same with the intermediate symbols
           (10, 2000, 256, 1, False), (10, 1040, 512, 3, True)]
# (K, T, nblk, loss, overhead, want_inter, undecodable block or None)
DECODES = [(101, 17, 9, 0.1, 0, False, 4), (257, 64, 8, 0.05, 5, True, None), (10, 200, 33, 0.3, 0, False, 32), (101, 129, 16, 0.1, 5, False, 0),
           (10, 1040, 512, 0.3, 0, False, 511)]


def band(n, salt):
    return ((np.arange(n, dtype=np.uint32) * 131 + salt * 29 + 7) & 0xFF).astype(np.uint8)


class Carved:
    """one device allocation: band, src, band, rep, band, inter, band -- each array `off` bytes behind a 16-byte boundary"""

    def __init__(self, c, off, sizes):
        self.c, self.sizes = c, sizes
        self.at, pos = [], BAND
        for n in sizes:
            pos = (pos + 15) // 16 * 16 + off
            self.at.append(pos)
            pos += n + BAND
        self.total = pos
        self.host = band(self.total, off)
        self.base = c.alloc(self.total)
        assert self.base % 16 == 0

    def ptr(self, i):
        return self.base + self.at[i] if self.sizes[i] else 0

    def put(self, i, data):
        self.host[self.at[i]:self.at[i] + self.sizes[i]] = np.ascontiguousarray(data, np.uint8).reshape(-1)

    def run(self, call):
        """upload, call, sync, download; returns (what the arrays hold now, bytes outside them that changed)"""
        try:
            self.c.upload(self.base, self.host)
            res = call()
            self.c.sync()
            now = self.c.download(self.base, self.total)
        finally:
            self.c.free(self.base)
        outside = np.ones(self.total, bool)
        for a, n in zip(self.at, self.sizes):
            outside[a:a + n] = False
        changed = np.nonzero(outside & (now != self.host))[0]
        return res, [now[a:a + n] for a, n in zip(self.at, self.sizes)], changed


def expect_aligned(cv, T, stats):
    """the host's rule (Rows::aligned, solve_shape): every row of the call on a 16-byte boundary, T a multiple of 16, strips of 4 bytes at least"""
    rows16 = all(cv.ptr(i) % 16 == 0 for i in range(3)) and T % 16 == 0
    return 1 if rows16 and stats["strip_bytes"] >= 4 else 0


def encode_case(G, orc, wb, K, T, nblk, nrep, want_inter, off):
    c = G.ctx()
    L = nanorq_amd.params(K)["L"]
    what = (G.kind, wb, "encode", K, T, nblk, nrep, want_inter, off)
    src = np.stack([payload(K * T, seed=3, block=b).reshape(K, T) for b in range(nblk)])
    esis = np.arange(K, K + nrep, dtype=np.uint32)
    cv = Carved(c, off, [nblk * K * T, nblk * nrep * T, nblk * L * T if want_inter else 0])
    cv.put(0, src)
    _, (d_src, d_rep, d_int), changed = cv.run(
        lambda: c.encode_blocks(K, T, nblk, cv.ptr(0), K * T, cv.ptr(1), nrep * T, esis, cv.ptr(2), L * T))
    st = c.stats()
    assert changed.size == 0, (what, "bytes outside the arrays changed", changed[:8] - np.array(cv.at[:1]), cv.at, cv.sizes)
    assert np.array_equal(d_src, src.reshape(-1)), (what, "the source symbols were written")
    assert st["strip_bytes"] == wb and st["movers_aligned"] == expect_aligned(cv, T, st), (what, st)
    rep = d_rep.reshape(nblk, nrep, T)
    inter = d_int.reshape(nblk, L, T) if want_inter else None
    for b in range(nblk):
        r_rep, r_int, _ = orc.encode_block(src[b], K, T, esis, want_inter=want_inter)
        assert np.array_equal(rep[b], r_rep), (what, b, "repair symbols")
        if want_inter:
            assert np.array_equal(inter[b], r_int), (what, b, "intermediate symbols")
    return st


def decode_case(G, orc, wb, K, T, nblk, loss, oh, want_inter, bad, off):
    c = G.ctx()
    L = nanorq_amd.params(K)["L"]
    what = (G.kind, wb, "decode", K, T, nblk, loss, oh, want_inter, bad, off)
    src = np.stack([payload(K * T, seed=4, block=b).reshape(K, T) for b in range(nblk)])
    lost = [undecodable(orc, K, b) if b == bad else loss_pattern(K, loss, seed=77, block=b) for b in range(nblk)]
    use = [len(x) + (oh if len(x) and b != bad else 0) for b, x in enumerate(lost)]
    cap = max(1, max(use))
    lost_a = np.zeros((nblk, max(1, max(len(x) for x in lost))), np.uint32)
    esi_a = np.tile(np.arange(K, K + cap, dtype=np.uint32), (nblk, 1))
    reps = np.zeros((nblk, cap, T), np.uint8)
    work = src.copy()
    inters, ok = [], []
    for b in range(nblk):
        lost_a[b, :len(lost[b])] = lost[b]
        r, r_int, _ = orc.encode_block(src[b], K, T, esi_a[b, :use[b]], want_inter=True)
        reps[b, :use[b]] = r
        reps[b, use[b]:] = 0x5C  # (rows the call is not given: it must not need them)
        inters.append(r_int)
        work[b][lost[b]] = 0x77
        rx = received_set(K, lost[b], use[b] - len(lost[b]))  # the verdict of the reference algorithm (no overhead: ~1 % of the blocks fail)
        ok.append(orc.decode_block(rx, np.concatenate([src[b][rx[rx < K]], r]) if use[b] else src[b], K, T)[0])
    assert bad is None or not ok[bad]
    cv = Carved(c, off, [nblk * K * T, nblk * cap * T, nblk * L * T if want_inter else 0])
    cv.put(0, work)
    cv.put(1, reps)
    nl, nu = np.array([len(x) for x in lost], np.uint32), np.array(use, np.uint32)
    status, (d_src, d_rep, d_int), changed = cv.run(
        lambda: c.decode_blocks(K, T, nblk, cv.ptr(0), K * T, lost_a, nl, esi_a, nu, cv.ptr(1), cap * T, cv.ptr(2), L * T))
    st = c.stats()
    assert changed.size == 0, (what, "bytes outside the arrays changed", changed[:8], cv.at, cv.sizes)
    assert np.array_equal(d_rep, reps.reshape(-1)), (what, "the repair symbols were written")
    assert st["strip_bytes"] == wb and st["movers_aligned"] == expect_aligned(cv, T, st), (what, st)
    out = d_src.reshape(nblk, K, T)
    for b in range(nblk):
        assert bool(status[b]) == ok[b], (what, b, "verdict")
        assert np.array_equal(out[b], src[b] if ok[b] else work[b]), (what, b, "recovered rows" if ok[b] else "undecodable block touched")
        if want_inter and ok[b] and len(lost[b]):
            assert np.array_equal(d_int.reshape(nblk, L, T)[b], inters[b]), (what, b, "intermediate symbols")
    return st


@pytest.mark.parametrize("wb", [16, 12, 8, 4, 2])
@pytest.mark.parametrize("kind", ["forced", "default"])
def test_calls_stay_inside_the_caller_s_buffers(orc, kind, wb):
    import gpu_support
    G = gpu_support.bound(kind)
    c = G.ctx()
    c.set_option("max_wb", wb)
    seen = set()
    try:
        for i, (K, T, nblk, nrep, want_inter) in enumerate(ENCODES):
            for off in (0, (1, 4, 8)[i % 3]):
                st = encode_case(G, orc, wb, K, T, nblk, nrep, want_inter, off)
                seen.add((st["movers_aligned"], st["wg_threads"], st["strips_per_slot"] > 1))
        for i, (K, T, nblk, loss, oh, want_inter, bad) in enumerate(DECODES):
            for off in (0, (4, 8, 1)[i % 3]):
                st = decode_case(G, orc, wb, K, T, nblk, loss, oh, want_inter, bad, off)
                seen.add((st["movers_aligned"], st["wg_threads"], st["strips_per_slot"] > 1))
    finally:
        c.set_option("max_wb", 16)
    # both mover instances ran (2-byte strips have the byte-wise one only), and a launch whose work slots hold several strips
    assert {a for a, _, _ in seen} == ({0, 1} if wb >= 4 else {0}), seen
    assert any(multi for _, _, multi in seen), seen
