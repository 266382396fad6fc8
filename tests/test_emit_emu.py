"""CPU tier of the device-resident senders (nrq_tx_*, nrq_otx_*): the emulated emit kernel (nanorq_amd/csrc/emit_emu.cpp
running the bodies of emit_body.h) on the oracle's intermediate symbols, against the oracle's source and repair symbols byte
for byte: tag lists mixing source ESIs, repair ESIs near K and ESIs near 2^24, foreign SBNs, inline headers, several strides, and
both emit_range orders against the equivalent tag list; and an object's class table of three segments (emit_all in both orders,
a tag list)."""
import numpy as np
import pytest

import nanorq_amd
from tx_support import (FILL, check_packets, emu_emit, emu_emit_range, emu_emit_table, oracle_blocks, random_tags, range_tags)


def _setup(orc, K, T, nblk, Kp, tags, seed, src_pad=0):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 256, (nblk, K * T + src_pad), dtype=np.uint8)
    reps = [[int(t) & 0xFFFFFF for t in tags if (int(t) >> 24) == sb and (int(t) & 0xFFFFFF) >= K] for sb in range(nblk)]
    blocks = oracle_blocks(orc, src, K, T, Kp, reps)
    inter = np.stack([b[0] for b in blocks])
    return src, blocks, inter


def _stride(kind, T, inline):
    need = T + (4 if inline else 0)
    return {"tight": need, "pad4": need + 4, "r16": (need + 15) // 16 * 16, "odd": need + 3 if need % 2 == 0 else need + 2}[kind]


@pytest.mark.parametrize("K,T,nblk,sbn0,kp_of", [
    (10, 16, 2, 0, None),
    (100, 13, 3, 5, None),       # K' > K, T not a multiple of 4
    (100, 16, 2, 1, 1000),       # an object's larger K' (block 0's row coded into a short block)
    (1000, 20, 2, 254, None),    # SBNs up to 255, T a multiple of 4 but not of 16
    (300, 48, 3, 0, None),
    (100, 1040, 2, 0, None),     # the sizes at which the device's 16-byte and 4-byte lane forms go into a second round of the wave
    (100, 260, 2, 0, None),
])
@pytest.mark.parametrize("inline", [False, True])
@pytest.mark.parametrize("stride_kind", ["tight", "pad4", "r16", "odd"])
def test_emulated_emit_matches_oracle(orc, K, T, nblk, sbn0, kp_of, inline, stride_kind):
    Kp = nanorq_amd.params(kp_of or K)["Kp"]
    rng = np.random.default_rng(K + T + nblk)
    tags = random_tags(rng, K, nblk, sbn0, 300)
    local = np.array([((int(t) >> 24) - sbn0) << 24 | (int(t) & 0xFFFFFF) for t in tags], np.int64)
    src, blocks, inter = _setup(orc, K, T, nblk, Kp, [t for t in local if 0 <= (t >> 24) < nblk], seed=K)
    stride = _stride(stride_kind, T, inline)
    pk, res = emu_emit(K, Kp, T, src, inter, tags, inline, stride, sbn0=sbn0)
    assert set(res.tolist()) == {0, -1}
    check_packets(pk, tags, src, blocks, K, T, nblk, sbn0, inline, res)


def test_source_stride_longer_than_a_block(orc):
    K, T, nblk, Kp = 100, 12, 3, nanorq_amd.params(100)["Kp"]
    tags = random_tags(np.random.default_rng(2), K, nblk, 0, 200, foreign=False)
    src, blocks, inter = _setup(orc, K, T, nblk, Kp, tags, seed=3, src_pad=40)
    pk, res = emu_emit(K, Kp, T, src, inter, tags, True, T + 4)
    check_packets(pk, tags, src, blocks, K, T, nblk, 0, True, res)


@pytest.mark.parametrize("interleave", [False, True])
@pytest.mark.parametrize("K,T,nblk,sbn0,esi0,n,inline,stride", [
    (10, 16, 3, 0, 0, 25, True, 32),        # source and repair ESIs in one range
    (100, 13, 4, 7, 90, 33, False, 15),
    (100, 16, 5, 0, (1 << 24) - 9, 9, True, 21),  # the last ESIs there are
])
def test_emulated_range_equals_tag_list(orc, K, T, nblk, sbn0, esi0, n, inline, stride, interleave):
    Kp = nanorq_amd.params(K)["Kp"]
    want_tags = range_tags(nblk, sbn0, esi0, n, interleave)
    local = [((int(t) >> 24) - sbn0) << 24 | (int(t) & 0xFFFFFF) for t in want_tags]
    src, blocks, inter = _setup(orc, K, T, nblk, Kp, local, seed=n)
    pk_r, tg = emu_emit_range(K, Kp, T, src, inter, esi0, n, interleave, inline, stride, sbn0=sbn0)
    assert np.array_equal(tg, want_tags)
    pk_l, res = emu_emit(K, Kp, T, src, inter, want_tags, inline, stride, sbn0=sbn0)
    assert (res == 0).all()
    assert np.array_equal(pk_r, pk_l)
    check_packets(pk_r, want_tags, src, blocks, K, T, nblk, sbn0, inline)


def test_emulated_emit_leaves_other_packets_alone(orc):
    K, T, nblk, sbn0, Kp = 10, 8, 1, 3, nanorq_amd.params(10)["Kp"]
    tags = np.array([(2 << 24) | 1, (3 << 24) | 12, (4 << 24) | 0, (3 << 24) | 2], np.uint32)
    src, blocks, inter = _setup(orc, K, T, nblk, Kp, [12], seed=1)
    pk, res = emu_emit(K, Kp, T, src, inter, tags, False, T, sbn0=sbn0)
    assert res.tolist() == [-1, 0, -1, 0]
    assert (pk[0] == FILL).all() and (pk[2] == FILL).all()
    check_packets(pk, tags, src, blocks, K, T, nblk, sbn0, False, res)


@pytest.mark.parametrize("sbn0", [0, 3])
@pytest.mark.parametrize("inline,stride_kind", [(False, "tight"), (True, "odd"), (True, "r16")])
def test_emulated_class_table(orc, sbn0, inline, stride_kind):
    """A table as nrq_otx_create builds it for an object with a short last block: class L (K = 11, K' = 12), class S (K = 10,
    K' = 10) and the last block staged apart in rows of its own.  emit_all (ESIs 0 .. K_b + nrep - 1 of every block) block-major
    and interleaved against a numpy model of the order, and a tag list with SBNs below and past the span; every payload against
    the oracle."""
    T, Z, ZL, KL, KS, nrep = 12, 5, 2, 11, 10, 7
    Ks = [KL] * ZL + [KS] * (Z - ZL)
    Kps = {K: nanorq_amd.params(K)["Kp"] for K in (KL, KS)}
    rng = np.random.default_rng(sbn0 + T)
    src = [rng.integers(0, 256, K * T, dtype=np.uint8) for K in Ks]
    want_bm = np.array([(sbn0 + b) << 24 | i for b in range(Z) for i in range(Ks[b] + nrep)], np.uint32)
    want_il = np.array(sorted(want_bm.tolist(), key=lambda t: (t & 0xFFFFFF, t >> 24)), np.uint32)
    tags = random_tags(rng, KS, Z + 1, sbn0, 300)
    # the oracle's blocks, with every repair ESI either emit asks for
    reps = [list(range(Ks[b], Ks[b] + nrep)) + [int(t) & 0xFFFFFF for t in tags if (int(t) >> 24) == sbn0 + b and (int(t) & 0xFFFFFF) >= Ks[b]]
            for b in range(Z)]
    blocks = [oracle_blocks(orc, src[b][None], Ks[b], T, Kps[Ks[b]], [reps[b]])[0] for b in range(Z)]

    def seg(b0, nb):
        K = Ks[b0]
        return (K, Kps[K], sbn0 + b0, np.stack([src[b].copy() for b in range(b0, b0 + nb)]),
                np.stack([blocks[b][0] for b in range(b0, b0 + nb)]))
    segs = [seg(0, ZL), seg(ZL, Z - ZL - 1), seg(Z - 1, 1)]
    span = (sbn0, Z, ZL)
    stride = _stride(stride_kind, T, inline)
    off = 4 if inline else 0

    def check(pk, tgs, res=None):
        for k, t in enumerate(tgs):
            b, esi = (int(t) >> 24) - sbn0, int(t) & 0xFFFFFF
            if not 0 <= b < Z:
                assert res[k] == -1 and (pk[k] == FILL).all(), k
                continue
            assert res is None or res[k] == 0, k
            want = src[b][esi * T:(esi + 1) * T] if esi < Ks[b] else blocks[b][1][esi]
            assert np.array_equal(pk[k, off:off + T], want), (k, hex(int(t)))
            assert not inline or bytes(pk[k, :4]) == int(t).to_bytes(4, "big"), k
            assert (pk[k, off + T:] == FILL).all(), k

    for interleave, want in ((0, want_bm), (1, want_il)):
        pk, got = emu_emit_table(segs, span, T, inline, stride, rng=(0, KL + nrep, KS + nrep, interleave))
        assert np.array_equal(got, want), interleave
        check(pk, want)
        pk_l, res = emu_emit_table(segs, span, T, inline, stride, tags=want)
        assert (res == 0).all() and np.array_equal(pk_l, pk), interleave
    pk, res = emu_emit_table(segs, span, T, inline, stride, tags=tags)
    assert set(res.tolist()) == {0, -1}
    check(pk, tags, res)
