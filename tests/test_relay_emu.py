"""CPU tier of the relay's emit: the emulated emit kernel (emit_body.h through emu_emit_table_ready) over one-, two- and
three-segment tables with random ready masks.  Packets of ready blocks equal the unmasked emulation's, packets of the span's
other blocks keep the fill byte and get -2 (NRQ_TX_NOT_READY), SBNs outside the span still get -1; an all-ones mask is
byte-identical to the existing entry point (emu_emit_table), in list mode and in both range orders.

The rows are random bytes, not solved blocks: what the emulation XORs is decided by the tag alone, and whether the unmasked
emulation equals the oracle is test_emit_emu.py's subject."""
import numpy as np
import pytest

import nanorq_amd
from relay_support import FOREIGN, NOT_READY, emu_emit_table_ready, mask_words
from tx_support import FILL, emu_emit_table, random_tags, tag


def _table(rng, shape, T, sbn0):
    """shape: (K, nblk) per segment, consecutive SBNs from sbn0 -> (segs, span, Ks per block of the span)"""
    segs, Ks, b0 = [], [], sbn0
    for K, nblk in shape:
        Kp = nanorq_amd.params(K)["Kp"]
        L = nanorq_amd.params(Kp)["L"]
        segs.append((K, Kp, b0, rng.integers(0, 256, (nblk, K * T), dtype=np.uint8), rng.integers(0, 256, (nblk, L, T), dtype=np.uint8)))
        Ks += [K] * nblk
        b0 += nblk
    KL = shape[0][0]
    ZL = sum(n for K, n in shape if K == KL) if len(shape) > 1 else shape[0][1]
    return segs, (sbn0, len(Ks), ZL), Ks


# one segment (a transmission), two (both block classes), three (a class split in two, as a staged last block splits it);
# a span of more than 32 blocks so that the mask's second word is used
SHAPES = [
    ([(40, 5)], 3),
    ([(31, 3), (30, 4)], 0),
    ([(31, 2), (30, 3), (30, 1)], 7),
    ([(12, 70)], 1),
    ([(13, 33), (12, 40)], 0),
]


@pytest.mark.parametrize("inline", [False, True])
@pytest.mark.parametrize("T", [16, 20, 13])
@pytest.mark.parametrize("shape,sbn0", SHAPES)
def test_masked_emit(shape, sbn0, T, inline):
    rng = np.random.default_rng(len(shape) * 1000 + T + sbn0)
    segs, span, Ks = _table(rng, shape, T, sbn0)
    Z = span[1]
    stride = T + (4 if inline else 0) + 5
    tags = random_tags(rng, min(Ks), Z + 2, max(0, sbn0 - 1), 600)  # (SBNs on both sides of the span where there is room)
    # every block of the span at least once, as a source and as a repair packet
    tags = np.concatenate([tags, [tag(sbn0 + b, 0) for b in range(Z)], [tag(sbn0 + b, Ks[b] + 3) for b in range(Z)]]).astype(np.uint32)
    ref_pk, ref_res = emu_emit_table(segs, span, T, inline, stride, tags=tags)
    blk = (tags >> 24).astype(np.int64) - sbn0
    inside = (blk >= 0) & (blk < Z)
    assert inside.any() and (~inside).any()
    assert (ref_res[inside] == 0).all() and (ref_res[~inside] == FOREIGN).all()

    for trial in range(4):
        ready = rng.random(Z) < (0.0, 0.3, 0.6, 0.9)[trial]
        if trial:  # (at least one block of either kind)
            i = int(rng.integers(0, Z))
            ready[i], ready[(i + 1) % Z] = True, False
        pk, res = emu_emit_table_ready(segs, span, T, inline, stride, ready, tags=tags)
        ok = np.zeros(len(tags), bool)
        ok[inside] = ready[blk[inside]]
        held = inside & ~ok
        assert trial == 0 or ok.any()
        assert held.any()
        assert (res[ok] == 0).all() and np.array_equal(pk[ok], ref_pk[ok])
        assert (res[held] == NOT_READY).all() and (pk[held] == FILL).all()
        assert (res[~inside] == FOREIGN).all() and (pk[~inside] == FILL).all()


@pytest.mark.parametrize("inline", [False, True])
@pytest.mark.parametrize("shape,sbn0", SHAPES)
def test_all_ones_is_the_existing_entry_point(shape, sbn0, inline):
    T = 20
    rng = np.random.default_rng(77 + len(shape) + sbn0)
    segs, span, Ks = _table(rng, shape, T, sbn0)
    Z = span[1]
    stride = T + (4 if inline else 0) + 3
    ones = np.ones(Z, bool)
    assert (mask_words(ones)[:Z // 32] == 0xFFFFFFFF).all()
    tags = random_tags(rng, min(Ks), Z + 2, max(0, sbn0 - 1), 500)
    a = emu_emit_table(segs, span, T, inline, stride, tags=tags)
    b = emu_emit_table_ready(segs, span, T, inline, stride, ones, tags=tags)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    KL, KS = Ks[0], Ks[-1]
    for interleave in (0, 1):
        r = (0, KL + 4, KS + 4, interleave)
        a = emu_emit_table(segs, span, T, inline, stride, rng=r)
        b = emu_emit_table_ready(segs, span, T, inline, stride, ones, rng=r)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert not (a[0][:, :T] == FILL).all()
