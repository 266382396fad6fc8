"""CPU tier of the sender sets: the emulated set emit (emit_set_body.h through txset_emu.cpp) against the emulated emit of each
member alone (emit_body.h through emit_emu.cpp / held_emu.cpp) on the tags of its key, packet for packet.
  a packet whose (key, SBN) names a member: the member's FEC Payload ID, payload and result, the key in front when it is inline;
  any other packet -- unknown key, known key with a foreign SBN, an object's key with SBN >= Z -- all FILL with result -1."""
import numpy as np
import pytest

import nanorq_amd
from held_support import emu_emit_held
from rx_support import EmuRx, payloads_for
from rxset_support import MIX4, MIX360
from tx_support import emu_emit
from txset_support import (FILL, FOREIGN, NOT_READY, UNKNOWN_KEY, Seg, be32, emu_txset_emit, global_blocks, keyed_tags, mix_segs, tag)

MIXES = {"one": MIX4[2:3], "mix4": MIX4, "mix360": MIX360}
# (hdr, slack): no header, the tag, key + tag; strides with and without bytes behind the packet
FORMS = [(0, 0), (0, 5), (4, 0), (4, 12), (8, 0), (8, 3)]


def check_against_members(segs, keys, tags, pk, res, T, hdr, held_ref=None):
    """every packet of the set against its member's own emit; returns the number of packets that belong to no member"""
    inline = hdr > 0
    koff = 4 if hdr == 8 else 0
    sbn = tags >> 24
    owned = np.zeros(len(tags), bool)
    for s in segs:
        sel = np.flatnonzero((keys == s.key) & (sbn >= s.sbn0) & (sbn < s.sbn0 + s.nblk))
        assert not owned[sel].any()
        owned[sel] = True
        if not len(sel):
            continue
        mstride = T + (4 if inline else 0)
        if held_ref is None:
            mpk, mres = emu_emit(s.K, s.Kp, T, s.src, s.inter, tags[sel], inline, mstride, sbn0=s.sbn0)
        else:
            mpk, mres = held_ref(s, tags[sel], inline, mstride)
        assert np.array_equal(res[sel], mres), s.key
        assert np.array_equal(pk[sel, koff:koff + mstride], mpk), s.key
        assert (pk[sel, koff + mstride:] == FILL).all()
        if hdr == 8:
            wrote = mres == 0
            assert np.array_equal(pk[sel[wrote], :4], be32(keys[sel[wrote]]))
            assert (pk[sel[~wrote], :4] == FILL).all()
    assert (res[~owned] == FOREIGN).all() and (pk[~owned] == FILL).all()
    return int((~owned).sum())


@pytest.mark.parametrize("hdr,slack", FORMS)
@pytest.mark.parametrize("mix", sorted(MIXES))
def test_set_emit_is_each_members_emit(mix, hdr, slack):
    _set_emit_is_each_members_emit(mix, 12, hdr, slack, 700)


def _set_emit_is_each_members_emit(mix, T, hdr, slack, n):
    rng = np.random.default_rng(len(mix) * 100 + hdr * 10 + slack + T - 12)
    segs = mix_segs(rng, MIXES[mix], T)
    keys, tags = keyed_tags(rng, segs, n)
    pk, res, _ = emu_txset_emit(segs, keys, tags, hdr, T + hdr + slack)
    assert check_against_members(segs, keys, tags, pk, res, T, hdr) > 0
    assert (res[keys == UNKNOWN_KEY] == FOREIGN).all()
    return res


@pytest.mark.parametrize("hdr", [0, 4, 8])
@pytest.mark.parametrize("T", [32, 1040, 2064, 260, 65])
def test_set_emit_is_each_members_emit_at_wave_edges(T, hdr):
    """the symbol sizes at which the device's lane forms wrap into a second and third round of the wave (tests/test_gpu_txset.py
    compares the device with this emulation there): the reference itself against each member's own emulated emit, with the
    stride slack the device cases use"""
    slack = (-(T + hdr)) % 16 + 16 if T % 16 == 0 else (4 - T - hdr) % 16 if T % 4 == 0 else 1 - (T + hdr) % 2
    res = _set_emit_is_each_members_emit("mix4", T, hdr, slack, 300)
    assert (res == 0).any() and (res == FOREIGN).any()


def test_object_key_with_sbn_beyond_Z_and_no_keys():
    """an object's table -- class L, class S, a last block staged apart -- under a key of its own: SBN >= Z is no member's; and
    keys = None names key 0"""
    rng = np.random.default_rng(3)
    T = 8
    obj = [(0, 11, 2, 0), (0, 10, 3, 2), (0, 10, 1, 5)]  # Z = 6
    segs = mix_segs(rng, obj, T) + mix_segs(rng, [(4, 10, 2, 6)], T)
    keys, tags = keyed_tags(rng, segs, 400, objects=[(0, 6)])
    pk, res, _ = emu_txset_emit(segs, keys, tags, 8, T + 8)
    check_against_members(segs, keys, tags, pk, res, T, 8)
    beyond = (keys == 0) & ((tags >> 24) >= 6)
    assert beyond.any() and (res[beyond] == FOREIGN).all() and (pk[beyond] == FILL).all()
    only0 = [s for s in segs if s.key == 0]
    pk0, res0, _ = emu_txset_emit(only0, None, tags, 4, T + 4)
    check_against_members(only0, np.zeros(len(tags), np.uint32), tags, pk0, res0, T, 4)


@pytest.mark.parametrize("n", [1, 64, 65, 4096, 4097])
@pytest.mark.parametrize("mix", ["mix4", "mix360"])
def test_work_order_is_block_major(mix, n):
    rng = np.random.default_rng(n)
    T = 4
    segs = mix_segs(rng, MIXES[mix], T)
    keys, tags = keyed_tags(rng, segs, n)
    assert len(tags) == n
    pk, res, order = emu_txset_emit(segs, keys, tags, 0, T)
    assert np.array_equal(np.sort(order), np.arange(n))
    g, nb = global_blocks(segs, keys, tags)
    assert (np.diff(g[order]) >= 0).all()
    assert np.array_equal(res == FOREIGN, g == nb) and np.array_equal(res == 0, g < nb)
    if n >= 4096 and mix == "mix360":
        assert len(np.unique(g)) > 257  # bucket counters beyond 256


def _filled(rng, key, K, T, nblk, sbn0, rep_cap, loss):
    """a relay's segment over an emulated reception fed a lossy stream -> (Seg, sent tags)"""
    Kp = nanorq_amd.params(K)["Kp"]
    L = nanorq_amd.params(Kp)["L"]
    rx = EmuRx(K, T, nblk, rep_cap, sbn0=sbn0, Kp=Kp)
    sent = np.array([tag(sbn0 + b, e) for b in range(nblk) for e in range(K + K // 4 + 4)], np.uint32)
    deliv = sent[rng.random(len(sent)) >= loss]
    rng.shuffle(deliv)
    for part in np.array_split(deliv, 2):
        rx.add(payloads_for(part, T, key), tags=part)
    seg = Seg(key, K, Kp, T, sbn0, rx.src, rng.integers(0, 256, (nblk, L, T), dtype=np.uint8), rx=rx)
    return seg, sent


@pytest.mark.parametrize("hdr,stride", [(0, 20), (4, 24), (8, 31)])
def test_held_set_emit_is_each_members_held_emit(hdr, stride):
    """relays of receptions filled by the emulated ingest, some blocks ready, beside a plain sender: with NRQ_TX_HELD every relay
    member answers as its own held emit, the sender as ever; without it nothing comes from a block that is not ready"""
    rng = np.random.default_rng(hdr)
    T = 20
    a, sent_a = _filled(rng, 7, 31, T, 3, 2, 6, 0.2)
    b, sent_b = _filled(rng, 7, 30, T, 2, 5, 40, 0.3)
    c, sent_c = _filled(rng, 2, 10, T, 2, 2, 3, 0.1)
    a.ready[:] = [True, False, False]
    b.ready[:] = [False, False]
    c.ready[:] = [False, True]
    snd = mix_segs(rng, [(9, 26, 2, 2)], T)
    segs = [a, b, c] + snd
    ts, ks = [], []
    for s, sent in ((a, sent_a), (b, sent_b), (c, sent_c)):
        extra = [tag(sbn, e) for sbn in range(max(0, s.sbn0 - 1), s.sbn0 + s.nblk + 1)
                 for e in (s.rx.max_esi, s.rx.max_esi + 1, s.rx.bm_words * 32 + 31, (1 << 24) - 1, s.K + 60)]
        ts.append(np.concatenate([sent, np.array(extra, np.uint32)]))
        ks.append(np.full(len(ts[-1]), s.key, np.uint32))
    k2, t2 = keyed_tags(rng, snd, 100)
    keys, tags = np.concatenate(ks + [k2]), np.concatenate(ts + [t2])
    perm = rng.permutation(len(tags))
    keys, tags = keys[perm], tags[perm]

    def held_ref(s, mtags, inline, mstride):
        if s.rx is None:
            return emu_emit(s.K, s.Kp, T, s.src, s.inter, mtags, inline, mstride, sbn0=s.sbn0)
        return emu_emit_held([s.rx], [s.Kp], [s.inter], (s.sbn0, s.nblk, s.nblk), s.ready, mtags, inline, mstride)

    pk, res, _ = emu_txset_emit(segs, keys, tags, hdr, stride, held=True)
    check_against_members(segs, keys, tags, pk, res, T, hdr, held_ref)
    g, nb = global_blocks(segs, keys, tags)
    bits = np.concatenate([s.ready for s in sorted(segs, key=lambda s: (s.key, s.sbn0))] + [[True]])
    cold = ~bits[g]
    assert (res[cold] == 0).any() and (res[cold] == NOT_READY).any()  # held and not held symbols of blocks that are not ready
    pk0, res0, _ = emu_txset_emit(segs, keys, tags, hdr, stride, held=False)
    assert (res0[cold] == NOT_READY).all() and (pk0[cold] == FILL).all()
    warm = bits[g] & (g < nb)
    assert np.array_equal(pk0[warm], pk[warm]) and (res0[warm] == 0).all()
