"""CPU tier of the range mode of a sender set: the emulated map pass (emit_set_range_body.h through txset_range_emu.cpp) against
the plain numpy statement of the map (txset_range_support.range_ref), word for word -- keys, first tags, counts -- with the work
order a block-major permutation; and the packets of those lists through the emulated set emit, which is not changed, against
each member's own emulated emit."""
import numpy as np
import pytest

from rxset_support import MIX4
from test_txset_emu import check_against_members
from txset_range_support import CALLS, TABLES, blocks_of, emu_range, global_block, range_ref
from txset_support import emu_txset_emit, mix_segs


@pytest.mark.parametrize("order,source,rep0,nrep,G", CALLS)
@pytest.mark.parametrize("table", sorted(TABLES))
def test_emulated_map_is_the_numpy_statement(table, order, source, rep0, nrep, G):
    mix = TABLES[table]
    keys, tags, cnts, lens = range_ref(mix, order, source, rep0, nrep, G)
    n = len(tags)
    assert n == int(lens.sum())
    ek, et, ec, seg, worder = emu_range(mix, order, source, rep0, nrep, G, n)
    assert np.array_equal(ek, keys), np.flatnonzero(ek != keys)[:10]
    assert np.array_equal(et, tags), np.flatnonzero(et != tags)[:10]
    assert np.array_equal(ec, cnts), np.flatnonzero(ec != cnts)[:10]
    if not n:
        return
    # the work order: a permutation of the packets, block after block, a block's packets in their own order
    assert np.array_equal(np.sort(worder), np.arange(n))
    g = global_block(mix, keys, tags)
    assert (np.diff(g[worder]) >= 0).all()
    bk, bt, _, _ = range_ref(mix, 0, source, rep0, nrep, G)
    assert np.array_equal(keys[worder], bk) and np.array_equal(tags[worder], bt)
    # the segment of every packet: the table row that holds its (key, SBN)
    rows = sorted(mix, key=lambda m: (m[0], m[3]))
    for k in range(0, n, max(1, n // 97)):
        key, K, nblk, sbn0 = rows[seg[k]]
        assert key == keys[k] and sbn0 <= (int(tags[k]) >> 24) < sbn0 + nblk
    # what the cases are chosen for
    if table == "mix4" and (source, nrep, G) == (1, 5, 1):
        assert n == 1052 and n % 64 and sorted(set(lens.tolist())) == [15, 31, 105]
    if table == "mix360" and (source, nrep, G) == (1, 5, 1):
        assert n == 360 * 15 > 4096 and len(blocks_of(mix)) > 256
    if G == 4 and source:
        assert (cnts[(tags & 0xFFFFFF) == 8] == 2).any()  # K = 10: a short last source packet
    if G == 64 and source:
        assert (cnts[(tags & 0xFFFFFF) == 0] == 10).any()  # G exceeds K = 10: the whole source run is one short packet


def test_mix360_with_two_repair_symbols():
    """the issue's count: 360 blocks of K = 10 with nrep = 2 are 4320 packets, every length tied"""
    keys, tags, cnts, lens = range_ref(TABLES["mix360"], 1, 1, 0, 2, 1)
    assert len(tags) == 4320 and (lens == 12).all()
    ek, et, ec, _, worder = emu_range(TABLES["mix360"], 1, 1, 0, 2, 1, 4320)
    assert np.array_equal(ek, keys) and np.array_equal(et, tags) and (ec == 1).all()
    assert np.array_equal(worder.reshape(360, 12), np.arange(4320).reshape(12, 360).T)  # round j, block g <-> item g * 12 + j


def test_rank_across_dead_segments():
    """MIX4 in order 1: the K = 10 segment (the middle one in block order) drops out at round 15, the K = 26 segment (the first) at
    round 31; behind that a block's rank is taken across a dead segment, then with a dead segment in front"""
    keys, tags, _, lens = range_ref(MIX4, 1, 1, 0, 5, 1)
    assert lens.tolist() == [31] * 2 + [15] * 3 + [105] * 9
    _, et, _, _, _ = emu_range(MIX4, 1, 1, 0, 5, 1, len(tags))
    assert np.array_equal(et, tags)
    esi = tags & 0xFFFFFF
    r15, r31 = np.flatnonzero(esi == 15), np.flatnonzero(esi == 31)
    assert len(r15) == 11 and np.array_equal(r15, 14 * 15 + np.arange(11)) and (keys[r15[:2]] == 0).all() and (keys[r15[2:]] != 0).all()
    assert len(r31) == 9 and np.array_equal(r31, 14 * 15 + 11 * 16 + np.arange(9)) and (keys[r31] != 0).all()


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("hdr", [0, 4, 8])
def test_packets_of_the_map_are_each_members_packets(hdr, order):
    """the lists of the map through the existing emulated set emit: every packet is its member's own emulated emit, none is foreign"""
    T = 12
    rng = np.random.default_rng(hdr + order)
    segs = mix_segs(rng, MIX4, T)
    keys, tags, cnts, _ = range_ref(MIX4, order, 1, 0, 5, 1)
    ek, et, ec, _, _ = emu_range(MIX4, order, 1, 0, 5, 1, len(tags))
    assert (ec == 1).all()
    pk, res, _ = emu_txset_emit(segs, ek, et, hdr, T + hdr + 3)
    assert check_against_members(segs, ek, et, pk, res, T, hdr) == 0
    assert (res == 0).all()
