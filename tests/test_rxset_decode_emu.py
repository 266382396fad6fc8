"""CPU tier of a reception set's counts, lists and decode grouping: the emulated listing passes (nanorq_amd/csrc/rxset_lists_emu.cpp:
the bodies of lists_set_body.h in the kernels' order and rounds) against a numpy model written from the header's words and
against each member's own books, and rxset_plan.h's grouping against its rules evaluated in numpy."""
import numpy as np
import pytest

import nanorq_amd
from rxset_decode_support import CHUNK, NONE, block_order, emu_lists, model_block_list, plan, selected
from rxset_support import MIX4, MIX360, EmuRx, EmuSet, keyed_payloads, keyed_stream, rep_cap_of

T = 16


def _filled(mix, small_cap, seed, n):
    """EmuRx members of a mix, filled through the emulated set ingest with a keyed stream"""
    kps = [nanorq_amd.params(m[1])["Kp"] for m in mix]
    st, mem = EmuSet(), []
    for (key, K, nblk, sbn0), Kp in zip(mix, kps):
        mem.append((key, EmuRx(K, T, nblk, rep_cap_of(K, small_cap), sbn0, Kp=Kp), 0))
        st.attach(key, mem[-1][1])
    rng = np.random.default_rng(seed)
    keys, tags = keyed_stream(rng, mix, kps, n)
    st.add(keyed_payloads(keys, tags, T), keys, tags)
    return mem


def _check(mem):
    """the emulated listing of `mem` against the model, block for block; returns (gaps, nrep, offsets)"""
    keys, sbns, (c_gaps, c_nrep), gaps, off, words = emu_lists(mem)
    order = block_order([(k, e) for k, e, _ in mem])
    nb = len(order)
    assert len(keys) == nb and off[0] == 0 if nb else len(words) == 0
    at = 0
    for j, (key, e, b) in enumerate(order):
        assert (keys[j], sbns[j]) == (key, e.sbn0 + b)
        exp = model_block_list(e, b)
        assert c_gaps[j] == gaps[j] == e.gaps[b] and c_nrep[j] == e.nrep[b]
        assert off[j] == at, j                                    # exclusive offsets
        got = words[at:at + len(exp)]
        assert np.array_equal(got, exp), (j, key, b)
        # the member's own books (the single-reception emulation's view of them)
        assert np.array_equal(got[:int(e.nrep[b])], e.rep_list(b)) and np.array_equal(got[int(e.nrep[b]):], e.lost(b))
        assert len(exp) == int(e.gaps[b]) + int(e.nrep[b])
        at += len(exp)
    assert off[nb] == at == len(words)                            # the total
    return gaps, c_nrep, off


@pytest.mark.parametrize("small_cap", [True, False])
@pytest.mark.parametrize("mix,n", [(MIX4, 1500), (MIX360, 20000)], ids=["mix4", "mix360"])
def test_lists_match_the_model(mix, n, small_cap):
    """K = 10 (one partial word), 26, 100; 360 blocks (more than one 256-thread count launch, a scan over 361 entries); rows that
    overflow (small_cap) and rows that do not"""
    mem = _filled(mix, small_cap, seed=7 + n + small_cap, n=n)
    gaps, nrep, off = _check(mem)
    assert gaps.any() and nrep.any()
    if small_cap:
        assert (nrep == 2).any()                                  # (rep_cap reached: FULL during the ingest)
    if mix is MIX360:
        assert len(gaps) == 360 and off[360] == int(gaps.sum()) + int(nrep.sum())


def test_many_rounds_and_the_extremes():
    """K = 8200: 257 seen words, two rounds of 256, the last word partial (set directly: filling it by ingest is slow); beside it a
    block with nothing missing, a block with everything missing, and a one-block K = 10 member in front and behind"""
    K = 8200
    Kp = nanorq_amd.params(K)["Kp"]
    big = EmuRx(K, T, 3, 5, sbn0=4, Kp=Kp)
    rng = np.random.default_rng(11)
    bits = rng.random(K) < 0.7
    for b, have in enumerate((bits, np.ones(K, bool), np.zeros(K, bool))):
        full = np.zeros(big.bm_words * 32, np.uint8)
        full[:K] = have
        full[K:big.m1] = rng.random(big.m1 - K) < 0.5                # seen repair ESIs: bits at and above K must not be listed
        big.seen[b * big.bm_words:(b + 1) * big.bm_words] = np.packbits(full, bitorder="little").view(np.uint32)
        big.gaps[b] = K - int(have.sum())
        big.nrep[b] = (3, 0, 5)[b]
        big.rep_esi[b * 5:b * 5 + 5] = K + 10 * b + np.arange(5)
    small = [EmuRx(10, T, 1, 2, sbn0=s, Kp=10) for s in (0, 9)]
    small[0].seen[0] = 0b1111111111 | (1 << 12)
    small[0].gaps[0] = 0
    mem = [(9, small[1], 0), (3, big, 0), (1, small[0], 0)]
    gaps, nrep, off = _check(mem)
    assert list(gaps) == [0, K - int(bits.sum()), 0, K, 10] and list(nrep) == [0, 3, 0, 5, 0]


def test_empty_set():
    keys, sbns, (g, r), gaps, off, words = emu_lists([])
    assert len(keys) == len(g) == len(gaps) == len(words) == 0 and list(off) == [0]


PAIRS = [(10, 10), (26, 30), (100, 101)]  # (K, K'): three groups, one of them with a larger K'


@pytest.mark.parametrize("seed", range(6))
def test_groups(seed):
    """random block tables over members of three (K, K') pairs, with and without a relay, up to 1024 blocks"""
    rng = np.random.default_rng(seed)
    mem, member = [], []
    if seed == 0:      # the caps: 64 members, 1024 blocks
        sizes = [16] * 64
    elif seed == 1:    # one group of 720 blocks: cut into chunks
        sizes = [120] * 6
    else:
        sizes, left = [], 1024
        for _ in range(int(rng.integers(3, 65))):
            if left == 0:
                break
            sizes.append(int(rng.integers(1, min(60, left) + 1)))
            left -= sizes[-1]
    for m, nblk in enumerate(sizes):
        K, Kp = PAIRS[0] if seed == 1 else PAIRS[int(rng.integers(0, 3))]
        relay = 0 if seed == 1 else int(rng.random() < 0.4)
        mem.append((K, Kp, K + 3 if rng.random() < 0.3 else 2 * Kp, relay))
        member += [m] * nblk
    member = np.array(member, np.uint32)
    nb = len(member)
    assert nb <= 1024
    K = np.array([mem[m][0] for m in member], np.int64)
    max_esi = np.array([mem[m][2] for m in member], np.int64)
    ng = rng.integers(0, K + 1)
    # edge values: nr == ng, nr - ng == max_esi - K and one above it, ng == 0, one below ng
    kind = rng.integers(0, 6, nb)
    nr = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4], [ng, ng + max_esi - K, ng + max_esi - K + 1, ng + 2, np.maximum(ng, 1) - 1],
                   rng.integers(0, K + 12))
    ng[kind == 5] = 0
    chunk_of, pos_of, chunks = plan(mem, member, ng, nr)
    sel = selected(ng, nr, K, max_esi)
    assert np.array_equal(chunk_of != NONE, sel)                    # the selection is the three-clause rule; every selected block once
    for k in range(5):
        assert (kind == k).any()
    assert sel.any() and (~sel).any()
    key_of = lambda j: (mem[member[j]][0], mem[member[j]][1], mem[member[j]][3])
    first_seen = []
    for c, (cK, cKp, crel, cn) in enumerate(chunks):
        blocks = np.flatnonzero(chunk_of == c)
        assert len(blocks) == cn and 1 <= cn <= CHUNK                # no chunk beyond 256 blocks
        assert all(key_of(j) == (cK, cKp, crel) for j in blocks)     # no chunk mixes (K, K', has_relay)
        assert np.array_equal(pos_of[blocks], np.arange(cn))         # ascending inside the chunk (flatnonzero is ascending)
        if (cK, cKp, crel) not in first_seen:
            first_seen.append((cK, cKp, crel))
        else:                                                        # a group's chunks follow each other, full ones first, in block order
            assert first_seen[-1] == (cK, cKp, crel) and chunks[c - 1][3] == CHUNK
            assert blocks[0] > np.flatnonzero(chunk_of == c - 1)[-1]
    # groups in first-appearance order of block order
    exp_order = []
    for j in np.flatnonzero(sel):
        if key_of(j) not in exp_order:
            exp_order.append(key_of(j))
    assert first_seen == exp_order
    counts = {g: sum(1 for j in np.flatnonzero(sel) if key_of(j) == g) for g in exp_order}
    assert len(chunks) == sum((n + CHUNK - 1) // CHUNK for n in counts.values())
    if seed == 1:
        assert len(exp_order) == 1 and (len(chunks) > 1) == (int(sel.sum()) > CHUNK)
