"""CPU tier of the reception sets (nrq_rxset_*): the emulated set ingest (nanorq_amd/csrc/rxset_emu.cpp: the bodies of
ingest_set_body.h in kernel order) against one EmuRx (the emulated single-reception ingest) and one ModelRx (the rules, packet by
packet) per member, each fed exactly the packets of its key in packet order.  Bit-exact: codes in their entries, rows, repair
lists in arrival order, counts, seen bits.  The emulation's poison check (pass 5 wrote every dst[] entry pass 6 reads) is an
assertion inside EmuSet.add: it must never trip."""
import numpy as np
import pytest

import nanorq_amd
from rx_support import ADDED, DUP, ERR, FULL, IGN, payloads_for, random_stream
from rxset_support import (MIX4, MIX360, UNKNOWN_KEY, UNTOUCHED, EmuRx, EmuSet, ModelRx, expected_codes, keyed_payloads, keyed_stream,
                           packets, rep_cap_of, tag)

T = 16
CARRIERS = ("arrays", "nokeys", "inline", "keyinline")


def _kps(mix):
    return [nanorq_amd.params(m[1])["Kp"] for m in mix]


def _build(mix, small_cap, obj_key=None, objZ=0, T=T):
    """the set under test, and per member an EmuRx twin and a ModelRx twin"""
    kps = _kps(mix)
    st, mem, twins, models = EmuSet(), [], [], []
    for (key, K, nblk, sbn0), Kp in zip(mix, kps):
        a = (K, T, nblk, rep_cap_of(K, small_cap), sbn0)
        mem.append(EmuRx(*a, Kp=Kp))
        twins.append((key, EmuRx(*a, Kp=Kp)))
        models.append((key, ModelRx(*a, Kp=Kp)))
        st.attach(key, mem[-1], objZ if key == obj_key else 0)
    return kps, st, mem, twins, models


def _same_books(mem, twins, models):
    for m, (_, e), (_, mo) in zip(mem, twins, models):
        assert np.array_equal(m.src, e.src) and np.array_equal(m.rep, e.rep)
        for name in ("seen", "gaps", "nrep", "rep_esi", "first"):
            assert np.array_equal(getattr(m, name), getattr(e, name)), name
        assert (m.first == 0xFFFFFFFF).all()
        assert np.array_equal(m.src, mo.src) and np.array_equal(m.rep, mo.rep)
        for b in range(m.nblk):
            assert np.array_equal(m.lost(b), mo.lost(b)) and list(m.rep_list(b)) == mo.reps[b], b
            assert int(m.gaps[b]) == len(mo.missing[b])


def _one_call(rng, mix, kps, st, twins, models, n, carrier, exact=False, stride_extra=0, objects=(), T=T):
    keys, tags = keyed_stream(rng, mix, kps, n, exact=exact)
    if carrier == "nokeys":
        keys = np.zeros_like(keys)
    pl = keyed_payloads(keys, tags, T)
    pk, k_arg, t_arg, _, kinl = packets(pl, keys, tags, carrier, stride_extra)
    got = st.add(pk, k_arg, t_arg, kinl)
    exp = expected_codes(twins, keys, tags, pl, objects=objects)
    assert np.array_equal(got, exp), np.flatnonzero(got != exp)[:10]
    assert np.array_equal(expected_codes(models, keys, tags, pl, objects=objects), exp)
    return keys, tags, got


@pytest.mark.parametrize("carrier", CARRIERS)
@pytest.mark.parametrize("n", [1, 255, 256, 257, 3000])
def test_set_matches_members_alone(n, carrier):
    """two set calls in a row over the four-member mix, every key / tag carrier, with a small rep_cap on the second half of the
    sizes: FULL and its duplicates"""
    rng = np.random.default_rng(1000 + n)
    kps, st, mem, twins, models = _build(MIX4, small_cap=n in (257, 3000))
    seen_codes = set()
    for call in range(2):
        keys, _, got = _one_call(rng, MIX4, kps, st, twins, models, n, carrier, exact=n < 1000, stride_extra=4 * call)
        _same_books(mem, twins, models)
        seen_codes |= set(np.unique(got).tolist())
        if carrier != "nokeys" and n >= 255:
            assert (got[keys == UNKNOWN_KEY] == UNTOUCHED).all() and (keys == UNKNOWN_KEY).any()
    if n == 3000 and carrier != "nokeys":
        assert seen_codes == {ERR, ADDED, IGN, DUP, FULL, UNTOUCHED}


@pytest.mark.parametrize("carrier", ["arrays", "keyinline"])
def test_set_matches_members_alone_at_t_1040(carrier):
    """T = 1040, where the device's 16-byte copy gives lane 0 alone a second access (tests/test_gpu_rxset.py compares the device
    with this emulation there): the reference itself against the members alone"""
    rng = np.random.default_rng(1040)
    kps, st, mem, twins, models = _build(MIX4, small_cap=False, T=1040)
    _, _, got = _one_call(rng, MIX4, kps, st, twins, models, 300, carrier, exact=True, stride_extra=8, T=1040)
    _same_books(mem, twins, models)
    assert ADDED in got and UNTOUCHED in got


@pytest.mark.parametrize("stride_extra", [0, 4])
def test_inline_key_and_tag_strides(stride_extra):
    """packet = key, FEC Payload ID, payload at +8: strides T + 8 and T + 12"""
    rng = np.random.default_rng(7 + stride_extra)
    kps, st, mem, twins, models = _build(MIX4, small_cap=False)
    keys, tags = keyed_stream(rng, MIX4, kps, 3000)
    pl = keyed_payloads(keys, tags, T)
    pk, k_arg, t_arg, inl, kinl = packets(pl, keys, tags, "keyinline", stride_extra)
    assert pk.shape[1] == T + 8 + stride_extra and k_arg is None and t_arg is None and inl and kinl
    got = st.add(pk, None, None, True)
    assert np.array_equal(got, expected_codes(twins, keys, tags, pl))
    expected_codes(models, keys, tags, pl)
    _same_books(mem, twins, models)


def test_many_packets_and_rep_cap_overflow():
    """about 20000 packets into 14 blocks with two repair rows each: most repair packets find the rows full, and their duplicates
    fold to FULL"""
    rng = np.random.default_rng(20000)
    kps, st, mem, twins, models = _build(MIX4, small_cap=True)
    _, tags, got = _one_call(rng, MIX4, kps, st, twins, models, 20000, "arrays")
    _same_books(mem, twins, models)
    assert (got == FULL).sum() > 100 and all((m.nrep <= m.rep_cap).all() for m in mem)


@pytest.mark.parametrize("n", [257, 20000])
def test_360_blocks(n):
    """six members of 60 blocks: global block numbers, and their LDS counters, beyond 256"""
    rng = np.random.default_rng(360 + n)
    kps, st, mem, twins, models = _build(MIX360, small_cap=True)
    for _ in range(2):
        _one_call(rng, MIX360, kps, st, twins, models, n, "arrays", exact=n < 1000)
        _same_books(mem, twins, models)
    assert sum(int(m.nrep.sum()) for m in mem[3:]) > 0  # (blocks past 256 took repair rows)


def test_object_rule_for_sbn_at_or_above_z():
    """key 5 attached as an object of Z = 8 blocks (its two classes cover SBNs 0..7): its packets with SBN >= Z get ERR above
    max_esi, else IGN; the same SBNs under key 9, a plain reception, stay untouched"""
    rng = np.random.default_rng(58)
    kps, st, mem, twins, models = _build(MIX4, small_cap=False, obj_key=5, objZ=8)
    assert mem[0].max_esi != mem[1].max_esi  # (the emulated classes keep their own max_esi: the rule takes the class it meets)
    keys, tags = keyed_stream(rng, MIX4, kps, 3000)
    extra_t = np.array([tag(8, 3), tag(9, mem[1].max_esi), tag(200, mem[1].max_esi + 1), tag(255, 0xFFFFFF), tag(8, 3), tag(9, 1)], np.uint32)
    extra_k = np.array([5, 5, 5, 5, 9, UNKNOWN_KEY], np.uint32)
    keys, tags = np.concatenate([keys, extra_k]), np.concatenate([tags, extra_t])
    perm = rng.permutation(len(tags))
    keys, tags = keys[perm], tags[perm]
    pl = keyed_payloads(keys, tags, T)
    got = st.add(pl, keys, tags)
    exp = expected_codes(twins, keys, tags, pl)
    high = (keys == 5) & ((tags >> 24) >= 8)
    assert high.sum() >= 4 and (exp[high] == UNTOUCHED).all()
    exp[high] = np.where((tags[high] & 0xFFFFFF) > mem[1].max_esi, ERR, IGN)
    assert np.array_equal(got, exp)
    assert {ERR, IGN} <= set(got[high].tolist())
    expected_codes(models, keys, tags, pl)
    _same_books(mem, twins, models)


def test_candidates_across_a_tile_edge_and_three_members_in_a_wave():
    """300 repair packets, round robin over one block of each of three members: every wave holds candidates of three members, each
    block's candidates straddle the edge between tile 0 and tile 1, and the rows run out (rep_cap 62 < 100 candidates a block)"""
    kps, st, mem, twins, models = _build(MIX4, small_cap=False)
    assert mem[1].rep_cap == 62 and mem[2].rep_cap == 62
    who = [(5, 1, 4, 100), (9, 2, 1, 100), (0, 3, 251, 26)]  # (key, member, SBN, K)
    keys = np.array([who[i % 3][0] for i in range(300)], np.uint32)
    tags = np.array([tag(who[i % 3][2], who[i % 3][3] + i // 3) for i in range(300)], np.uint32)
    assert (tags[2::3] & 0xFFFFFF).max() > mem[3].max_esi  # (the small member's ESIs run past its max_esi: ERR)
    pl = keyed_payloads(keys, tags, T)
    got = st.add(pl, keys, tags)
    exp = expected_codes(twins, keys, tags, pl)
    expected_codes(models, keys, tags, pl)
    assert np.array_equal(got, exp)
    _same_books(mem, twins, models)
    assert int(mem[1].nrep[1]) == 62 and list(mem[1].rep_list(1)) == list(range(100, 162))
    assert (got[0::3] == ADDED).sum() == 62 and (got[0::3] == FULL).sum() == 38 and (got[2::3] == ERR).any()


def test_member_add_between_two_set_calls():
    """a set call, the members' own ingest (the single-reception emulation on the same arrays), a set call: one set of books"""
    rng = np.random.default_rng(99)
    kps, st, mem, twins, models = _build(MIX4, small_cap=False)
    _one_call(rng, MIX4, kps, st, twins, models, 1500, "arrays")
    for i, ((key, K, nblk, sbn0), Kp) in enumerate(zip(MIX4, kps)):
        t = random_stream(rng, K, nblk, sbn0, 2 * Kp, 200, sbn_span=1)
        p = payloads_for(t, T, salt=3)
        r = mem[i].add(p, t)
        assert np.array_equal(r, twins[i][1].add(p, t)) and np.array_equal(r, models[i][1].add(p, t))
    _same_books(mem, twins, models)
    _one_call(rng, MIX4, kps, st, twins, models, 1500, "inline")
    _same_books(mem, twins, models)


def test_empty_calls():
    kps, st, mem, twins, models = _build(MIX4, small_cap=False)
    assert len(st.add(np.zeros((0, T), np.uint8), np.zeros(0, np.uint32), np.zeros(0, np.uint32))) == 0
    res = EmuSet().add(np.zeros((3, T), np.uint8), np.zeros(3, np.uint32), np.zeros(3, np.uint32))
    assert (res == UNTOUCHED).all()
    _same_books(mem, twins, models)
