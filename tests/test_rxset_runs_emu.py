"""CPU tier of a reception set's want and held listings as runs (nrq_rxset_want_syms / nrq_rxset_held_syms) and of a sender set's
held emit of packets of several symbols (NRQ_TX_HELD in nrq_txset_emit_syms), through rxset_runs_emu.cpp over runs_set_body.h.
The reference of a listing is the packetisation of include/nanorq_hip.h (runs_support.packetise) of the one-symbol set listing
(rxset_want_support.emu_list, itself pinned against a numpy model in test_rxset_want_emu.py) with each block's own member's K; the
reference of an emit is the header's result table per member and the one-symbol held set emit's bytes.  Every comparison is exact.
The emulation is handed bitmaps with poison words behind them and outputs with guards behind them."""
import numpy as np
import pytest

import runs_support as U
import rxset_runs_support as RR
from rx_support import EmuRx, payloads_for, tag
from rxset_want_support import QUERIES, emu_list
from test_rxset_want_emu import _filled
from tx_support import FILL
from want_support import BIG, CASE_NAMES, NBLK, SBN0, WANT_SOURCE, case as case_of

T = 16
CAPS = [(m // 4, 10, 16, 16 * (m % 4)) for m in range(64)]  # both caps at once: 64 members, 1024 blocks (test_gpu_rxset_want.CAPS)
HI = RR.HI


def _check(members, G, queries=QUERIES, held=True):
    """every query and the held listing of a set at G against the reference -> {query or "held": Listing}"""
    out = {}
    for what, q in [("want", q) for q in queries] + ([("held", None)] if held else []):
        if what == "want":
            source, extra, esi_from = q
            args = (WANT_SOURCE if source else 0, extra, esi_from)
        else:
            args = ()
        rc, n, one_cnt, one_keys, one_tags = emu_list(members, what, *args)
        assert rc == 0
        ref = RR.reference(members, one_keys, one_tags, one_cnt, G)
        got = RR.emu_list_syms(members, what, G, *args)
        assert got.rc == 0, (what, q, G)
        RR.check_listing((got.keys, got.tags, got.ns, got.cnt, got.npkt, got.nsym), ref, one_tags, G)
        out[q if what == "want" else "held"] = got
    return out


# ------------------------------------------------------------------------------------------------------------- listings ----
_CASE_SET = []


def _case_set():
    """every reception of want_support.CASE_NAMES (the "rounds" cases among them, at T = 4) as a member of ONE set: K, max_esi and
    rep_cap all differ, the keys' order is not the list's, and the members are handed over in reverse table order"""
    if not _CASE_SET:
        for i, name in enumerate(CASE_NAMES):
            c = case_of(name)
            e = EmuRx(c.K, 4, NBLK, c.rep_cap, sbn0=SBN0, max_esi=c.max_esi, Kp=c.Kp)
            for part in np.array_split(c.stream, 2):
                e.add(payloads_for(part, 4), tags=part)
            _CASE_SET.append((1000 - 7 * i, e, 0))
        _CASE_SET.sort(key=lambda m: -m[0])
    return _CASE_SET


@pytest.mark.parametrize("G", U.GS)
def test_the_single_cases_as_members_of_different_K(G):
    """a packet's source / repair split follows its own member's K: K = 10, 31, 32, 33, 8200 side by side"""
    mem = _case_set()
    assert len({e.K for _, e, _ in mem}) >= 5 and [m[0] for m in mem] == sorted((m[0] for m in mem), reverse=True)
    out = _check(mem, G)
    assert all(out[q].npkt > 0 for q in QUERIES) and out["held"].npkt > 0
    if G > 1:
        assert any(out[q].npkt < out[q].nsym for q in QUERIES)


def test_packets_across_a_word_and_across_a_round():
    """the "rounds" member among small ones: K = 8200 takes 257 seen words, two rounds of the walk"""
    mem = _case_set()
    key = next(k for k, e, _ in mem if e.K == 8200 and e.rep_cap == 4)
    got = RR.emu_list_syms(mem, "want", 5, WANT_SOURCE)
    mine = got.keys == key
    pk = {int(t): int(c) for t, c in zip(got.tags[mine], got.ns[mine])}
    b1 = (SBN0 + 1) << 24  # one run of 8200: the packet of ESI 8190 straddles the round (8192 % 5 = 2)
    assert pk[b1 | 8190] == 5 and pk[b1 | 8195] == 5 and (b1 | 8192) not in pk and sum(1 for t in pk if t >> 24 == SBN0 + 1) == 1640
    b0 = SBN0 << 24  # runs of two: (31, 32) straddles a word, (8191, 8192) the round
    assert pk[b0 | 31] == 2 and (b0 | 32) not in pk and pk[b0 | 8191] == 2 and (b0 | 8192) not in pk
    assert not (got.keys[~mine] == key).any() and len(set(got.keys.tolist())) > 3


@pytest.mark.parametrize("G", U.GS)
def test_one_span_under_two_keys_and_an_object_of_two_classes(G):
    mem = _filled([(1, 10, 3, 0), (2, 10, 3, 0), (4, 26, 2, 6), (4, 26, 2, 0)], False, seed=3, n=500)
    out = _check(mem, G)
    src = out[(True, 0, 0)]
    assert not np.array_equal(src.tags[src.keys == 1], src.tags[src.keys == 2]) and (src.keys == 1).any() and (src.keys == 2).any()
    # an object of Z = 5 blocks: ZL = 2 blocks of K = 12, then ZS = 3 blocks of K = 10, under one key, beside a plain reception
    mem = _filled([(8, 12, 2, 0), (8, 10, 3, 2), (3, 10, 2, 0)], False, seed=9, n=400, objZ={8: 5})
    out = _check(mem, G)
    held = out["held"]
    assert len(held.cnt) == 7 and held.cnt[2:4].any() and held.cnt[4:].any()
    if G >= 16:  # no source packet reaches its class's K: 12 in blocks of SBN 0, 1 and 10 in those of SBN 2 .. 4
        ob = held.keys == 8
        e, c, sbn = held.tags[ob] & HI, held.ns[ob].astype(np.int64), held.tags[ob] >> 24
        K = np.where(sbn < 2, 12, 10)
        assert ((e >= K) | (e + c <= K)).all() and ((e < K) & (e + c == K)).any()


@pytest.mark.parametrize("G", (1, 5, 64))
def test_a_member_that_lists_nothing_between_two_that_do(G):
    """equal offsets in the middle of the scan: the middle member's blocks are complete (want) or untouched (held)"""
    def member(key, state):
        e = EmuRx(10, T, 2, 6, sbn0=key, Kp=10)
        if state == "partial":
            tg = np.array([tag(key + b, x) for b in range(2) for x in (0, 1, 2, 5, 6, 9, 12, 13, 11)], np.uint32)
            e.add(payloads_for(tg, T), tags=tg)
        elif state == "complete":
            for b in range(2):
                e.mark_complete(b)
        return (key, e, 0)
    for middle, what in (("complete", (True, 0, 0)), ("untouched", "held")):
        mem = [member(3, "partial"), member(2, middle), member(1, "partial")]
        got = _check(mem, G)[what]
        assert list(got.cnt[2:4]) == [0, 0] and got.cnt[:2].all() and got.cnt[4:].all() and not (got.keys == 2).any()


@pytest.mark.parametrize("G", U.GS)
def test_the_reception_whose_repair_runs_cross_a_round_of_rows(G):
    emu, _ = U.r600_filled()
    small = EmuRx(10, T, 2, 6, sbn0=0, Kp=10)
    tg = np.array([tag(b, x) for b in range(2) for x in (3, 4, 5, 10, 11)], np.uint32)
    small.add(payloads_for(tg, T), tags=tg)
    mem = [(9, small, 0), (5, emu, 0), (2, small, 0)]  # (the same small books under two keys around it)
    got = _check(mem, G, queries=[(False, 2, 0)])["held"]
    if G == 5:
        s0, mine = U.R600["sbn0"], got.keys == 5
        pk = [(int(t) >> 24, int(t) & HI, int(c)) for t, c in zip(got.tags[mine], got.ns[mine])]
        assert pk[:106] == [(s0, 10 + 5 * j, 5) for j in range(106)]       # one run of 530 rows: row 256 is inside a packet
        assert pk[106:636] == [(s0 + 1, e, 1) for e in range(539, 9, -1)]  # descending arrival: all counts 1
        assert pk[636:] == [(s0 + 2, 0, 5), (s0 + 2, 5, 4), (s0 + 2, 10, 3)]  # nothing joins K - 1 to K
        assert list(got.cnt) == [2, 2, 106, 530, 3, 2, 2]


_CAPS = []


@pytest.mark.parametrize("G", U.GS)
def test_both_caps(G):
    """1024 blocks of K = 10 over 64 members: the scan takes 1025 entries, the symbol total a word behind them"""
    if not _CAPS:
        _CAPS.extend(_filled(CAPS, False, seed=5, n=24000))
    out = _check(_CAPS, G, queries=[(True, 0, 0), (False, 2, 0)])
    assert len(out["held"].cnt) == 1024 and (out[(False, 2, 0)].cnt > 0).sum() > 200


def test_an_empty_set_and_a_set_that_lists_nothing():
    for what in ("want", "held"):
        got = RR.emu_list_syms([], what, 5, cap=3)
        assert got.rc == 0 and got.npkt == 0 and got.nsym == 0 and len(got.cnt) == 0 and (got.tags == RR.GUARD).all() and (got.keys == RR.GUARD).all()
    mem = [(k, EmuRx(10, T, 2, 4, sbn0=s, Kp=10), 0) for k, s in ((2, 0), (1, 4))]
    got = RR.emu_list_syms(mem, "held", 5, cap=3)
    assert got.rc == 0 and got.npkt == 0 and not got.cnt.any() and (got.tags == RR.GUARD).all() and (got.ns == RR.GUARD_B).all()
    for _, e, _ in mem:
        for b in range(e.nblk):
            e.mark_complete(b)
    got = RR.emu_list_syms(mem, "want", 5, cap=3)
    assert got.rc == 0 and got.npkt == 0 and not got.cnt.any() and (got.tags == RR.GUARD).all()
    got = RR.emu_list_syms(mem, "held", 4)  # (held: all K of every block, in packets of 4, 4, 2)
    assert list(got.cnt) == [3] * 4 and got.nsym == 40 and list(got.ns[:3]) == [4, 4, 2]


# ------------------------------------------------------------------------------------------------------- listing rules ----
def test_listing_rules():
    from rxset_support import MIX4
    mem = _filled(MIX4, False, seed=21, n=1500)
    G = 5
    for what, args in (("want", (0, 2, 0)), ("held", ())):
        rc, n1, one_cnt, one_keys, one_tags = emu_list(mem, what, *args)
        rk, rt, rn, rcnt = RR.reference(mem, one_keys, one_tags, one_cnt, G)
        n = len(rt)
        assert n > 8 and n < len(one_tags)
        lst = lambda **kw: RR.emu_list_syms(mem, what, G, *args, **kw)
        got = lst(count_only=True)                                         # both lists NULL: the totals and the counts
        assert (got.rc, got.npkt, got.nsym) == (0, n, len(one_tags)) and np.array_equal(got.cnt, rcnt)
        got = lst(cap=n)                                                   # exactly enough room
        assert got.rc == 0 and np.array_equal(got.tags, rt) and np.array_equal(got.ns, rn) and np.array_equal(got.keys, rk)
        got = lst(cap=n - 1)                                               # one short: refused, totals and counts filled,
        assert got.rc == -1 and (got.npkt, got.nsym) == (n, len(one_tags)) and np.array_equal(got.cnt, rcnt)
        assert (got.tags == RR.GUARD).all() and (got.keys == RR.GUARD).all() and (got.ns == RR.GUARD_B).all()   # nothing written
        got = lst(cap=n + 3)
        assert got.rc == 0 and np.array_equal(got.tags[:n], rt) and (got.tags[n:] == RR.GUARD).all() and (got.ns[n:] == RR.GUARD_B).all()
        assert (got.keys[n:] == RR.GUARD).all()
        got = lst(with_keys=False)                                         # d_keys NULL: tags and counts alone
        assert got.rc == 0 and got.keys is None and np.array_equal(got.tags, rt) and np.array_equal(got.ns, rn)
        # refused: exactly one of the two lists, keys without tags, no packet total, G outside 1 .. 64
        for kw in (dict(give=("tags",)), dict(give=("nsym",)), dict(give=())):
            got = lst(**kw)
            assert got.rc == -1 and (got.npkt, got.nsym) == (0, 0), kw
            assert (got.tags == RR.GUARD).all() and (got.keys == RR.GUARD).all() and (got.ns == RR.GUARD_B).all() and (got.cnt == RR.GUARD).all()
        assert lst(no_npkt=True).rc == -1
        for bad_G in (0, 65):
            got = RR.emu_list_syms(mem, what, bad_G, *args)
            assert got.rc == -1 and got.npkt == 0 and (got.cnt == RR.GUARD).all()
    for flags, extra, esi_from in ((2, 0, 0), (3, 0, 0), (0x80000000, 0, 0), (WANT_SOURCE, 1, 0), (WANT_SOURCE, 0, 1), (0, BIG + 1, 0)):
        got = RR.emu_list_syms(mem, "want", G, flags, extra, esi_from)      # what nrq_rxset_want refuses
        assert got.rc == -1 and got.npkt == 0 and (got.cnt == RR.GUARD).all(), (flags, extra, esi_from)
    assert RR.emu_list_syms(mem, "want", G, 0, BIG, 0).rc == 0


# ------------------------------------------------------------------------------------------------------- held set emit ----
@pytest.mark.parametrize("G", U.GS)
@pytest.mark.parametrize("T_,hdr,kind,path", RR.PATH_ROWS, ids=[r[3] for r in RR.PATH_ROWS])
def test_held_set_emit(T_, hdr, kind, path, G):
    """a relay in three states, a plain sender and an object's relay of two classes under three keys, their packets interleaved:
    the header's result table per member, the one-symbol held set emit's bytes, the fill everywhere else"""
    m = RR.Mixed(T_, G)
    b2 = m.emu.rep_esi[2 * m.emu.rep_cap:3 * m.emu.rep_cap].tolist()
    assert b2.index(U.K3 + 5) >= 64 and m.emu.nrep[2] <= m.emu.rep_cap      # block 2's held runs lie beyond row 64 of its list
    keys, tags, counts = m.packets()
    stride = RR.stride_of(T_, G, hdr, kind)
    import syms_set_support as SS
    rows = [(0, s.src.shape[1]) for s in m.segs] + [(0, s.inter.shape[1] * T_) for s in m.segs] + [(0, m.emu.rep_cap * T_), (0, 12 * T_)]
    assert SS.emit_path(0, stride, T_, hdr, rows) == path
    for given in (True, False):
        if given:
            cnts, nsym = counts, counts
        else:  # the sender's rule, with the K of each packet's own segment
            ks, ts, ns = SS.case_arrays(m.segs, [(int(k), int(t), None) for k, t in zip(keys, tags)], G, True)
            cnts, nsym = ns, None
        pk, res, order = RR.emu_txset_emit_held_syms(m.segs, keys, tags, nsym, G, hdr, stride)
        want_res = m.results(keys, tags, cnts)
        assert np.array_equal(res, want_res), (given, np.flatnonzero(res != want_res)[:8])
        if given:
            for key in (RR.KEY_R, RR.KEY_O):
                assert {0, RR.NOT_READY, RR.BAD_RANGE, RR.FOREIGN} == set(res[keys == key].tolist()), key
            assert RR.NOT_READY not in res[keys == RR.KEY_S] and (res[keys == RR.KEY_NONE] == RR.FOREIGN).all()
            segs_of = {k: [i for i, s in enumerate(m.segs) if s.key == k] for k in (RR.KEY_R, RR.KEY_S, RR.KEY_O)}
            assert len({tuple(v) for v in segs_of.values()}) == 3 and len(segs_of[RR.KEY_O]) == 2
        want = m.expected(keys, tags, cnts, res, hdr, stride)
        bad = np.flatnonzero((pk != want).any(1))
        assert len(bad) == 0, (given, bad[:8], keys[bad[:8]], tags[bad[:8]])
        assert (pk[res != 0] == FILL).all()
    # the plain sender answers as without the flag: the several-symbol set emit's own emulation over the same table
    pk0, res0, _ = SS.emu_txset_emit_syms(m.segs, keys, tags, counts, G, hdr, stride)
    pk, res, _ = RR.emu_txset_emit_held_syms(m.segs, keys, tags, counts, G, hdr, stride)
    snd = (keys == RR.KEY_S) | (keys == RR.KEY_NONE)
    assert np.array_equal(res[snd], res0[snd]) and np.array_equal(pk[snd], pk0[snd]) and (res0[snd] == 0).any()
    rdy = (keys == RR.KEY_R) & ((tags >> 24) == U.S3) & (res != RR.BAD_RANGE)   # ... and so does a relay's ready block
    assert np.array_equal(res[rdy], res0[rdy]) and np.array_equal(pk[rdy], pk0[rdy]) and rdy.any()


# ------------------------------------------------------------------------------- the seed of the GPU tier's loop ----
def test_the_loop_seed_stays_within_one_round_by_the_host_planner():
    """tests/test_gpu_rxset_runs.py bounds its want_syms -> emit_syms -> add_syms -> decode loop by 3 rounds; its losses (LOOP,
    LOOP_LOSS, LOOP_SEED) are chosen so that the host planner alone solves every block from exactly its gaps' worth of repair
    symbols: one round, two to spare"""
    assert RR.oracle_rounds(RR.LOOP_SEED) == 1
    assert sum(len(v) > 0 for v in RR.loop_losses(RR.LOOP_SEED).values()) >= 10
