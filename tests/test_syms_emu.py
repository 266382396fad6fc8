"""CPU tier of the packets of several symbols (RFC 6330 section 4.4.2; nanorq_amd/csrc/syms_body.h run by syms_emu.cpp): the slot
maps and the count rule against plain restatements, the emulated ingest against ModelRx over the expansion, the emulated emit
against the one-symbol emulation of the expansion and the oracle, and G = 1 against the existing emulations byte for byte."""
import numpy as np
import pytest

import nanorq_amd
import rx_support as R
import syms_support as S
import tx_support as X

MAX_ESI_100 = 2 * 101  # K = 100: K' = 101


# ---- slot maps and count rule ----
@pytest.mark.parametrize("G", [1, 3, 16, 64])
def test_count_rule(G):
    L, K = S.emu_lib(), 100
    for e in (0, 95, 96, 99, 100, MAX_ESI_100):
        assert L.emu_sy_rule(K, e, G) == S.rule(K, e, G), e
    assert L.emu_sy_rule(K, 99, G) == 1 and L.emu_sy_rule(K, 100, G) == G and L.emu_sy_rule(K, 0, G) == min(G, 100)


@pytest.mark.parametrize("G", [1, 3, 16, 64])
def test_range_packetisation_one_block(G):
    L, K = S.emu_lib(), 100
    first, cnt = np.zeros(1, np.uint32), np.zeros(1, np.uint32)
    for esi0 in (0, 1, 90, 99, 100, 101, 130):
        for n in (0, 1, 9, 10, 11, 100 - esi0 if esi0 < 100 else 5, 40, 117):
            want = S.range_packets(K, esi0, n, G)
            assert L.emu_sy_pkt_count(K, esi0, n, G) == len(want), (esi0, n)
            for j, (f, c) in enumerate(want):
                L.emu_sy_range_pkt(K, esi0, n, G, j, X._p(first), X._p(cnt))
                assert (int(first[0]), int(cnt[0])) == (f, c), (esi0, n, j)
                assert 1 <= c <= G and (f + c <= K or f >= K)
                for e in (f, f + c - 1):
                    assert L.emu_sy_range_index(K, esi0, n, G, e) == j, (esi0, n, e)
            # every ESI once
            assert sorted(e for f, c in want for e in range(f, f + c)) == list(range(esi0, esi0 + n))


@pytest.mark.parametrize("interleave", [0, 1])
@pytest.mark.parametrize("G,esi0,nrep", [(5, 0, 7), (16, 0, 0), (3, 0, 10), (64, 0, 3), (1, 0, 4)])
def test_range_maps_two_block_classes(G, esi0, nrep, interleave):
    """an object's table: 2 blocks of K = 11, 3 of K = 10 (each class cut by its own K), both ways"""
    KL, KS, ZL, ZS, T = 11, 10, 2, 3, 16
    Kp = {K: nanorq_amd.params(K)["Kp"] for K in (KL, KS)}
    segs = [(KL, Kp[KL], 0, ZL, None), (KS, Kp[KS], ZL, ZS, None)]
    _, tags, cnt, back = S.emu_emit_table(segs, (0, ZL + ZS, ZL), T, G, False, G * T, rng=(esi0, KL + nrep, KS + nrep, interleave),
                                          maps_only=True)
    w_tags, w_cnt = S.range_list([KL] * ZL + [KS] * ZS, 0, esi0, [KL + nrep] * ZL + [KS + nrep] * ZS, G, interleave)
    assert np.array_equal(tags, w_tags) and np.array_equal(cnt, w_cnt)
    assert np.array_equal(back, np.arange(len(tags)))


@pytest.mark.parametrize("interleave", [0, 1])
@pytest.mark.parametrize("G,esi0,n", [(16, 0, 110), (3, 95, 5), (3, 97, 9), (64, 120, 70), (5, 0, 0), (7, 100, 15)])
def test_range_maps_one_class(G, esi0, n, interleave):
    K, nblk, sbn0, T = 100, 3, 7, 16
    segs = [(K, nanorq_amd.params(K)["Kp"], sbn0, nblk, None)]
    _, tags, cnt, back = S.emu_emit_table(segs, (sbn0, nblk, nblk), T, G, False, G * T, rng=(esi0, n, n, interleave), maps_only=True)
    w_tags, w_cnt = S.range_list([K] * nblk, sbn0, esi0, [n] * nblk, G, interleave)
    assert np.array_equal(tags, w_tags) and np.array_equal(cnt, w_cnt)
    assert np.array_equal(back, np.arange(len(tags)))


# ---- ingest ----
def build_packets(tags, counts, G, T, hdr, stride, salt=0):
    pay = []
    for t, c in zip(tags, counts):
        c = int(c) if 1 <= int(c) <= G else G  # (a malformed packet still has bytes)
        sym = [R.tag(int(t) >> 24, min((int(t) & 0xFFFFFF) + i, 0xFFFFFF)) for i in range(c)]
        pay.append(R.payloads_for(np.array(sym, np.uint32), T, salt).reshape(-1))
    return S.pack(pay, tags, G, T, hdr, stride, fill=0x5A)


def assert_same_books(emu, model):
    for b in range(model.nblk):
        assert np.array_equal(emu.lost(b), model.lost(b)), b
        assert emu.rep_list(b).tolist() == model.reps[b], b
        assert int(emu.gaps[b]) == len(model.missing[b])
        got = set(np.flatnonzero(emu.seen_bits(b)).tolist())
        assert got == model.seen[b], b
    assert np.array_equal(emu.src, model.src) and np.array_equal(emu.rep, model.rep)
    assert (emu.first == 0xFFFFFFFF).all()


@pytest.mark.parametrize("G,T,inline,given", [(4, 16, False, True), (16, 8, True, True), (3, 13, True, False), (64, 4, False, False),
                                              (5, 20, False, True)])
def test_emulated_ingest_matches_model_over_the_expansion(G, T, inline, given):
    K, nblk, sbn0, rep_cap = 100, 3, 2, 12
    Kp = nanorq_amd.params(K)["Kp"]
    max_esi = 2 * Kp
    hdr = 4 if inline else 0
    stride = hdr + G * T + 3
    emu = S.EmuRxSyms(K, T, nblk, rep_cap, sbn0=sbn0, Kp=Kp)
    model = R.ModelRx(K, T, nblk, rep_cap, sbn0=sbn0, Kp=Kp)
    rng = np.random.default_rng(G * 100 + T)
    for call in range(3):
        tags = R.random_stream(rng, K, nblk, sbn0, max_esi, 90, sbn_span=1)
        nsym = rng.integers(1, G + 1, len(tags)).astype(np.uint8)
        if call == 0:  # the edge packets (counts are clipped to G below)
            edge = [(R.tag(sbn0, 10), 4), (R.tag(sbn0, 12), 4),            # overlapping packets
                    (R.tag(sbn0 + 1, 98), 4),                              # crosses K with a given count
                    (R.tag(sbn0 + 1, max_esi - 1), 4),                     # runs past max_esi
                    (R.tag(sbn0 + 2, 0xFFFFFE), 3),                        # runs past 2^24 - 1
                    (R.tag(sbn0, 20), 0), (R.tag(sbn0, 30), G + 1),        # malformed counts
                    (R.tag(sbn0 - 1, 5), 0)]                               # malformed, outside the reception: untouched
            tags = np.concatenate([np.array([e[0] for e in edge], np.uint32), tags])
            nsym = np.concatenate([np.array([min(e[1], G) if e[1] not in (0, G + 1) else e[1] for e in edge], np.uint8), nsym])
        pkts = build_packets(tags, nsym, G, T, hdr, stride, salt=call)
        ns = nsym if given else None
        got = emu.add_syms(pkts, G, tags=None if inline else tags, nsym=ns)
        want = S.model_add(model, pkts, tags, ns, G, hdr, np.full(len(tags) * G, R.UNTOUCHED, np.int32))
        assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
        assert_same_books(emu, model)
        cnt = S.rx_counts(tags, ns, G, lambda sbn: K if sbn0 <= sbn < sbn0 + nblk else None)
        for k in range(len(tags)):  # slots behind the count keep their fill
            lo = max(cnt[k], 1 if cnt[k] == 0 else 0)
            assert (got[k * G + lo:(k + 1) * G] == R.UNTOUCHED).all(), k
    codes = set(got.tolist())
    assert {R.ADDED, R.DUP, R.UNTOUCHED} <= codes


def test_emulated_ingest_full_and_complete_inside_a_packet():
    """rep_cap reached in the middle of a packet (FULL and its duplicates), a block that completes in the middle of a packet
    (ADDED then IGN), and more than one tile of slots"""
    K, T, G, nblk, rep_cap = 100, 8, 4, 2, 6
    Kp = nanorq_amd.params(K)["Kp"]
    emu = S.EmuRxSyms(K, T, nblk, rep_cap, Kp=Kp)
    model = R.ModelRx(K, T, nblk, rep_cap, Kp=Kp)
    tags = [R.tag(0, 100), R.tag(0, 104), R.tag(0, 106), R.tag(0, 105)]  # rows 0..3, 4..5 then FULL FULL, dup of FULL ones
    tags += [R.tag(1, e) for e in range(0, 96, 4)] + [R.tag(1, 98), R.tag(1, 96), R.tag(1, 100)]  # block 1 completes at 99
    tags += [R.tag(0, e) for e in range(0, 100, 4)] * 3  # (over a tile: 4 * 103 slots)
    tags = np.array(tags, np.uint32)
    nsym = np.full(len(tags), G, np.uint8)
    pkts = build_packets(tags, nsym, G, T, 0, G * T)
    got = emu.add_syms(pkts, G, tags=tags, nsym=nsym)
    want = S.model_add(model, pkts, tags, nsym, G, 0, np.full(len(tags) * G, R.UNTOUCHED, np.int32))
    assert np.array_equal(got, want)
    assert got[1 * G:2 * G].tolist() == [R.ADDED, R.ADDED, R.FULL, R.FULL]
    assert got[2 * G:3 * G].tolist() == [R.FULL] * 4
    assert got[3 * G:4 * G].tolist() == [R.DUP, R.FULL, R.FULL, R.FULL]
    k96 = 4 + 24 + 1  # (1, 96): 96 and 97 complete the block, 98 and 99 find it complete
    assert got[k96 * G:(k96 + 1) * G].tolist() == [R.ADDED, R.ADDED, R.IGN, R.IGN]
    assert len(tags) * G > 256
    assert_same_books(emu, model)


# ---- emit ----
def _sender(orc, K, T, nblk, seed, reps):
    Kp = nanorq_amd.params(K)["Kp"]
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 256, (nblk, K * T), dtype=np.uint8)
    blocks = X.oracle_blocks(orc, src, K, T, Kp, [reps] * nblk)
    inter = np.stack([b[0] for b in blocks])
    return Kp, src, blocks, inter


@pytest.mark.parametrize("T,G,inline,pad", [(16, 4, False, 0), (13, 5, True, 3), (48, 3, True, 8), (8, 64, False, 0)])
def test_emulated_emit_matches_expansion_and_oracle(orc, T, G, inline, pad):
    K, nblk, sbn0 = 100, 2, 3
    hi = (1 << 24) - 1
    reps = list(range(K, K + 80)) + list(range(hi - 70, hi + 1))
    Kp, src, blocks, inter = _sender(orc, K, T, nblk, T + G, reps)
    hdr = 4 if inline else 0
    stride = hdr + G * T + pad
    c2 = min(2, G)
    cases = [(R.tag(sbn0, 0), None), (R.tag(sbn0, 96), None),              # the rule: G, and short at K
             (R.tag(sbn0 + 1, 99), None), (R.tag(sbn0 + 1, 100), None),
             (R.tag(sbn0, 50), 1), (R.tag(sbn0, 98), c2), (R.tag(sbn0 + 1, K + 3), G),   # given counts
             (R.tag(sbn0, hi - G + 1), G),                                  # ends exactly at 2^24 - 1
             (R.tag(sbn0, 5), 0), (R.tag(sbn0, 5), G + 1),                  # TX_BAD_RANGE: count 0, above G
             (R.tag(sbn0, 99), 2), (R.tag(sbn0, hi), 2),                    # ... crosses K; passes 2^24 - 1
             (R.tag(sbn0 + 2, 1), 1), (R.tag(sbn0 - 1, 1), 0)]              # foreign (whatever the count)
    tags = np.array([c[0] for c in cases], np.uint32)
    for given in (True, False):
        if given:
            nsym = np.array([S.rule(K, int(t) & 0xFFFFFF, G) if c is None else c for t, (_, c) in zip(tags, cases)], np.uint8)
        else:
            nsym = None
        pk, res = S.emu_emit_table([(K, Kp, sbn0, src, inter)], (sbn0, nblk, nblk), T, G, inline, stride, tags=tags, nsym=nsym)
        want_res, counts = [], []
        for k, (t, c) in enumerate(cases):
            sbn, e = int(t) >> 24, int(t) & 0xFFFFFF
            cc = S.rule(K, e, G) if nsym is None else int(nsym[k])
            if not sbn0 <= sbn < sbn0 + nblk:
                want_res.append(-1)
            elif cc == 0 or cc > G or (nsym is not None and e < K < e + cc) or e + cc - 1 > hi:
                want_res.append(S.BAD_RANGE)
            else:
                want_res.append(0)
            counts.append(cc if want_res[-1] == 0 else 0)
        assert res.tolist() == want_res
        if given:
            assert {0, -1, S.BAD_RANGE} == set(want_res) and want_res.count(S.BAD_RANGE) == 4
        want = S.expanded_emit(K, Kp, T, src, inter, tags, counts, G, inline, stride, sbn0=sbn0)
        assert np.array_equal(pk, want), np.flatnonzero((pk != want).any(1))
        # the oracle, symbol by symbol; guard bytes behind short packets; untouched packets whole
        for k, t in enumerate(tags):
            if counts[k] == 0:
                assert (pk[k] == X.FILL).all(), k
                continue
            b, e = (int(t) >> 24) - sbn0, int(t) & 0xFFFFFF
            if inline:
                assert bytes(pk[k, :4]) == int(t).to_bytes(4, "big")
            for i in range(counts[k]):
                assert np.array_equal(pk[k, hdr + i * T: hdr + (i + 1) * T], X.expected_payload(src, blocks, K, T, b, e + i)), (k, i)
            assert (pk[k, hdr + counts[k] * T:] == X.FILL).all(), k


def test_emulated_emit_not_ready_block(orc):
    K, T, G, nblk = 100, 16, 4, 2
    Kp, src, blocks, inter = _sender(orc, K, T, nblk, 5, list(range(K, K + 8)))
    tags = np.array([R.tag(0, 0), R.tag(1, 0), R.tag(1, K), R.tag(0, K)], np.uint32)
    ready = np.zeros(8, np.uint32)
    ready[0] = 1  # block 0 only
    pk, res = S.emu_emit_table([(K, Kp, 0, src, inter)], (0, nblk, nblk), T, G, True, 4 + G * T, tags=tags, ready=ready)
    assert res.tolist() == [0, -2, -2, 0]
    assert (pk[1] == X.FILL).all() and (pk[2] == X.FILL).all()


@pytest.mark.parametrize("interleave", [0, 1])
def test_emulated_range_equals_its_list(orc, interleave):
    K, T, G, nblk, esi0, n = 100, 16, 16, 2, 90, 42  # (a repair run of two full packets: the rule cuts no repair packet short)
    Kp, src, blocks, inter = _sender(orc, K, T, nblk, 9, list(range(K, K + 32)))
    seg = [(K, Kp, 0, src, inter)]
    pk, tags, cnt, back = S.emu_emit_table(seg, (0, nblk, nblk), T, G, True, 4 + G * T, rng=(esi0, n, n, interleave))
    w_tags, w_cnt = S.range_list([K] * nblk, 0, esi0, [n] * nblk, G, interleave)
    assert np.array_equal(tags, w_tags) and np.array_equal(cnt, w_cnt)
    pk2, res = S.emu_emit_table(seg, (0, nblk, nblk), T, G, True, 4 + G * T, tags=tags, nsym=cnt)
    assert (res == 0).all() and np.array_equal(pk, pk2)
    pk3, res = S.emu_emit_table(seg, (0, nblk, nblk), T, G, True, 4 + G * T, tags=tags)  # the rule gives the same counts
    assert (res == 0).all() and np.array_equal(pk, pk3)


# ---- G = 1 ----
@pytest.mark.parametrize("inline", [False, True])
def test_g1_is_the_one_symbol_emulation(orc, inline):
    K, T, nblk, sbn0 = 100, 13, 2, 1
    Kp = nanorq_amd.params(K)["Kp"]
    rng = np.random.default_rng(11)
    tags = X.random_tags(rng, K, nblk, sbn0, 200)
    reps = sorted({int(t) & 0xFFFFFF for t in tags if (int(t) & 0xFFFFFF) >= K} | set(range(K, K + 10)))
    Kp, src, blocks, inter = _sender(orc, K, T, nblk, 12, reps)
    stride = T + (4 if inline else 0) + 2
    pk1, res1 = X.emu_emit(K, Kp, T, src, inter, tags, inline, stride, sbn0=sbn0)
    pk, res = S.emu_emit_table([(K, Kp, sbn0, src, inter)], (sbn0, nblk, nblk), T, 1, inline, stride, tags=tags)
    assert np.array_equal(pk, pk1) and np.array_equal(res, res1)
    for il in (0, 1):
        pk1, tg1 = X.emu_emit_range(K, Kp, T, src, inter, 95, 15, il, inline, stride, sbn0=sbn0)
        pk, tg, cnt, _ = S.emu_emit_table([(K, Kp, sbn0, src, inter)], (sbn0, nblk, nblk), T, 1, inline, stride, rng=(95, 15, 15, il))
        assert np.array_equal(pk, pk1) and np.array_equal(tg, tg1) and (cnt == 1).all()
    # ingest
    max_esi = 2 * Kp
    a, b = R.EmuRx(K, T, nblk, 8, sbn0=sbn0, Kp=Kp), S.EmuRxSyms(K, T, nblk, 8, sbn0=sbn0, Kp=Kp)
    for call in range(2):
        st = R.random_stream(rng, K, nblk, sbn0, max_esi, 300, sbn_span=1)
        pay = R.payloads_for(st, T, call)
        pkts = R.inline_packets(pay, st, stride) if inline else np.pad(pay, ((0, 0), (0, 3)))
        ra = a.add(pkts, None if inline else st)
        rb = b.add_syms(pkts, 1, tags=None if inline else st)
        assert np.array_equal(ra, rb)
        for name in ("src", "rep", "first", "seen", "gaps", "nrep", "rep_esi", "live"):
            assert np.array_equal(getattr(a, name), getattr(b, name)), name
