"""CPU tier of the sets' packets of several symbols (nanorq_amd/csrc/syms_set_body.h run by syms_set_emu.cpp): the emulated set
ingest against each member's own emulated add_syms over the packets of its key and against ModelRx over their expansion; the
emulated set emit against each member's own emulated emit_syms, packet by packet, in the three header forms; and G = 1 against
the one-symbol set emulations byte for byte."""
import numpy as np
import pytest

import nanorq_amd
import rx_support as R
import rxset_support as RS
import syms_set_support as SS
import syms_support as S
import txset_support as XS

BOOKS = ("src", "rep", "first", "seen", "gaps", "nrep", "rep_esi", "live")


def _members(T):
    """the shared members three times over: in the emulated set, as emulated twins fed alone, as models"""
    eset, twins, models = SS.EmuSetSyms(), {}, {}
    for spec in SS.MEMBERS:
        name, key, _, _, _, objZ, _ = spec
        p = SS.member_params(spec)
        mk = lambda cls: cls(p["K"], T, p["nblk"], p["rep_cap"], sbn0=p["sbn0"], max_esi=p["max_esi"], Kp=p["Kp"])
        e = mk(S.EmuRxSyms)
        eset.attach(key, e, objZ)
        twins[name], models[name] = mk(S.EmuRxSyms), mk(R.ModelRx)
    return eset, twins, models


def _merge(exp, sel, G, r):
    """a member's codes over its key's packets into the set's slots; no slot is claimed twice"""
    slots = (sel[:, None] * G + np.arange(G)[None, :]).reshape(-1)
    hit = r != R.UNTOUCHED
    assert (exp[slots[hit]] == R.UNTOUCHED).all()
    exp[slots[hit]] = r[hit]


# (G, T, hdr, counts given): every header form; G = 3: a packet whose slots straddle the tile edge 255..257
@pytest.mark.parametrize("G,T,hdr,given", [(3, 13, 8, True), (4, 16, 0, True), (16, 8, 4, True), (5, 20, 8, False), (64, 4, 4, False),
                                           (3, 16, 0, False)])
def test_emulated_set_ingest_matches_members_and_model(G, T, hdr, given):
    eset, twins, models = _members(T)
    stride = hdr + G * T + 3
    seen_codes = set()
    for call, (keys, tags, nsym) in enumerate(SS.ingest_calls(G, T, given)):
        counts = nsym if nsym is not None else np.full(len(tags), G, np.uint8)
        pkts = SS.build_packets(keys, tags, counts, G, T, hdr, stride, salt=call)
        got = eset.add_syms(pkts, G, key_inline=hdr == 8, nsym=nsym, **SS.carrier(keys, tags, hdr))
        exp_twin = np.full(len(tags) * G, R.UNTOUCHED, np.int32)
        exp_model = exp_twin.copy()
        for (name, key, _, _, _, _, _), (_, e, _) in zip(SS.MEMBERS, eset.members):
            sel = np.flatnonzero(keys == key)
            ns = None if nsym is None else nsym[sel]
            view, inline = SS.member_view(pkts, sel, hdr)
            _merge(exp_twin, sel, G, twins[name].add_syms(view, G, tags=None if inline else tags[sel], nsym=ns))
            mhdr = 4 if inline else 0
            _merge(exp_model, sel, G, S.model_add(models[name], view, tags[sel], ns, G, mhdr, np.full(len(sel) * G, R.UNTOUCHED, np.int32)))
            for a in BOOKS[:-1]:  # the same rows, repair list in slot order, counts and seen bits (live: slot indices of the call)
                assert np.array_equal(getattr(e, a), getattr(twins[name], a)), (name, a)
            m = models[name]
            for b in range(m.nblk):
                assert np.array_equal(e.lost(b), m.lost(b)) and e.rep_list(b).tolist() == m.reps[b], (name, b)
            assert np.array_equal(e.src, m.src) and np.array_equal(e.rep, m.rep)
        SS.foreign_codes(keys, tags, nsym, G, exp_twin)
        SS.foreign_codes(keys, tags, nsym, G, exp_model)
        assert np.array_equal(got, exp_twin), np.flatnonzero(got != exp_twin)[:10]
        assert np.array_equal(got, exp_model), np.flatnonzero(got != exp_model)[:10]
        unknown = np.flatnonzero(keys == SS.UNKNOWN_KEY)
        assert (got.reshape(-1, G)[unknown] == R.UNTOUCHED).all()  # a packet of no member: every slot untouched
        seen_codes |= set(got.tolist())
        if call == 0 and G == 3:
            assert got[255:258].tolist() == [R.ADDED] * 3  # the packet across the tile edge
    assert {R.ADDED, R.DUP, R.IGN, R.ERR, R.FULL, R.UNTOUCHED} <= seen_codes


@pytest.mark.parametrize("carrier", ["arrays", "nokeys", "inline", "keyinline"])
def test_g1_ingest_is_the_one_symbol_set(carrier):
    T, small = 12, True
    rng = np.random.default_rng(7)
    kps = [nanorq_amd.params(K)["Kp"] for _, K, _, _ in RS.MIX4]
    a, b = RS.EmuSet(), SS.EmuSetSyms()
    for (key, K, nblk, sbn0), Kp in zip(RS.MIX4, kps):
        if carrier == "nokeys":
            key = 0
        for s in (a, b):
            s.attach(key, S.EmuRxSyms(K, T, nblk, RS.rep_cap_of(K, small), sbn0=sbn0, Kp=Kp))
        if carrier == "nokeys":
            break
    for call in range(2):
        keys, tags = RS.keyed_stream(rng, RS.MIX4, kps, 400)
        pk, ks, tg, inline, kinl = RS.packets(RS.keyed_payloads(keys, tags, T), keys, tags, carrier, stride_extra=2)
        ra = a.add(pk, keys=ks, tags=tg, key_inline=kinl)
        rb = b.add_syms(pk, 1, keys=ks, tags=tg, key_inline=kinl)
        assert np.array_equal(ra, rb)
        for (_, ea, _), (_, eb, _) in zip(a.members, b.members):
            for name in BOOKS:
                assert np.array_equal(getattr(ea, name), getattr(eb, name)), name


def _segs(rng, T):
    """two senders with the same SBN span under different keys, one key with two spans, a sender with a block that is not ready
    (what a relay's segment looks like to the emit), an object of two block classes"""
    mix = [(5, 100, 2, 0), (9, 100, 2, 0), (5, 10, 2, 4), (11, 26, 2, 250), (SS.OBJ_KEY, 103, 1, 0), (SS.OBJ_KEY, 102, 2, 1)]
    segs = XS.mix_segs(rng, mix, T)
    segs[3].ready = np.array([True, False])
    return segs


@pytest.mark.parametrize("T,G,hdr,pad", [(16, 4, 8, 0), (13, 5, 4, 3), (48, 3, 8, 8), (8, 64, 0, 0), (20, 4, 0, 4), (16, 16, 4, 12)])
def test_emulated_set_emit_matches_members(T, G, hdr, pad):
    rng = np.random.default_rng(T * 10 + G)
    segs = _segs(rng, T)
    stride = hdr + G * T + pad
    cases = SS.emit_cases(segs, G, rng)
    cases += [(SS.OBJ_KEY, R.tag(SS.OBJ_Z, 1), 1), (11, R.tag(251, 0), None), (11, R.tag(251, 30), 2)]  # SBN >= Z; not ready
    across_K = [i for i, c in enumerate(cases) if c == (5, R.tag(0, 99), 2)][0]
    for given in (True, False):
        keys, tags, nsym = SS.case_arrays(segs, cases, G, given)
        pk, res, order = SS.emu_txset_emit_syms(segs, keys, tags, nsym, G, hdr, stride)
        want, wres = SS.expected_emit(segs, keys, tags, nsym, G, hdr, stride)
        assert np.array_equal(res, wres), np.flatnonzero(res != wres)[:10]
        bad = np.flatnonzero((pk != want).any(1))
        assert len(bad) == 0, (bad[:8], tags[bad[:8]])
        assert sorted(order.tolist()) == list(range(len(tags)))
        assert set(res.tolist()) == {0, XS.FOREIGN, XS.NOT_READY, S.BAD_RANGE}
        if given:  # a given count across K: the receiver takes it (the ingest test), the sender refuses it
            assert res[across_K] == S.BAD_RANGE
        for k in np.flatnonzero(res != 0):  # no packet is half written
            assert (pk[k] == XS.FILL).all(), k
        for k in np.flatnonzero(res == 0):  # header, and the bytes behind the run are untouched
            c = int(nsym[k]) if given else None
            if hdr == 8:
                assert bytes(pk[k, :4]) == int(keys[k]).to_bytes(4, "big")
            if hdr:
                assert bytes(pk[k, hdr - 4:hdr]) == int(tags[k]).to_bytes(4, "big")
            if c is not None:
                assert (pk[k, hdr + c * T:] == XS.FILL).all(), k


@pytest.mark.parametrize("hdr", [0, 4, 8])
def test_g1_emit_is_the_one_symbol_set(hdr):
    T = 13
    rng = np.random.default_rng(3 + hdr)
    segs = _segs(rng, T)
    stride = T + hdr + 2
    keys, tags = XS.keyed_tags(rng, segs, 300, objects=[(SS.OBJ_KEY, SS.OBJ_Z)])
    pk1, res1, order1 = XS.emu_txset_emit(segs, keys, tags, hdr, stride)
    pk, res, order = SS.emu_txset_emit_syms(segs, keys, tags, None, 1, hdr, stride)
    assert np.array_equal(pk, pk1) and np.array_equal(res, res1) and np.array_equal(order, order1)
    assert {0, XS.FOREIGN, XS.NOT_READY} <= set(res.tolist())


def test_path_and_word_rules():
    """the exported rules: the 8-byte header takes the key walk where everything is 16-byte aligned, and 4-byte words in the copy"""
    assert SS.emit_path(0x1000, 1040, 64, 8) == "TXS_V16_KEY" and SS.emit_path(0x1000, 1040, 64, 4) == "TX_V16_SHIFT"
    assert SS.emit_path(0x1000, 1024, 64, 0) == "TX_V16" and SS.emit_path(0x1000, 88, 20, 8) == "TX_DWORD"
    assert SS.emit_path(0x1000, 73, 13, 8) == "TX_BYTE"
    assert SS.copy_word(0x1000, 1024, 0, 64) == 16 and SS.copy_word(0x1000, 1040, 8, 64) == 4 and SS.copy_word(0x1000, 73, 8, 13) == 1
