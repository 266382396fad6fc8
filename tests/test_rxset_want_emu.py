"""CPU tier of a reception set's want and held listings with keys (nrq_rxset_want / nrq_rxset_held, want_set_body.h through
rxset_want_emu.cpp): emulated members filled by the emulated ingest, the emulated set-wide listing run over their books in the
kernels' rounds, and every list compared with a numpy model written from the words of include/nanorq_hip.h
(rxset_want_support.model_want / model_held: want_support.host_want per member's block in rxset_decode_support.block_order, the key
repeated).  The emulation gets bitmaps with all-zero words behind them and lists with guard words behind them: a read past a
bitmap shows as a wanted ESI above max_esi, a write past a list in the guards."""
import numpy as np
import pytest

import nanorq_amd
from rx_support import EmuRx, payloads_for
from rxset_support import MIX4, MIX360, EmuSet, keyed_payloads, keyed_stream, rep_cap_of
from rxset_want_support import QUERIES, check_held, check_want, emu_list, model_held, model_want
from want_support import BIG, CASE_NAMES, GUARD, NBLK, SBN0, WANT_SOURCE, case as case_of

T = 16


def _filled(mix, small_cap, seed, n, objZ=None):
    """EmuRx members of a mix (key, K, nblk, sbn0), attached in reverse order and filled through the emulated set ingest with a
    keyed stream; objZ: {key: Z} of the keys that are objects"""
    kps = [nanorq_amd.params(m[1])["Kp"] for m in mix]
    st, mem = EmuSet(), []
    for (key, K, nblk, sbn0), Kp in reversed(list(zip(mix, kps))):
        mem.append((key, EmuRx(K, T, nblk, rep_cap_of(K, small_cap), sbn0, Kp=Kp), (objZ or {}).get(key, 0)))
        st.attach(*mem[-1])
    keys, tags = keyed_stream(np.random.default_rng(seed), mix, kps, n)
    st.add(keyed_payloads(keys, tags, T), keys, tags)
    return mem


def _check_all(mem, queries=QUERIES):
    out = {}
    for source, extra, esi_from in queries:
        out[(source, extra, esi_from)] = check_want(mem, extra=extra, source=source, esi_from=esi_from)
    out["held"] = check_held(mem)
    return out


_CASE_SET = []


def _case_set():
    """every reception of want_support.CASE_NAMES as a member of ONE set, under distinct keys whose order is not the list's"""
    if not _CASE_SET:
        for i, name in enumerate(CASE_NAMES):
            c = case_of(name)
            e = EmuRx(c.K, T, NBLK, c.rep_cap, sbn0=SBN0, max_esi=c.max_esi, Kp=c.Kp)
            for part in np.array_split(c.stream, 2):
                e.add(payloads_for(part, T), tags=part)
            _CASE_SET.append((1000 - 7 * i, e, 0))
    return _CASE_SET


def test_every_single_case_as_a_member_of_one_set():
    """one-word bitmaps, K = 31 / 32 / 33, max_esi = K', two source rounds at K = 8200, thousands of repair ESIs across 256 words:
    members whose K, max_esi and rep_cap all differ, so a wn_q taken from the wrong member gives a wrong list.  Every query of
    every case is put to the whole set."""
    mem = _case_set()
    assert len({(e.K, e.max_esi, e.rep_cap) for _, e, _ in mem}) >= 8
    queries = sorted({q for name in CASE_NAMES for q in case_of(name).queries})
    assert len(queries) > 20
    nonempty = 0
    for source, extra, esi_from in queries:
        mk, mt, mc = check_want(mem, extra=extra, source=source, esi_from=esi_from)
        nonempty += len(mt) > 0
        for key, e, _ in mem:  # nothing above a member's own max_esi, nothing of a repair query below its own K
            es = mt[mk == key] & 0xFFFFFF
            assert (es <= e.max_esi).all() and (source or (es >= max(e.K, min(esi_from, 1 << 24))).all())
    assert nonempty > 15
    mk, mt, mc = check_held(mem)
    assert len(mc) == NBLK * len(CASE_NAMES) and (mc > 0).sum() > len(CASE_NAMES)


@pytest.mark.parametrize("small_cap", [True, False])
@pytest.mark.parametrize("mix,n", [(MIX4, 1500), (MIX360, 5000)], ids=["mix4", "mix360"])
def test_mixes_after_a_keyed_stream(mix, n, small_cap):
    """K = 10, 26, 100 in one set; 360 blocks: a scan over 361 entries, more than the 256 threads of its workgroup"""
    mem = _filled(mix, small_cap, seed=11 + n + small_cap, n=n)
    out = _check_all(mem)
    assert len(out[(True, 0, 0)][1]) > 0 and len(out["held"][1]) > 0
    if not small_cap:  # (with two repair rows per block most incomplete blocks are full: they may ask for nothing)
        assert len(out[(False, 2, 0)][1]) > len(out[(False, 0, 0)][1]) > 0 and len(out[(False, 2, 15)][1]) > 0
        assert len(set(out[(False, 2, 0)][0].tolist())) > 1                      # more than one key asks
    if mix is MIX360:
        assert len(out["held"][2]) == 360


def test_both_caps():
    """1024 blocks of K = 10 over 64 members: the scan takes 1025 entries, five per thread"""
    mix = [(m // 4, 10, 16, 16 * (m % 4)) for m in range(64)]
    mem = _filled(mix, False, seed=5, n=24000)
    out = _check_all(mem, [(True, 0, 0), (False, 2, 0)])
    assert len(out["held"][2]) == 1024 and (out[(False, 2, 0)][2] > 0).sum() > 200


def test_one_span_under_two_keys_and_two_spans_under_one_key():
    mem = _filled([(1, 10, 3, 0), (2, 10, 3, 0), (4, 26, 2, 6), (4, 26, 2, 0)], False, seed=3, n=500)
    assert [m[0] for m in mem] == [4, 4, 2, 1] and mem[0][1].sbn0 == 0 and mem[1][1].sbn0 == 6  # (attached in reverse)
    out = _check_all(mem)
    mk, mt, _ = out[(True, 0, 0)]
    assert (np.diff(mk.astype(np.int64)) >= 0).all()                         # keys ascending ...
    sb = mt[mk == 4] >> 24
    assert (np.diff(sb.astype(np.int64)) >= 0).all() and {0, 1, 6, 7} >= set(sb.tolist()) and sb.min() < 2 and sb.max() >= 6
    assert not np.array_equal(mt[mk == 1], mt[mk == 2])                      # ... and the twin spans have books of their own


def test_an_objects_two_classes():
    """an object of Z = 5 blocks: ZL = 2 blocks of K = 12, then ZS = 3 blocks of K = 10, under one key, beside a plain reception"""
    mem = _filled([(8, 12, 2, 0), (8, 10, 3, 2), (3, 10, 2, 0)], False, seed=9, n=400, objZ={8: 5})
    out = _check_all(mem)
    mk, mt, mc = out[(True, 0, 0)]
    assert len(mc) == 7 and mc[2:4].any() and mc[4:].any()                     # both classes ask
    sb = mt[mk == 8] >> 24
    assert (np.diff(sb.astype(np.int64)) >= 0).all() and sb.max() <= 4         # class L, then class S: SBN order


def test_a_set_whose_blocks_are_all_complete():
    mem = [(k, EmuRx(10, T, 2, 4, sbn0=s, Kp=10), 0) for k, s in ((2, 0), (1, 4))]
    for _, e, _ in mem:
        for b in range(e.nblk):
            e.mark_complete(b)
    for flags in (0, WANT_SOURCE):
        rc, n, cnt, keys, tags = emu_list(mem, "want", flags, 0, 0, cap=6)
        assert rc == 0 and n == 0 and not cnt.any() and (tags == GUARD).all() and (keys == GUARD).all()
    assert len(model_want(mem)[1]) == 0
    mk, mt, mc = check_held(mem)                                               # (held: all K of every block)
    assert list(mc) == [10] * 4


def test_an_empty_set():
    for what in ("want", "held"):
        rc, n, cnt, keys, tags = emu_list([], what, cap=3)
        assert rc == 0 and n == 0 and len(cnt) == 0 and (tags == GUARD).all() and (keys == GUARD).all()


def test_contract():
    mem = _filled(MIX4, False, seed=21, n=1500)
    for what, (mk, mt, mc), args in (("want", model_want(mem, extra=2), (0, 2, 0)), ("held", model_held(mem), ())):
        n = len(mt)
        assert n > 8
        rc, n1, cnt, _, _ = emu_list(mem, what, *args, with_tags=False)            # NULL lists: total and counts
        assert rc == 0 and n1 == n and np.array_equal(cnt, mc)
        rc, n2, cnt, keys, tags = emu_list(mem, what, *args, cap=n - 1)            # too small: refused, total and counts filled,
        assert rc == -1 and n2 == n and np.array_equal(cnt, mc)                    # nothing written, the guards intact
        assert (tags == GUARD).all() and (keys == GUARD).all()
        rc, n3, cnt, keys, tags = emu_list(mem, what, *args, cap=n + 3)
        assert rc == 0 and n3 == n and np.array_equal(tags[:n], mt) and np.array_equal(keys[:n], mk)
        assert (tags[n:] == GUARD).all() and (keys[n:] == GUARD).all()
        rc, n4, cnt, keys, tags = emu_list(mem, what, *args, with_keys=False)      # d_keys NULL: the tags alone
        assert rc == 0 and keys is None and np.array_equal(tags, mt) and np.array_equal(cnt, mc)
        rc, n5, _, _, _ = emu_list(mem, what, *args, raw_keys_only=True)           # d_keys without d_tags
        assert rc == -1 and n5 == 0


def test_argument_errors():
    mem = _filled(MIX4, False, seed=21, n=300)
    for flags, extra, esi_from in ((2, 0, 0), (3, 0, 0), (0x80000000, 0, 0), (WANT_SOURCE, 1, 0), (WANT_SOURCE, 0, 1), (0, BIG + 1, 0)):
        rc, n, cnt, _, _ = emu_list(mem, "want", flags, extra, esi_from)
        assert rc == -1 and n == 0 and (cnt == GUARD).all(), (flags, extra, esi_from)
    assert emu_list(mem, "want", 0, BIG, 0)[0] == 0
