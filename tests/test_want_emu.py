"""CPU tier of the want listing (nrq_rx_want, want_body.h through want_emu.cpp): the emulated ingest (ingest_body.h) fills
receptions, the emulated listing runs over their books in the kernels' rounds, and every list is compared with a numpy model
written from the words of include/nanorq_hip.h (want_support.host_want) over a plain Python model of the reception
(rx_support.ModelRx).  The emulation is handed a seen bitmap with all-zero words behind it and a list with guard words behind
it: a read past the bitmap shows as a wanted ESI above max_esi, a write past the list in the guards."""
import numpy as np
import pytest

from rx_support import ADDED, FULL, EmuRx, ModelRx, payloads_for
from want_support import BIG, GUARD, NBLK, SBN0, WANT_SOURCE, case as case_of, emu_rx_want, host_want, model_want

T = 4


def _fill(case):
    """the case's stream through the emulated ingest and the model, in two calls -> (emu, model, codes)"""
    emu = EmuRx(case.K, T, NBLK, case.rep_cap, sbn0=SBN0, max_esi=case.max_esi, Kp=case.Kp)
    mod = ModelRx(case.K, T, NBLK, case.rep_cap, sbn0=SBN0, max_esi=case.max_esi, Kp=case.Kp)
    codes = []
    for part in np.array_split(case.stream, 2):
        pay = payloads_for(part, T)
        a, m = emu.add(pay, tags=part), mod.add(pay, part)
        assert np.array_equal(a, m)
        codes.append(a)
    assert np.array_equal(emu.gaps, [len(x) for x in mod.missing]) and np.array_equal(emu.nrep, [len(x) for x in mod.reps])
    return emu, mod, np.concatenate(codes)


_FILLED = {}


def _filled(case):
    if case.name not in _FILLED:
        _FILLED[case.name] = _fill(case)
    return _FILLED[case.name]


def _lists(case):
    """every query of the case: the emulation's list equals the model's -> {query: list}"""
    emu, mod, _ = _filled(case)
    out = {}
    for source, extra, esi_from in case.queries:
        want = model_want(mod, extra=extra, source=source, esi_from=esi_from)
        rc, n, got = emu_rx_want(emu, WANT_SOURCE if source else 0, extra, esi_from)
        assert rc == 0 and n == len(want), (case, source, extra, esi_from, n, len(want))
        assert np.array_equal(got, want), (case, source, extra, esi_from)
        assert ((got & 0xFFFFFF) <= case.max_esi).all() and np.array_equal(got, np.unique(got))  # (ascending, block-major)
        out[(source, extra, esi_from)] = got
    return out


def _esis(lst, b):
    return [int(t) & 0xFFFFFF for t in lst if int(t) >> 24 == SBN0 + b]


def test_one_word_per_block():
    case = case_of("one_word")
    emu, mod, codes = _filled(case)
    assert (codes == FULL).sum() == 1 and emu.gaps[0] == 0 and emu.gaps[1] == 10 and emu.nrep[2] == case.rep_cap and emu.nrep[0] == 1
    assert case.max_esi == 20 and emu.bm_words == 1
    ls = _lists(case)
    src = ls[(True, 0, 0)]
    assert _esis(src, 0) == [] and _esis(src, 1) == list(range(10)) and _esis(src, 2) == [1, 4, 6, 9]
    for extra in (0, 1, 2, BIG):  # the untouched block: capped at its 4 free rows; the complete and the full one: nothing
        assert ls[(False, extra, 0)].tolist() == [((SBN0 + 1) << 24) | e for e in (10, 11, 12, 13)]
    assert _esis(ls[(False, 2, 12)], 1) == [12, 13, 14, 15]
    assert _esis(ls[(False, 2, 19)], 1) == [19, 20]  # the last word's mask: nothing above bit 20
    assert _esis(ls[(False, 2, 20)], 1) == [20]
    assert len(ls[(False, 2, 21)]) == 0


def test_cap_by_free_rows_and_surplus():
    case = case_of("free_rows")
    ls = _lists(case)
    assert [_esis(ls[(False, 0, 0)], b) for b in range(3)] == [[10, 11], [], [10 + 1]]  # block 2: ESI 10 is in, 11 the lowest unseen
    assert [_esis(ls[(False, 1, 0)], b) for b in range(3)] == [[10, 11, 13], [], [11]]  # (12 is seen: skipped)
    assert [_esis(ls[(False, 2, 0)], b) for b in range(3)] == [[10, 11, 13], [12], [11]]  # block 1's surplus of 1 is exceeded
    assert _esis(ls[(False, 3, 0)], 2) == [11]  # a need of 5 with r = 3 of 4 rows used lists 1


@pytest.mark.parametrize("K", [31, 32, 33])
def test_word_boundaries(K):
    case = case_of("boundary_K%d" % K)
    emu, mod, _ = _filled(case)
    ls = _lists(case)
    assert all(len(ls[(False, 40, f)]) == 0 for f in (case.max_esi + 1, (1 << 24) - 1, 0xFFFFFFFF))
    assert ls[(False, 40, case.max_esi)].tolist() == [((SBN0 + b) << 24) | case.max_esi for b in range(NBLK) if case.max_esi not in mod.seen[b]]
    assert np.array_equal(ls[(False, 40, K - 1)], ls[(False, 40, K)])  # (esi_from below K: K)
    assert min(int(t) & 0xFFFFFF for t in ls[(False, 40, 0)]) >= K
    assert any(_esis(ls[(False, 40, 0)], b)[-1] >> 5 > K >> 5 for b in range(NBLK))  # a list crosses a word


@pytest.mark.parametrize("K", [10, 31])
def test_need_larger_than_the_range(K):
    case = case_of("short_range_K%d" % K)
    ls = _lists(case)
    got = ls[(False, 1000, 0)]
    per = case.Kp - K + 1
    assert [len(_esis(got, b)) for b in range(NBLK)] == [per, per - (1 if case.Kp > K else 0), per]
    assert ((got & 0xFFFFFF) <= case.max_esi).all() and ((got & 0xFFFFFF) >= K).all()
    assert len(ls[(False, 1000, case.Kp + 1)]) == 0


def test_after_decode_and_reset():
    case = case_of("boundary_K33")
    emu, mod, _ = _fill(case)
    emu.mark_complete(1)
    mod.mark_complete(1)
    for source, extra in ((True, 0), (False, 0), (False, 40)):
        rc, n, got = emu_rx_want(emu, WANT_SOURCE if source else 0, extra, 0)
        assert rc == 0 and np.array_equal(got, model_want(mod, extra=extra, source=source))
        assert _esis(got, 1) == [] and _esis(got, 0) and _esis(got, 2)
    fresh = EmuRx(case.K, T, NBLK, case.rep_cap, sbn0=SBN0, max_esi=case.max_esi, Kp=case.Kp)  # what nrq_rx_reset leaves
    rc, n, got = emu_rx_want(fresh, WANT_SOURCE)
    assert rc == 0 and got.tolist() == [((SBN0 + b) << 24) | e for b in range(NBLK) for e in range(case.K)]


def test_contract():
    case = case_of("boundary_K32")
    emu, mod, _ = _filled(case)
    want = model_want(mod, extra=2)
    n = len(want)
    assert n > 4
    assert emu_rx_want(emu, 0, 2, 0, count_only=True)[:2] == (0, n)  # a NULL list: the count
    rc, n2, small = emu_rx_want(emu, 0, 2, 0, cap=n - 1)  # too small a buffer: refused, the count still given, nothing written
    assert rc == -1 and n2 == n and (small == GUARD).all()
    rc, n3, big = emu_rx_want(emu, 0, 2, 0, cap=n + 3)
    assert rc == 0 and n3 == n and np.array_equal(big[:n], want) and (big[n:] == GUARD).all()
    for flags, extra, esi_from in ((2, 0, 0), (3, 0, 0), (0x80000000, 0, 0), (WANT_SOURCE, 1, 0), (WANT_SOURCE, 0, 1), (0, BIG + 1, 0)):
        assert emu_rx_want(emu, flags, extra, esi_from)[0] == -1, (flags, extra, esi_from)
    assert emu_rx_want(emu, 0, BIG, 0)[0] == 0


def test_more_than_one_fill_round():
    case = case_of("rounds_source")
    emu, mod, _ = _filled(case)
    assert (case.K + 31) // 32 > 256
    ls = _lists(case)
    src = ls[(True, 0, 0)]
    assert [len(_esis(src, b)) for b in range(NBLK)] == [case.K - (case.K + 2) // 3, case.K, (case.K + 2) // 3]
    assert max(_esis(src, 0)) >= 256 * 32 and _esis(src, 2)[-1] == 8199
    case = case_of("rounds_repair")
    emu, mod, codes = _filled(case)
    assert (codes == ADDED).sum() == len(codes) and emu.gaps[2] == 0
    ls = _lists(case)
    r0 = int(emu.nrep[0])
    got = ls[(False, 8600, 0)]
    assert [len(_esis(got, b)) for b in range(NBLK)] == [2 + 8600 - r0, 10 + 8600, 0]
    assert _esis(got, 1)[-1] == 10 + 8610 - 1 >= 256 * 32 and _esis(got, 0)[-1] > 256 * 32
    assert not set(_esis(got, 0)) & set(range(10, 3000, 7))
    big = ls[(False, BIG, 0)]
    assert [len(_esis(big, b)) for b in range(NBLK)] == [9000 - r0, 9000, 0]  # capped at the free rows
    assert _esis(ls[(False, 8600, 8191)], 1)[0] == 8191 and _esis(ls[(False, 8600, 5000)], 0)[0] == 5000


def test_model_is_the_header():
    """the model itself, on a reception written out by hand (K = 4, max_esi = 9, rep_cap = 3)"""
    seen = np.zeros((2, 10), bool)
    seen[0, [0, 2, 5]] = True  # block 0: source 0 and 2, repair 5; block 1: nothing

    def tags(b, es):
        return [((7 + b) << 24) | e for e in es]
    assert host_want(7, 4, 9, 3, seen, [2, 4], [1, 0], source=True).tolist() == tags(0, [1, 3]) + tags(1, [0, 1, 2, 3])
    assert host_want(7, 4, 9, 3, seen, [2, 4], [1, 0]).tolist() == tags(0, [4]) + tags(1, [4, 5, 6])
    assert host_want(7, 4, 9, 3, seen, [2, 4], [1, 0], extra=2).tolist() == tags(0, [4, 6]) + tags(1, [4, 5, 6])
    assert host_want(7, 4, 9, 3, seen, [2, 4], [1, 0], extra=2, esi_from=9).tolist() == tags(0, [9]) + tags(1, [9])
    assert host_want(7, 4, 9, 3, seen, [0, 4], [1, 0], extra=2, esi_from=10).tolist() == []
