"""CPU tier of the listings as runs (nrq_rx_want_syms / nrq_rx_held_syms) and of the held emit of packets of several symbols
(NRQ_TX_HELD in nrq_tx_emit_syms), through runs_emu.cpp over runs_body.h.  The reference is the packetisation of
include/nanorq_hip.h in ten lines of Python (runs_support.packetise) applied to the one-symbol lists of the models the one-symbol
listings are tested against; every comparison is exact, (first tags, counts) word for word, and the expansion of every list is
the one-symbol list.  The emulation is handed bitmaps with poison words behind them and outputs with guards behind them."""
import numpy as np
import pytest

import nanorq_amd
import runs_support as U
import syms_support as S
from held_support import emu_emit_held, emu_rx_held
from relay_support import FOREIGN, NOT_READY
from rx_support import EmuRx, ModelRx, payloads_for, tag
from test_gpu_syms import ROWS
from tx_support import FILL
from want_support import CASE_NAMES, NBLK, SBN0, WANT_SOURCE, case as case_of, emu_rx_want, model_want

T = 4
HI = (1 << 24) - 1
BAD_RANGE = S.BAD_RANGE


def _fill(case):
    emu = EmuRx(case.K, T, NBLK, case.rep_cap, sbn0=SBN0, max_esi=case.max_esi, Kp=case.Kp)
    mod = ModelRx(case.K, T, NBLK, case.rep_cap, sbn0=SBN0, max_esi=case.max_esi, Kp=case.Kp)
    for part in np.array_split(case.stream, 2):
        pay = payloads_for(part, T)
        assert np.array_equal(emu.add(pay, tags=part), mod.add(pay, part))
    return emu, mod


_FILLED = {}


def _filled(name):
    if name not in _FILLED:
        _FILLED[name] = _fill(case_of(name))
    return _FILLED[name]


def _same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ------------------------------------------------------------------------------------------------------------ want lists ----
@pytest.mark.parametrize("G", U.GS)
@pytest.mark.parametrize("name", CASE_NAMES)
def test_want_lists(name, G):
    case = case_of(name)
    emu, mod = _filled(name)
    for source, extra, esi_from in case.queries:
        L = model_want(mod, extra=extra, source=source, esi_from=esi_from)
        want = U.packetise(L, G, lambda sbn: case.K)
        rc, npkt, nsym, tg, ns = U.emu_want_syms(emu, G, WANT_SOURCE if source else 0, extra, esi_from)
        q = (name, G, source, extra, esi_from)
        assert rc == 0 and npkt == len(want[0]) and nsym == len(L), (q, npkt, len(want[0]), nsym, len(L))
        assert _same((tg, ns), want), q
        assert np.array_equal(U.expanded(tg, ns, G), L), q
        if G == 1:
            assert np.array_equal(tg, L) and (ns == 1).all()
        assert np.array_equal(emu_rx_want(emu, WANT_SOURCE if source else 0, extra, esi_from)[2], L), q  # (the one-symbol emulation)


def test_want_shapes_that_can_go_wrong():
    """the packets the cases were built for, written out"""
    case = case_of("rounds_source")
    emu, _ = _filled("rounds_source")
    _, _, _, tg, ns = U.emu_want_syms(emu, 5, WANT_SOURCE)
    pk = {int(t): int(c) for t, c in zip(tg, ns)}
    b1 = (SBN0 + 1) << 24  # one run of 8200: the packet of ESI 8190 straddles the round (8192 % 5 = 2)
    assert pk[b1 | 8190] == 5 and pk[b1 | 8195] == 5 and (b1 | 8192) not in pk and sum(1 for t in pk if t >> 24 == SBN0 + 1) == 1640
    b0 = SBN0 << 24  # runs of two: (31, 32) straddles a word, (8191, 8192) the round
    assert pk[b0 | 31] == 2 and (b0 | 32) not in pk and pk[b0 | 8191] == 2 and (b0 | 8192) not in pk
    _, _, _, tg2, ns2 = U.emu_want_syms(emu, 2, WANT_SOURCE)
    assert (ns2[(tg2 >> 24) == SBN0] == 2).sum() == 8200 // 3 and (ns2[(tg2 >> 24) == SBN0] == 1).sum() == 0
    # runs of 6 between every 7th ESI; `need` cuts the last packet
    emu, mod = _filled("rounds_repair")
    L = model_want(mod, extra=8600)
    _, _, nsym, tg, ns = U.emu_want_syms(emu, 5, 0, 8600, 0)
    blk0 = (tg >> 24) == SBN0
    assert nsym == len(L) and set(ns[blk0][:100].tolist()) == {5, 1}
    tg64, ns64 = U.emu_want_syms(emu, 64, 0, 8600, 0)[3:]
    last0 = np.flatnonzero((tg64 >> 24) == SBN0)[-1]
    n0 = int(((L >> 24) == SBN0).sum())
    assert int(ns64[(tg64 >> 24) == SBN0].sum()) == n0 and ns64[last0] == (n0 - int(ns64[:last0].sum()))


# ------------------------------------------------------------------------------------------------------------ held lists ----
def _held_receptions():
    """the receptions of test_held_emu.py's listing cases, and the one whose repair runs cross a round of rows"""
    from test_held_emu import _fill as held_fill
    out = []
    for K in (10, 32, 100, 257):
        rng = np.random.default_rng(K)
        emu, mod, _, _, _, _ = held_fill(rng, K, 8, 5, 250, K // 6 + 1, K // 3 + 2, 0.25, batches=3)
        emu.mark_complete(1)
        mod.mark_complete(1)
        out.append(("K%d" % K, emu, mod))
    out.append(("rows600",) + U.r600_filled())
    return out


_HELD = []


def _held():
    if not _HELD:
        _HELD.extend(_held_receptions())
    return _HELD


@pytest.mark.parametrize("G", U.GS)
def test_held_lists(G):
    for name, emu, mod in _held():
        L = U.model_held(mod)
        assert np.array_equal(emu_rx_held(emu)[2], L), name
        want = U.packetise(L, G, lambda sbn: emu.K)
        rc, npkt, nsym, tg, ns = U.emu_held_syms(emu, G)
        assert rc == 0 and npkt == len(want[0]) and nsym == len(L), (name, G)
        assert _same((tg, ns), want), (name, G)
        assert np.array_equal(U.expanded(tg, ns, G), L), (name, G)


def test_held_rows_across_a_round():
    emu, mod = U.r600_filled()
    s0 = U.R600["sbn0"]
    _, npkt, nsym, tg, ns = U.emu_held_syms(emu, 5)
    pk = [(int(t) >> 24, int(t) & HI, int(c)) for t, c in zip(tg, ns)]
    assert pk[:106] == [(s0, 10 + 5 * j, 5) for j in range(106)]  # one run of 530 rows: row 256 is inside the packet of row 255
    assert pk[106:636] == [(s0 + 1, e, 1) for e in range(539, 9, -1)]  # descending arrival: all counts 1
    assert pk[636:] == [(s0 + 2, 0, 5), (s0 + 2, 5, 4), (s0 + 2, 10, 3)]  # nothing joins K - 1 to K, and there is no symbol 9
    assert nsym == 530 + 530 + 12 and npkt == len(pk)
    # arrival 12, 13, 14 is one packet; 14, 13, 12 three
    for order, want in (((12, 13, 14), [(12, 3)]), ((14, 13, 12), [(14, 1), (13, 1), (12, 1)])):
        rx = EmuRx(10, 4, 1, 8, max_esi=40, Kp=10)
        tags = np.array([tag(0, e) for e in order], np.uint32)
        rx.add(payloads_for(tags, 4), tags=tags)
        _, _, _, tg, ns = U.emu_held_syms(rx, 16)
        assert [(int(t) & HI, int(c)) for t, c in zip(tg, ns)] == want


# -------------------------------------------------------------------------------------------------------------- contract ----
def test_contract():
    emu, mod = _filled("boundary_K32")
    L = model_want(mod, extra=2)
    want = U.packetise(L, 5, lambda sbn: 32)
    n = len(want[0])
    assert n > 4
    for lst, wantl, nsyms in ((lambda **kw: U.emu_want_syms(emu, 5, 0, 2, 0, **kw), want, len(L)),
                              (lambda **kw: U.emu_held_syms(emu, 5, **kw), U.packetise(U.model_held(mod), 5, lambda sbn: 32), len(U.model_held(mod)))):
        n = len(wantl[0])
        assert lst(count_only=True)[:3] == (0, n, nsyms)  # both outputs NULL: the counts only
        rc, n2, s2, tg, ns = lst(cap=n - 1)  # cap one short: refused, the totals still filled, nothing written
        assert rc == -1 and (n2, s2) == (n, nsyms) and (tg == U.GUARD).all() and (ns == U.GUARD_B).all()
        rc, n3, s3, tg, ns = lst(cap=n + 3)
        assert rc == 0 and (n3, s3) == (n, nsyms) and _same((tg[:n], ns[:n]), wantl) and (tg[n:] == U.GUARD).all() and (ns[n:] == U.GUARD_B).all()
        for only in ("tags", "nsym"):  # exactly one of the two outputs
            rc, _, _, tg, ns = lst(only=only)
            assert rc == -1 and (tg == U.GUARD).all() and (ns == U.GUARD_B).all()
    for G in (0, 65):
        assert U.emu_want_syms(emu, G, 0, 2, 0)[0] == -1 and U.emu_held_syms(emu, G)[0] == -1
    for flags, extra, esi_from in ((2, 0, 0), (WANT_SOURCE, 1, 0), (WANT_SOURCE, 0, 1), (0, (1 << 24) + 1, 0)):  # wn_check's refusals
        assert U.emu_want_syms(emu, 5, flags, extra, esi_from)[0] == -1


# ------------------------------------------------------------------------------------------------------------ held emit ----
from runs_support import K3, LOST3, MAXE3, NB3, S3, counts_of, from_one_symbol, mixed_packets, mixed_stream, table  # noqa: E402


@pytest.mark.parametrize("T,G,inline,stride_kind,_path,_w", [r for r in ROWS if r[1] != 1])
def test_held_emit(T, G, inline, stride_kind, _path, _w):
    rng = np.random.default_rng(T * 100 + G)
    Kp = nanorq_amd.params(K3)["Kp"]
    emu = EmuRx(K3, T, NB3, 5 * 64 + 8, sbn0=S3, max_esi=MAXE3, Kp=Kp)
    mod = ModelRx(K3, T, NB3, 5 * 64 + 8, sbn0=S3, max_esi=MAXE3, Kp=Kp)
    for b, es in enumerate(mixed_stream(G)):
        tg = np.array([tag(S3 + b, e) for e in es], np.uint32)
        pay = payloads_for(tg, T, salt=G)
        assert np.array_equal(emu.add(pay, tags=tg), mod.add(pay, tg))
    for b in (0, 1):  # decoded: the lost rows recovered
        fixed = rng.integers(0, 256, (len(LOST3[b]), T), dtype=np.uint8)
        emu.src[b, LOST3[b]] = fixed
        emu.mark_complete(b)
        mod.mark_complete(b)
    ready = np.array([True, False, False])
    inter = rng.integers(0, 256, (NB3, nanorq_amd.params(Kp)["L"], T), dtype=np.uint8)
    span = (S3, NB3, NB3)
    stride = G * T + (4 if inline else 0)
    stride = {"tight": stride, "pad4": stride + 4, "r16": (stride + 15) // 16 * 16}[stride_kind]
    packets = mixed_packets(G)
    tags = np.array([a for a, _ in packets], np.uint32)
    for given in (True, False):
        counts = counts_of(packets, G) if given else [S.rule(K3, int(a) & HI, G) for a in tags]
        nsym = np.array(counts, np.uint8) if given else None
        pk, res = U.emu_emit_held_syms([emu], [Kp], [inter], span, ready, tags, nsym, G, inline, stride)
        want_res = table(tags, counts, G, lambda b: mod.seen[b], ready)
        assert np.array_equal(res, want_res), (given, np.flatnonzero(res != want_res))
        if given:
            assert set(res.tolist()) == {0, FOREIGN, NOT_READY, BAD_RANGE}
        one_tags = U.expanded(tags[res == 0], [c for c, r in zip(counts, res) if r == 0], G)
        one, one_res = emu_emit_held([emu], [Kp], [inter], span, ready, one_tags, False, T)
        assert (one_res == 0).all()
        want = from_one_symbol(one, tags, counts, res, G, T, inline, stride)
        bad = np.flatnonzero((pk != want).any(1))
        assert len(bad) == 0, (given, bad[:8], tags[bad[:8]])
    # without the flag nothing changed: the several-symbol emit's own emulation, same mask
    seg = [(K3, Kp, S3, emu.src.reshape(NB3, -1), inter)]
    pk0, res0 = S.emu_emit_table(seg, span, T, G, inline, stride, tags=tags, nsym=np.array(counts_of(packets, G), np.uint8), ready=U.mask_words(ready))
    blk = (tags >> 24).astype(int) - S3
    assert (res0[(blk == 1) | (blk == 2)] != 0).all() and (pk0[blk != 0] == FILL).all()


def test_held_emit_two_classes():
    """an object's relay: two receptions of different K side by side (the MULTI form of the admission)"""
    from test_held_emu import _fill as held_fill
    rng = np.random.default_rng(3)
    T, G = 20, 4
    eL, mL, KpL, _, _, _ = held_fill(rng, 31, T, 2, 0, 6, 10, 0.15, salt=1)
    eS, mS, KpS, _, _, _ = held_fill(rng, 30, T, 3, 2, 40, 10, 0.3, batches=3, salt=1)
    span, ready = (0, 5, 2), np.array([False, True, False, False, False])
    inters = [rng.integers(0, 256, (r.nblk, nanorq_amd.params(Kp)["L"], T), dtype=np.uint8) for r, Kp in ((eL, KpL), (eS, KpS))]
    lists = [U.emu_held_syms(r, G)[3:] for r in (eL, eS)]
    tags = np.concatenate([lists[0][0], lists[1][0], [tag(1, 25), tag(3, 28), tag(5, 0)]]).astype(np.uint32)
    nsym = np.concatenate([lists[0][1], lists[1][1], [4, 4, 1]]).astype(np.uint8)
    pk, res = U.emu_emit_held_syms([eL, eS], [KpL, KpS], inters, span, ready, tags, nsym, G, True, G * T + 4)
    n = len(tags) - 3
    assert (res[:n] == 0).all() and res[n:].tolist() == [0, BAD_RANGE, FOREIGN]  # (block 1 is ready; 28 + 4 crosses KS = 30)
    one_tags = U.expanded(tags[res == 0], nsym[res == 0], G)
    one, one_res = emu_emit_held([eL, eS], [KpL, KpS], inters, span, ready, one_tags, False, T)
    assert (one_res == 0).all()
    assert np.array_equal(pk, from_one_symbol(one, tags, [int(c) for c in nsym], res, G, T, True, G * T + 4))
