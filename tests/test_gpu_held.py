"""GPU tier of the held symbols (NRQ_TX_HELD on a relay's tag-list emit, nrq_rx_held / nrq_orx_held): a relay answers, for a block
that is not ready, with the symbols its reception holds, and a reception lists what it holds.

Every payload comparison is byte-exact.  Expected packets are the origin's (a Sender / ObjectSender over the original data, whose
own agreement with the oracle is test_gpu_tx.py's and test_gpu_obj.py's subject), and a sample of held repair packets is checked
against the oracle directly.  Packets that must stay untouched are checked against the buffer's fill byte.  Where a decode is part
of a test, the oracle's verdict on the very reception pattern is asserted first, on the CPU, so no case depends on a lucky rank."""
import hashlib

import numpy as np
import pytest

import nanorq_amd
from nanorq_amd import EXT_PER_BLOCK_KP, EXT_SUBBLOCKS, TX_NOT_READY, NrqError
from held_support import emu_emit_held, host_held
from rx_support import ADDED, DUP, FULL, EmuRx, ModelRx, payloads_for
from tx_support import FILL, emit_mode, params_L, range_tags, tag
from util import payload

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available()
    return t


@pytest.fixture(scope="module")
def ctx(torch):
    import gpu_support as G
    return G.ctx()


def _dev(torch, a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()  # (torch's stream and the library's are not ordered)
    return t


def _tags_dev(torch, tags):
    return _dev(torch, np.ascontiguousarray(tags, np.uint32).view(np.int32))


def _host(ctx, t):
    ctx.sync()
    return t.cpu().numpy()


def _emit(ctx, torch, tx, tags, T, inline=False, slack=0, held=True):
    """tx.emit(tags) into a prefilled buffer with a guard row on either side -> (packets [n, stride] device, results numpy)"""
    n = len(tags)
    stride = T + (4 if inline else 0) + slack
    buf = torch.full((n + 2, stride), FILL, dtype=torch.uint8, device="cuda")
    res = torch.full((n,), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    tx.emit(_tags_dev(torch, tags), out=buf[1:n + 1], inline=inline, results=res, held=held)
    ctx.sync()
    assert bool((buf[0] == FILL).all()) and bool((buf[n + 1] == FILL).all()), "guard rows"
    return buf[1:n + 1], res.cpu().numpy()


def _add(ctx, torch, rx, pkts, tags=None, inline=False):
    """rx.add -> the result codes (numpy)"""
    res = torch.full((pkts.shape[0],), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rx.add(pkts, tags=None if tags is None else _tags_dev(torch, tags), inline=inline, results=res)
    return _host(ctx, res)


def _untouched(torch, pk, rows):
    """the packets `rows` (bool numpy) still hold the fill byte"""
    return bool((pk[_dev(torch, rows)] == FILL).all())


def _same(torch, a, b, rows, width):
    """the first `width` bytes of the packets `rows` (bool numpy) are equal (what lies behind a packet is nobody's)"""
    m = _dev(torch, rows)
    return bool(torch.equal(a[m][:, :width], b[m][:, :width]))


def _blocks(K, T, nblk, seed):
    return np.stack([payload(K * T, seed=seed, block=b).reshape(K, T) for b in range(nblk)])


def _oracle_symbols(orc, src, K, T, esis, Kp=0):
    esis = np.asarray(esis, np.uint32)
    out = np.zeros((len(esis), T), np.uint8)
    lo = esis < K
    out[lo] = src[esis[lo]]
    if (~lo).any():
        out[~lo] = orc.encode_block(src, K, T, esis[~lo], Kp=Kp)[0]
    return out


# ------------------------------------------------------------------------------------------------------ 1. partial blocks ----
@pytest.mark.parametrize("K,nblk,inline", [(1000, 5, False), (1000, 4, True), (8192, 4, False)])
def test_partial_blocks(ctx, torch, orc, K, nblk, inline):
    T, sbn0, R = 1280, 2, K // 8
    src = _blocks(K, T, nblk, seed=K + nblk)
    rng = np.random.default_rng(K + nblk)
    with nanorq_amd.Sender(ctx, K, T, nblk, _dev(torch, src), sbn0=sbn0) as tx:
        tx.encode()
        sent = tx.emit_range(0, K + R, interleave=True, inline=inline)
        ctx.sync()
        tags = range_tags(nblk, sbn0, 0, K + R, True)
        n = len(tags)
        deliv = np.flatnonzero(rng.random(n) >= 0.1)
        rng.shuffle(deliv)
        with nanorq_amd.Receiver(ctx, K, T, nblk, rep_cap=R, sbn0=sbn0) as rx:
            codes = _add(ctx, torch, rx, sent[_dev(torch, deliv)].contiguous(), tags=None if inline else tags[deliv], inline=inline)
            assert (codes == ADDED).all()  # (no block is complete, every repair symbol finds a row)
            with rx.relay() as relay:
                assert not relay.ready().any()
                got = np.zeros(n, bool)
                got[deliv] = True
                off = 4 if inline else 0
                slack = sent.shape[1] - T - off
                pk, res = _emit(ctx, torch, relay, tags, T, inline=inline, slack=slack)
                assert np.array_equal(res == 0, got) and (res[~got] == TX_NOT_READY).all()
                assert _same(torch, pk, sent, got, T + off), "a held packet differs from the origin's"
                assert _untouched(torch, pk, ~got)
                # a sample of the held repair packets against the oracle
                rep = np.flatnonzero(got & ((tags & 0xFFFFFF) >= K) & ((tags >> 24) == sbn0 + 1))[:6]
                want = _oracle_symbols(orc, src[1], K, T, tags[rep] & 0xFFFFFF)
                assert np.array_equal(pk[_dev(torch, rep)].cpu().numpy()[:, off:off + T], want)
                # without the flag: as ever, nothing of a block that is not ready
                pk0, res0 = _emit(ctx, torch, relay, tags, T, inline=inline, slack=slack, held=False)
                assert (res0 == TX_NOT_READY).all() and bool((pk0 == FILL).all())
                # every path of the payload copy: dword (a packet stride of T + 4) and byte (an odd one) beside the 16-byte ones
                some = rng.choice(n, 3000, replace=False)
                for inl, slack in ((True, 0), (False, 3), (True, 12)):
                    pk2, res2 = _emit(ctx, torch, relay, tags[some], T, inline=inl, slack=slack)
                    o2 = 4 if inl else 0
                    assert np.array_equal(res2 == 0, got[some]) and (res2[~got[some]] == TX_NOT_READY).all()
                    assert bool(torch.equal(pk2[_dev(torch, got[some])][:, o2:o2 + T], sent[_dev(torch, some[got[some]])][:, off:off + T]))
                    assert _untouched(torch, pk2, ~got[some])
                    if inl:
                        hd = pk2[_dev(torch, got[some])][:, :4].cpu().numpy()
                        assert np.array_equal(hd, tags[some][got[some]].astype(">u4").view(np.uint8).reshape(-1, 4))


def test_second_round_of_the_shifted_form_matches_emulation(ctx, torch):
    """nrq_emit_held_kernel<TX_V16_SHIFT, false> at T = 1040 (65 chunks of 16 bytes: a second round of the wave with one live lane,
    whose left neighbour is the carry of lane 63) against the emulated held emit, whole buffer and guard rows: a reception and
    its emulation fed the same lossy stream, block 0 complete and made ready by the relay's encode, so ready packets (gathers
    over the intermediate symbols), held source and repair rows (copies), symbols not held and foreign SBNs are all asked for"""
    K, T, nblk, sbn0, cap = 30, 1040, 3, 2, 8
    Kp = nanorq_amd.params(K)["Kp"]
    L = params_L(Kp)
    rng = np.random.default_rng(1040)
    emu = EmuRx(K, T, nblk, cap, sbn0=sbn0, Kp=Kp)
    sent = np.array([tag(sbn0 + b, e) for b in range(nblk) for e in range(K + K // 4 + 4)], np.uint32)
    keep = (rng.random(len(sent)) >= 0.25) | ((sent >> 24) == sbn0)  # (block 0 loses nothing)
    deliv = sent[keep]
    rng.shuffle(deliv)
    with nanorq_amd.Receiver(ctx, K, T, nblk, cap, sbn0=sbn0) as rx, rx.relay() as relay:
        for part in np.array_split(deliv, 2):
            pl = payloads_for(part, T, 3)
            _add(ctx, torch, rx, _dev(torch, pl), tags=part)
            emu.add(pl, tags=part)
        relay.encode()
        ctx.sync()
        ready = relay.ready()
        assert ready[0] and not ready[1:].any()
        inter = ctx.download(relay.inter_ptr, nblk * L * T).reshape(nblk, L, T)
        extra = [tag(s, e) for s in range(sbn0 - 1, sbn0 + nblk + 1) for e in (emu.max_esi, emu.max_esi + 1, (1 << 24) - 1, K + 60)]
        ask = np.concatenate([sent, np.array(extra, np.uint32)])
        rng.shuffle(ask)
        n, stride = len(ask), T + 16
        buf = torch.full((n + 2, stride), FILL, dtype=torch.uint8, device="cuda")
        out = buf[1:n + 1]
        rows = [(rx.src_ptr, K * T), (relay.inter_ptr, L * T), (rx.rep_ptr, cap * T)]
        assert emit_mode(out.data_ptr(), stride, T, 4, rows) == "TX_V16_SHIFT"
        res = torch.full((n,), 77, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        relay.emit(_tags_dev(torch, ask), out=out, inline=True, results=res, held=True)
        ctx.sync()
        epk, eres = emu_emit_held([emu], [Kp], [inter], (sbn0, nblk, nblk), ready, ask, True, stride)
        res = res.cpu().numpy()
        assert np.array_equal(res, eres), np.flatnonzero(res != eres)[:10]
        got = buf.cpu().numpy()
        assert (got[0] == FILL).all() and (got[-1] == FILL).all(), "guard rows"
        assert np.array_equal(got[1:-1], epk), np.flatnonzero((got[1:-1] != epk).any(axis=1))[:10]
        blk, esi = (ask >> 24).astype(int) - sbn0, ask & 0xFFFFFF
        cold = (blk >= 1) & (blk < nblk)
        assert (res[(blk == 0) & (esi >= K)] == 0).any() and (res[cold & (esi < K)] == 0).any() and (res[cold & (esi >= K)] == 0).any()
        assert (res[cold] == TX_NOT_READY).any() and (res == -1).any()


# ---------------------------------------------------------------------------------------------------------------- 2. codes ----
def test_codes(ctx, torch, orc):
    K, T, nblk, sbn0, rep_cap = 100, 32, 3, 4, 5
    max_esi = 2 * nanorq_amd.params(K)["Kp"]
    src = _blocks(K, T, nblk, seed=3)
    keep = [np.setdiff1d(np.arange(K), [3, 9, 50 + b]) for b in range(nblk)]
    reps = [np.array([K + 7, K + 1, K + 30, K + 2, K + 90, K + 4, K + 5], np.uint32) for b in range(nblk)]  # 7 for 5 rows
    tags, rows = [], []
    for b in range(nblk):
        es = np.concatenate([keep[b], reps[b], keep[b][:4], reps[b][:2]]).astype(np.uint32)  # (some twice: DUP)
        tags.append(((sbn0 + b) << 24) | es)
        rows.append(_oracle_symbols(orc, src[b], K, T, es))
    tags, rows = np.concatenate(tags).astype(np.uint32), np.concatenate(rows)
    with nanorq_amd.Receiver(ctx, K, T, nblk, rep_cap=rep_cap, sbn0=sbn0) as rx, rx.relay() as relay:
        codes = _add(ctx, torch, rx, _dev(torch, rows), tags=tags)
        assert (codes == DUP).sum() == nblk * 6 and (codes == FULL).sum() == nblk * 2
        held_tags = rx.held().cpu().numpy().view(np.uint32)
        assert len(held_tags) == len(np.unique(held_tags)) == (codes == ADDED).sum()  # a DUP symbol is held once
        ask = np.concatenate([tags, [tag(sbn0 + b, e) for b in range(nblk) for e in
                                     (3, 50 + b, K + 8, max_esi, max_esi + 1, max_esi + 40, (max_esi // 32 + 1) * 32, (1 << 24) - 1)],
                              [tag(sbn0 - 1, 0), tag(sbn0 + nblk, 1), tag(255, K + 7)]]).astype(np.uint32)
        pk, res = _emit(ctx, torch, relay, ask, T, inline=True, slack=4)
        pk = pk.cpu().numpy()
        have = set(int(t) for t in tags[codes == ADDED])
        assert all(int(t) not in have for t in tags[codes == FULL])
        for k, t in enumerate(ask):
            b = (int(t) >> 24) - sbn0
            if not 0 <= b < nblk:
                assert res[k] == -1 and (pk[k] == FILL).all(), k
            elif int(t) in have:
                assert res[k] == 0 and bytes(pk[k, :4]) == int(t).to_bytes(4, "big"), k
                assert np.array_equal(pk[k, 4:4 + T], _oracle_symbols(orc, src[b], K, T, [int(t) & 0xFFFFFF])[0]), k
                assert (pk[k, 4 + T:] == FILL).all(), k
            else:  # lost, never sent, FULL, above max_esi
                assert res[k] == TX_NOT_READY and (pk[k] == FILL).all(), (k, hex(int(t)))
        # the range forms and a plain sender refuse the flag
        with pytest.raises(NrqError, match="NRQ_TX_HELD goes with a tag list"):
            relay.emit_range(0, 4, held=True)
        with nanorq_amd.Sender(ctx, K, T, nblk, _dev(torch, src), sbn0=sbn0) as tx:
            tx.encode()
            with pytest.raises(NrqError, match="NRQ_TX_HELD needs a relay"):
                tx.emit(_tags_dev(torch, ask), held=True)
            with pytest.raises(NrqError, match="NRQ_TX_HELD goes with a tag list"):
                tx.emit_range(0, 4, held=True)
        # nothing is held after a reset
        rx.reset()
        assert rx.held().numel() == 0
        pk, res = _emit(ctx, torch, relay, ask, T)
        inside = ((ask >> 24) >= sbn0) & ((ask >> 24) < sbn0 + nblk)
        assert (res[inside] == TX_NOT_READY).all() and (res[~inside] == -1).all() and bool((pk == FILL).all())


def test_object_sender_refuses_the_flag(ctx, torch):
    Kt, T = 213, 64
    obj = _dev(torch, payload(Kt * T - 37, seed=4))
    with nanorq_amd.ObjectSender(ctx, obj, T, Z=5) as tx:
        tx.encode()
        with pytest.raises(NrqError, match="NRQ_TX_HELD needs a relay"):
            tx.emit(_tags_dev(torch, [tag(0, 1)]), held=True)
        with pytest.raises(NrqError, match="NRQ_TX_HELD goes with a tag list"):
            tx.emit_all(2, held=True)


# --------------------------------------------------------------------------------------------------------- 3. mixed states ----
def test_mixed_states_in_one_call(ctx, torch, orc):
    """block 0: decoded with the relay attached (ready); block 1: decoded before it was attached (complete, not ready); block 2:
    short of symbols"""
    K, T, nblk, sbn0 = 100, 48, 3, 9
    src = _blocks(K, T, nblk, seed=11)
    lost = [np.array([1, 17, 60, 99]), np.array([0, 5, 44]), np.array([2, 3, 70, 71, 72])]
    reps = [np.array([K + 3, K + 40, K + 9, K + 1, K + 77, K + 6], np.uint32), np.array([K + 12, K + 2, K + 31, K + 8, K + 50], np.uint32),
            np.array([K + 5, K + 6], np.uint32)]
    got = [np.concatenate([np.setdiff1d(np.arange(K), lost[b]), reps[b]]).astype(np.uint32) for b in range(nblk)]
    sym = [_oracle_symbols(orc, src[b], K, T, got[b]) for b in range(nblk)]
    for b in (0, 1):
        ok, out, _ = orc.decode_block(got[b], sym[b], K, T, max_esi=(1 << 24) - 1)
        assert ok and np.array_equal(out, src[b]), "the oracle does not decode block %d of this reception" % b
    fresh = np.array([K + 200, K + 201, (1 << 24) - 1], np.uint32)
    ask_e = [np.concatenate([np.arange(K), reps[b], fresh]).astype(np.uint32) for b in range(nblk)]
    ask = np.concatenate([((sbn0 + b) << 24) | ask_e[b] for b in range(nblk)]).astype(np.uint32)
    want = np.concatenate([_oracle_symbols(orc, src[b], K, T, ask_e[b]) for b in range(nblk)])
    blk = (ask >> 24).astype(int) - sbn0
    esi = ask & 0xFFFFFF
    is_fresh = np.isin(esi, fresh)
    with nanorq_amd.Receiver(ctx, K, T, nblk, rep_cap=16, sbn0=sbn0) as rx:
        assert (_add(ctx, torch, rx, _dev(torch, sym[1]), tags=((sbn0 + 1) << 24) | got[1]) == ADDED).all()
        assert list(rx.decode()[0]) == [0, 1, 0]
        with rx.relay() as relay:
            for b in (0, 2):
                assert (_add(ctx, torch, rx, _dev(torch, sym[b]), tags=((sbn0 + b) << 24) | got[b]) == ADDED).all()
            assert list(rx.decode()[0]) == [1, 1, 0]
            assert list(relay.ready()) == [True, False, False]
            pk, res = _emit(ctx, torch, relay, ask, T)
            pk = pk.cpu().numpy()
            held2 = np.isin(esi, got[2])
            ok = (blk == 0) | ((blk == 1) & ~is_fresh) | ((blk == 2) & held2)
            assert np.array_equal(res == 0, ok) and (res[~ok] == TX_NOT_READY).all()
            assert np.array_equal(pk[ok], want[ok]) and (pk[~ok] == FILL).all()
            # the ready block without the flag: the same bytes
            pk0, res0 = _emit(ctx, torch, relay, ask, T, held=False)
            pk0 = pk0.cpu().numpy()
            assert np.array_equal(res0 == 0, blk == 0) and np.array_equal(pk0[blk == 0], pk[blk == 0]) and (pk0[blk != 0] == FILL).all()
            # the encode makes the complete block ready: it answers everything
            relay.encode()
            assert list(relay.ready()) == [True, True, False]
            pk, res = _emit(ctx, torch, relay, ask, T)
            pk = pk.cpu().numpy()
            ok = (blk != 2) | held2
            assert np.array_equal(res == 0, ok) and np.array_equal(pk[ok], want[ok]) and (pk[~ok] == FILL).all()


# -------------------------------------------------------------------------------------------------------------- 4. listing ----
def _reception(orc, K, T, nblk, sbn0, seed, loss=0.1, extra=2):
    """per block: the original rows, the ESIs that arrive (kept source ESIs and lost + extra repair ESIs, shuffled) and their
    symbols; the oracle decodes each block from exactly these"""
    rng = np.random.default_rng(seed)
    src = _blocks(K, T, nblk, seed=seed)
    esis, syms = [], []
    for b in range(nblk):
        gone = rng.choice(K, max(1, int(K * loss)), replace=False)
        es = np.concatenate([np.setdiff1d(np.arange(K), gone), rng.choice(np.arange(K, 2 * K), len(gone) + extra, replace=False)])
        es = es.astype(np.uint32)
        rng.shuffle(es)
        sy = _oracle_symbols(orc, src[b], K, T, es)
        ok, out, _ = orc.decode_block(es, sy, K, T, max_esi=(1 << 24) - 1)
        assert ok and np.array_equal(out, src[b]), "the oracle does not decode block %d of this reception" % b
        esis.append(es)
        syms.append(sy)
    return src, esis, syms


def _stream(esis, syms, sbn0, rng):
    tags = np.concatenate([((sbn0 + b) << 24) | e for b, e in enumerate(esis)]).astype(np.uint32)
    rows = np.concatenate(syms)
    order = rng.permutation(len(tags))
    return tags[order], rows[order]


def _state(ctx, rx, K, T):
    """counts, lists, the source rows that are seen and the repair rows in use"""
    nl, nr = rx.counts()
    lost, reps = rx.lists()
    srcrows = _host(ctx, rx.source)
    rep = ctx.download(rx.rep_ptr, rx.nblk * rx.rep_cap * T).reshape(rx.nblk, rx.rep_cap, T)
    seen = [np.setdiff1d(np.arange(K), lost[b]) for b in range(rx.nblk)]
    return nl, nr, lost, reps, [srcrows[b][seen[b]] for b in range(rx.nblk)], [rep[b][:nr[b]] for b in range(rx.nblk)]


@pytest.mark.parametrize("K,T", [(100, 20), (1000, 1280)])
def test_listing_and_full_dump(ctx, torch, orc, K, T):
    nblk, sbn0, rep_cap = 3, 6, K // 5 + 8
    src, esis, syms = _reception(orc, K, T, nblk, sbn0, seed=K)
    rng = np.random.default_rng(K + 1)
    tags, rows = _stream(esis, syms, sbn0, rng)
    with nanorq_amd.Receiver(ctx, K, T, nblk, rep_cap=rep_cap, sbn0=sbn0) as rx, rx.relay() as relay:
        half = len(tags) // 2
        for part in (slice(0, half), slice(half, None)):
            assert (_add(ctx, torch, rx, _dev(torch, rows[part]), tags=tags[part]) == ADDED).all()
        nl, nr, lost, reps, srows, rrows = _state(ctx, rx, K, T)
        lst = rx.held()
        h = lst.cpu().numpy().view(np.uint32)
        seen = [~np.isin(np.arange(K), lost[b]) for b in range(nblk)]
        assert np.array_equal(h, host_held(sbn0, K, seen, reps))
        assert len(h) == int((K - nl + nr).sum()) == len(tags)
        # arrival order of the repair ESIs is the stream's
        for b in range(nblk):
            mine = tags[((tags >> 24) == sbn0 + b) & ((tags & 0xFFFFFF) >= K)] & 0xFFFFFF
            assert np.array_equal(reps[b], mine)
        # the whole list, emitted with held symbols, into a fresh reception: the same books and the same rows
        pk, res = _emit(ctx, torch, relay, h, T)
        assert (res == 0).all()
        with nanorq_amd.Receiver(ctx, K, T, nblk, rep_cap=rep_cap, sbn0=sbn0) as rx2:
            assert (_add(ctx, torch, rx2, pk.contiguous(), tags=h) == ADDED).all()
            nl2, nr2, lost2, reps2, srows2, rrows2 = _state(ctx, rx2, K, T)
            assert np.array_equal(nl, nl2) and np.array_equal(nr, nr2)
            for b in range(nblk):
                assert np.array_equal(lost[b], lost2[b]) and np.array_equal(reps[b], reps2[b])
                assert np.array_equal(srows[b], srows2[b]) and np.array_equal(rrows[b], rrows2[b])
            assert np.array_equal(rx2.held().cpu().numpy().view(np.uint32), h)
            assert rx2.decode()[0].all()
            assert np.array_equal(_host(ctx, rx2.source), src)


def test_listing_past_256_seen_words(ctx, torch):
    """K = 8200: 257 seen words per block, so the fill goes a second round with one live lane and the offset of the first"""
    K, T, nblk, sbn0, rep_cap = 8200, 16, 2, 3, 8
    rng = np.random.default_rng(8200)
    mod = ModelRx(K, T, nblk, rep_cap, sbn0=sbn0, Kp=nanorq_amd.params(K)["Kp"])
    tags = []
    for b in range(nblk):
        have = rng.random(K) < 0.5
        have[[b, 8192 + b, K - 1]] = True  # (seen symbols in the first word and in word 256)
        tags += [tag(sbn0 + b, e) for e in np.flatnonzero(have)] + [tag(sbn0 + b, K + 7 * q + b) for q in range(5)]
    tags = np.array(tags, np.uint32)[rng.permutation(len(tags))]
    pay = payloads_for(tags, T)
    with nanorq_amd.Receiver(ctx, K, T, nblk, rep_cap=rep_cap, sbn0=sbn0) as rx:
        for part in np.array_split(np.arange(len(tags)), 2):
            assert np.array_equal(_add(ctx, torch, rx, _dev(torch, pay[part]), tags=tags[part]), mod.add(pay[part], tags[part]))
        seen = [~np.isin(np.arange(K), mod.lost(b)) for b in range(nblk)]
        want = host_held(sbn0, K, seen, mod.reps)
        assert len(want) == len(tags)
        assert np.array_equal(rx.held().cpu().numpy().view(np.uint32), want)


def test_merge_two_partial_receptions(ctx, torch, orc):
    K, T, nblk, sbn0 = 100, 64, 3, 1
    src, esis, syms = _reception(orc, K, T, nblk, sbn0, seed=77)
    rng = np.random.default_rng(78)
    tags, rows = _stream(esis, syms, sbn0, rng)
    half = len(tags) // 2
    with nanorq_amd.Receiver(ctx, K, T, nblk, rep_cap=40, sbn0=sbn0) as rx3:
        for part in (slice(0, half), slice(half, None)):
            with nanorq_amd.Receiver(ctx, K, T, nblk, rep_cap=40, sbn0=sbn0) as rx, rx.relay() as relay:
                assert (_add(ctx, torch, rx, _dev(torch, rows[part]), tags=tags[part]) == ADDED).all()
                assert not rx.decode()[0].any()  # (half a reception decodes nothing)
                lst = rx.held()
                pk, res = _emit(ctx, torch, relay, lst.cpu().numpy().view(np.uint32), T, inline=True)
                assert (res == 0).all()
                assert (_add(ctx, torch, rx3, pk.contiguous(), inline=True) == ADDED).all()
        assert rx3.held().numel() == len(tags)
        assert rx3.decode()[0].all()
        assert np.array_equal(_host(ctx, rx3.source), src)


# ---------------------------------------------------------------------------------------------------------- 5. cut-through ----
def test_chain_with_cut_through(ctx, torch, orc):
    """A -> B -> C: B forwards what each ingest batch added, from blocks that are not complete, then decodes and tops C up with
    fresh repair symbols.  The link B -> C loses packets too."""
    K, T, nblk, sbn0 = 100, 64, 4, 3
    src, esis, syms = _reception(orc, K, T, nblk, sbn0, seed=91)  # what reaches B, which decodes it (asserted by _reception)
    rng = np.random.default_rng(92)
    tags, rows = _stream(esis, syms, sbn0, rng)
    lose_bc = rng.random(len(tags)) < 0.15
    fresh = [np.arange(3 * K + 10 * b, 3 * K + 10 * b + 24, dtype=np.uint32) for b in range(nblk)]  # ESIs A never sent
    # C's reception, in arrival order, on the CPU: the forwarded packets that survive, then B's fresh repair symbols
    for b in range(nblk):
        mine = ((tags >> 24) == sbn0 + b) & ~lose_bc
        es = np.concatenate([tags[mine] & 0xFFFFFF, fresh[b]]).astype(np.uint32)
        ok, out, _ = orc.decode_block(es, _oracle_symbols(orc, src[b], K, T, es), K, T, max_esi=(1 << 24) - 1)
        assert ok and np.array_equal(out, src[b]), "the oracle does not decode block %d of C's reception" % b
        fw = tags[mine] & 0xFFFFFF
        assert (fw >= K).sum() < K - (fw < K).sum(), "block %d of C would decode before the top-up" % b
    with nanorq_amd.Receiver(ctx, K, T, nblk, rep_cap=48, sbn0=sbn0) as rx_b, rx_b.relay() as relay_b, \
            nanorq_amd.Receiver(ctx, K, T, nblk, rep_cap=64, sbn0=sbn0, max_esi=4 * K) as rx_c:
        for part in np.array_split(np.arange(len(tags)), 5):
            codes = _add(ctx, torch, rx_b, _dev(torch, rows[part]), tags=tags[part])
            assert (codes == ADDED).all()
            assert not relay_b.ready().any() and rx_b.counts()[0].all()  # (no block of B is complete yet)
            fwd = part[codes == ADDED]
            pk, res = _emit(ctx, torch, relay_b, tags[fwd], T, inline=True)
            assert (res == 0).all()
            assert np.array_equal(pk.cpu().numpy()[:, 4:4 + T], rows[fwd])
            live = ~lose_bc[fwd]
            if live.any():
                assert (_add(ctx, torch, rx_c, pk[_dev(torch, live)].contiguous(), inline=True) == ADDED).all()
        assert not rx_c.decode()[0].any()
        assert rx_b.decode()[0].all() and relay_b.ready().all()
        top = np.concatenate([((sbn0 + b) << 24) | fresh[b] for b in range(nblk)]).astype(np.uint32)
        pk, res = _emit(ctx, torch, relay_b, top, T, inline=True)
        assert (res == 0).all()
        rx_c.add(pk.contiguous(), inline=True)
        st, _ = rx_c.decode()
        assert list(st) == [1] * nblk
        assert np.array_equal(_host(ctx, rx_c.source), src)


# -------------------------------------------------------------------------------------------------------------- 6. objects ----
# (Kt, T, Z, N, Al, flags): two block classes (3 blocks of K = 43, 2 of 42), F not a multiple of T
OBJ_CASES = [
    (213, 96, 5, 4, 8, EXT_SUBBLOCKS),
    (213, 64, 5, 1, 8, EXT_PER_BLOCK_KP),
    (213, 100, 5, 1, 4, 0),   # dword rows
]


@pytest.mark.parametrize("inline,slack,mode", [(False, 0, "TX_V16"), (True, 12, "TX_V16_SHIFT"), (True, 0, "TX_DWORD"), (False, 3, "TX_BYTE")])
def test_object_held_emit_modes(ctx, torch, inline, slack, mode):
    """nrq_emit_held_kernel<MODE, true> (an object relay's table of several segments: two block classes) in each of its four
    modes, picked by the packet stride and the header, against the object's own packets: what the reception holds comes back
    byte for byte, what it does not hold stays untouched.  The row images are the library's own allocations, so the mode
    assertion covers what the test hands over: the buffer, its stride and T."""
    Kt, T, Z, nrep = 213, 64, 5, 8
    data = payload(Kt * T - 37, seed=Kt + int(inline) + slack)
    rng = np.random.default_rng(slack + int(inline))
    with nanorq_amd.ObjectSender(ctx, _dev(torch, data), T, Z=Z) as tx:
        assert tx.params.ZL and tx.params.ZS
        tx.encode()
        n = tx.count_all(nrep)
        t_o = torch.zeros(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        sent = tx.emit_all(nrep, inline=True, tags_out=t_o)
        ctx.sync()
        tags = t_o.cpu().numpy().view(np.uint32)
        oti = tx.oti
    got = rng.random(n) >= 0.3
    got[(tags & 0xFFFFFF) == 0] = False  # (no block is complete)
    with nanorq_amd.ObjectReceiver(ctx, *oti, rep_cap=nrep) as rx, rx.relay() as relay:
        assert (_add(ctx, torch, rx, sent[_dev(torch, np.flatnonzero(got))].contiguous(), inline=True) == ADDED).all()
        assert not relay.ready().any()
        ask = np.concatenate([tags, [tag(Z, 0), tag(255, 3)]]).astype(np.uint32)
        off = 4 if inline else 0
        stride = T + off + slack
        pk, res = _emit(ctx, torch, relay, ask, T, inline=inline, slack=slack)
        assert emit_mode(pk.data_ptr(), stride, T, off) == mode
        assert list(res[n:]) == [-1, -1] and bool((pk[n:] == FILL).all())
        pk, res = pk[:n].cpu().numpy(), res[:n]
        assert np.array_equal(res == 0, got) and (res[~got] == TX_NOT_READY).all()
        sent_h = sent.cpu().numpy()
        assert ((tags[got] & 0xFFFFFF) >= 43).any()  # (held repair rows among them: K is 43 and 42)
        assert np.array_equal(pk[got, off:off + T], sent_h[got, 4:4 + T]), "a held packet differs from the origin's"
        if inline:
            assert np.array_equal(pk[got, :4], sent_h[got, :4])
        assert (pk[got, off + T:] == FILL).all() and (pk[~got] == FILL).all()


@pytest.mark.parametrize("case", OBJ_CASES)
def test_objects(ctx, torch, orc, case):
    Kt, T, Z, N, Al, flags = case
    data = payload(Kt * T - 37, seed=Kt + T + N)
    want_sha = hashlib.sha256(data.tobytes()).hexdigest()
    rng = np.random.default_rng(T + N)
    nrep = 16
    with nanorq_amd.ObjectSender(ctx, _dev(torch, data), T, Z=Z, N=N, Al=Al, flags=flags) as tx:
        p = tx.params
        assert p.ZL and p.ZS and p.F % T and p.N == N and (p.KpL != p.KpS) == bool(flags & EXT_PER_BLOCK_KP)
        tx.encode()
        n = tx.count_all(nrep)
        t_o = torch.zeros(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        sent = tx.emit_all(nrep, inline=True, tags_out=t_o)
        ctx.sync()
        tags = t_o.cpu().numpy().view(np.uint32)
        oti, blocks = tx.oti, tx.blocks
        # five source symbols of every block are lost, and a tenth of the rest
        sbn, esi = tags >> 24, tags & 0xFFFFFF
        Ks = np.array([K for K, _ in blocks])[sbn]
        drop = rng.random(n) < 0.1
        for b, (K, _) in enumerate(blocks):
            drop |= (sbn == b) & np.isin(esi, rng.choice(K, 5, replace=False))
        deliv = np.flatnonzero(~drop)
        rng.shuffle(deliv)
        # the oracle decodes this reception, block by block
        sent_h = sent.cpu().numpy()
        for b, (K, Kp) in enumerate(blocks):
            mine = deliv[sbn[deliv] == b]
            ok, _, _ = orc.decode_block(esi[mine], sent_h[mine, 4:4 + T], K, T, Kp=Kp, max_esi=p.max_esi)
            assert ok, "the oracle does not decode block %d of this reception" % b
        with nanorq_amd.ObjectReceiver(ctx, *oti, flags=flags, rep_cap=24) as rx, rx.relay() as relay:
            half = len(deliv) // 2
            for part in (deliv[:half], deliv[half:]):
                assert (_add(ctx, torch, rx, sent[_dev(torch, part)].contiguous(), inline=True) == ADDED).all()
            assert not relay.ready().any()
            got = ~drop
            ask = np.concatenate([tags, [tag(Z, 0), tag(0, p.max_esi + 1), tag(Z - 1, (1 << 24) - 1)]]).astype(np.uint32)
            pk, res = _emit(ctx, torch, relay, ask, T, inline=True, slack=sent.shape[1] - T - 4)
            assert list(res[n:]) == [-1, TX_NOT_READY, TX_NOT_READY] and bool((pk[n:] == FILL).all())
            pk, res = pk[:n], res[:n]
            assert np.array_equal(res == 0, got) and (res[~got] == TX_NOT_READY).all()
            m = _dev(torch, got)
            assert bool(torch.equal(pk[m][:, :T + 4], sent[m][:, :T + 4])), "a held packet differs from the origin's"
            assert _untouched(torch, pk, ~got)
            _, res0 = _emit(ctx, torch, relay, tags, T, inline=True, held=False)
            assert (res0 == TX_NOT_READY).all()
            # the listing: both classes in SBN order, per block the source ESIs ascending, then the repair ESIs as they arrived
            h = rx.held().cpu().numpy().view(np.uint32)
            d_sbn, d_esi = sbn[deliv], esi[deliv]
            seen = [np.isin(np.arange(K), d_esi[(d_sbn == b)]) for b, (K, _) in enumerate(blocks)]
            arr = [d_esi[(d_sbn == b) & (d_esi >= K)] for b, (K, _) in enumerate(blocks)]
            want = np.concatenate([host_held(b, K, [seen[b]], [arr[b]]) for b, (K, _) in enumerate(blocks)])
            assert np.array_equal(h, want) and len(h) == len(deliv)
            nl, nr = rx.counts()
            assert len(h) == int((np.array([K for K, _ in blocks]) - nl + nr).sum())
            # the full dump into a second receiver, which decodes the object
            pk, res = _emit(ctx, torch, relay, h, T, inline=True)
            assert (res == 0).all()
            with nanorq_amd.ObjectReceiver(ctx, *oti, flags=flags, rep_cap=24) as rx2:
                assert (_add(ctx, torch, rx2, pk.contiguous(), inline=True) == ADDED).all()
                nl2, nr2 = rx2.counts()
                assert np.array_equal(nl, nl2) and np.array_equal(nr, nr2)
                assert np.array_equal(rx2.held().cpu().numpy().view(np.uint32), h)
                assert rx2.decode()[0].all()
                out, left = rx2.write()
                assert left == 0 and hashlib.sha256(_host(ctx, out).tobytes()).hexdigest() == want_sha
            # after the relay's own decode every block is ready and the flag changes nothing
            assert rx.decode()[0].all() and relay.ready().all()
            pk, res = _emit(ctx, torch, relay, tags, T, inline=True, slack=sent.shape[1] - T - 4)
            assert (res == 0).all() and bool(torch.equal(pk[:, :T + 4], sent[:, :T + 4]))
