"""GPU tier of the want listing (nrq_rx_want / nrq_orx_want): a reception writes into device memory the tags it still wants, in the
form the emits take, so that want -> emit -> add -> decode runs without a host-built list.

The listing is compared with a numpy model written from the words of include/nanorq_hip.h (want_support.host_want) over books
that are known on the host.  The list is deterministic, so where a decode is part of a test the reception pattern after the
top-up is known beforehand: the oracle's verdict on exactly that pattern is asserted first, on the CPU, so no case depends on a
lucky rank."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import nanorq_amd
from nanorq_amd import EXT_PER_BLOCK_KP, TX_NOT_READY, WANT_SOURCE, NrqError
from rx_support import ADDED, ModelRx, payloads_for
from tx_support import FILL
from util import payload
from want_support import CASE_NAMES, GUARD, NBLK, SBN0, case as case_of, host_want, model_want

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


def _u32(ctx, t):
    return _host(ctx, t).view(np.uint32)


def _add(ctx, torch, rx, pkts, tags=None, inline=False):
    """rx.add -> the result codes (numpy); tags: a numpy array or a device tensor"""
    res = torch.full((pkts.shape[0],), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    if tags is not None and not hasattr(tags, "data_ptr"):
        tags = _tags_dev(torch, tags)
    rx.add(pkts, tags=tags, inline=inline, results=res)
    return _host(ctx, res)


def _emit(ctx, torch, tx, tags, T, inline=False, held=False):
    """tx.emit(tags: device tensor) into a prefilled buffer -> (packets [n, stride] device, results numpy)"""
    n = int(tags.shape[0])
    buf = torch.full((n, T + (4 if inline else 0)), FILL, dtype=torch.uint8, device="cuda")
    res = torch.full((n,), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    tx.emit(tags, out=buf, inline=inline, results=res, held=held)
    return buf, _host(ctx, res)


def _want_raw(ctx, torch, rx, flags, extra, esi_from, cap=None):
    """the C call itself, into a list with four guard words behind it -> (rc, n, the whole buffer as numpy uint32); cap None: the
    count, asked for first with a NULL list"""
    fn = getattr(rx._L, rx._api + "_want")
    n = C.c_uint32(0)
    if cap is None:
        rc = fn(rx._h, flags, extra, esi_from, None, 0, C.byref(n))
        if rc:
            return rc, n.value, None
        cap = n.value
    buf = torch.full((cap + 4,), int(np.uint32(GUARD).view(np.int32)), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = fn(rx._h, flags, extra, esi_from, C.c_void_p(buf.data_ptr()), cap, C.byref(n))
    return rc, n.value, _u32(ctx, buf)


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


def _decodes(orc, src, K, T, esis, what, Kp=0, max_esi=(1 << 24) - 1):
    esis = np.asarray(esis, np.uint32)
    ok, out, _ = orc.decode_block(esis, _oracle_symbols(orc, src, K, T, esis, Kp=Kp), K, T, Kp=Kp, max_esi=max_esi)
    assert ok and np.array_equal(out, src), "the oracle does not decode %s" % what


def _books(K, max_esi, got):
    """(seen, gaps, nrep) in host_want's form of blocks that ADDED exactly the ESIs got[b]"""
    seen = np.zeros((len(got), max_esi + 1), bool)
    for b, es in enumerate(got):
        seen[b, np.asarray(es, np.int64)] = True
    return seen, [int(K - seen[b, :K].sum()) for b in range(len(got))], [int(seen[b, K:].sum()) for b in range(len(got))]


# -------------------------------------------------------------------------------------------- 1. the listing equals the model ----
@pytest.mark.parametrize("name", CASE_NAMES)
def test_listing_equals_the_model(ctx, torch, name):
    case, T = case_of(name), 16
    mod = ModelRx(case.K, T, NBLK, case.rep_cap, sbn0=SBN0, max_esi=case.max_esi, Kp=case.Kp)
    with nanorq_amd.Receiver(ctx, case.K, T, NBLK, rep_cap=case.rep_cap, sbn0=SBN0, max_esi=case.max_esi) as rx:
        for part in np.array_split(case.stream, 2):
            pay = payloads_for(part, T)
            assert np.array_equal(_add(ctx, torch, rx, _dev(torch, pay), tags=part), mod.add(pay, part))
        for source, extra, esi_from in case.queries:
            want = model_want(mod, extra=extra, source=source, esi_from=esi_from)
            rc, n, buf = _want_raw(ctx, torch, rx, WANT_SOURCE if source else 0, extra, esi_from)
            assert rc == 0 and n == len(want), (source, extra, esi_from, n, len(want))
            assert np.array_equal(buf[:n], want), (source, extra, esi_from)
            assert (buf[n:] == GUARD).all(), "guard words"
            assert np.array_equal(_u32(ctx, rx.want(extra=extra, source=source, esi_from=esi_from)), want)


def test_source_listing_past_256_seen_words(ctx, torch):
    """K = 8200, two blocks: 257 seen words per block, so the source listing goes a second round with one live lane and the offset
    of the first"""
    K, T, nblk, sbn0, rep_cap = 8200, 16, 2, 3, 8
    rng = np.random.default_rng(8200)
    mod = ModelRx(K, T, nblk, rep_cap, sbn0=sbn0, Kp=nanorq_amd.params(K)["Kp"])
    tags = []
    for b in range(nblk):
        have = rng.random(K) < 0.5
        have[[b, 8192 + b, K - 1]] = False  # (missing symbols in the first word and in word 256)
        tags += [(sbn0 + b) << 24 | int(e) for e in np.flatnonzero(have)] + [(sbn0 + b) << 24 | (K + 7 * q + b) for q in range(5)]
    tags = np.array(tags, np.uint32)[rng.permutation(len(tags))]
    pay = payloads_for(tags, T)
    with nanorq_amd.Receiver(ctx, K, T, nblk, rep_cap=rep_cap, sbn0=sbn0) as rx:
        for part in np.array_split(np.arange(len(tags)), 2):
            assert np.array_equal(_add(ctx, torch, rx, _dev(torch, pay[part]), tags=tags[part]), mod.add(pay[part], tags[part]))
        want = model_want(mod, source=True)
        assert len(want) == sum(len(mod.lost(b)) for b in range(nblk)) and all(mod.lost(b).max() == K - 1 for b in range(nblk))
        rc, n, buf = _want_raw(ctx, torch, rx, WANT_SOURCE, 0, 0)
        assert rc == 0 and n == len(want) and np.array_equal(buf[:n], want) and (buf[n:] == GUARD).all()
        assert np.array_equal(_u32(ctx, rx.want(source=True)), want)


def test_contract(ctx, torch):
    case = case_of("boundary_K33")
    T = 16
    mod = ModelRx(case.K, T, NBLK, case.rep_cap, sbn0=SBN0, max_esi=case.max_esi, Kp=case.Kp)
    pay = payloads_for(case.stream, T)
    with nanorq_amd.Receiver(ctx, case.K, T, NBLK, rep_cap=case.rep_cap, sbn0=SBN0, max_esi=case.max_esi) as rx:
        assert np.array_equal(_add(ctx, torch, rx, _dev(torch, pay), tags=case.stream), mod.add(pay, case.stream))
        want = model_want(mod, extra=2)
        n = len(want)
        rc, n2, buf = _want_raw(ctx, torch, rx, 0, 2, 0, cap=n - 1)  # too small: refused, the count still given, nothing written
        assert rc == -1 and n2 == n and (buf == GUARD).all()
        rc, n3, buf = _want_raw(ctx, torch, rx, 0, 2, 0, cap=n + 3)
        assert rc == 0 and n3 == n and np.array_equal(buf[:n], want) and (buf[n:] == GUARD).all()
        for flags, extra, esi_from in ((2, 0, 0), (3, 0, 0), (WANT_SOURCE, 1, 0), (WANT_SOURCE, 0, 1), (0, (1 << 24) + 1, 0)):
            assert _want_raw(ctx, torch, rx, flags, extra, esi_from)[0] == -1, (flags, extra, esi_from)
        with pytest.raises(NrqError, match="NRQ_WANT_SOURCE takes neither"):
            rx.want(extra=1, source=True)
        with pytest.raises(NrqError, match="symbols are wanted"):
            cnt = C.c_uint32(0)
            small = torch.zeros(n, dtype=torch.int32, device="cuda")
            ctx._chk(rx._L.nrq_rx_want(rx._h, 0, 2, 0, C.c_void_p(small.data_ptr()), n - 1, C.byref(cnt)))
        # the call only reads the books
        assert np.array_equal(_u32(ctx, rx.want(extra=2)), want)
        # after a reset every block wants all of itself
        rx.reset()
        assert _u32(ctx, rx.want(source=True)).tolist() == [((SBN0 + b) << 24) | e for b in range(NBLK) for e in range(case.K)]


# -------------------------------------------------------------------------------------------- 2. the loop closes on one GPU ----
@pytest.mark.parametrize("T,rep_cap", [(16, 16), (20, 16), (16, 80)])
def test_the_loop_closes(ctx, torch, orc, T, rep_cap):
    """Three blocks of K = 64: block 0 complete, block 1 missing 7 source symbols with 3 repair symbols in, block 2 missing
    everything.  want(extra=2) -> emit -> add: every code ADDED, nothing wanted any more, everything decodes.
    A block that misses all 64 symbols cannot complete through 16 repair rows: with rep_cap = 16 its list is capped at the 16
    free rows (which all come back ADDED, and then it wants no repair symbol), and one more round in source mode -- want(source=True)
    -> emit -> add -- brings the source symbols blocks 1 and 2 still miss; with rep_cap = 80 the repair round alone completes it."""
    K, nblk, sbn0 = 64, 3, 2
    max_esi = 2 * nanorq_amd.params(K)["Kp"]
    src = _blocks(K, T, nblk, seed=T + rep_cap)
    lost1, rep1 = [3, 10, 11, 30, 45, 62, 63], [K + 1, K + 5, K + 2]
    got = [np.arange(K), np.concatenate([np.setdiff1d(np.arange(K), lost1), rep1]), np.zeros(0, np.int64)]
    top = host_want(sbn0, K, max_esi, rep_cap, *_books(K, max_esi, got), extra=2)
    top_e = [top[(top >> 24) == sbn0 + b] & 0xFFFFFF for b in range(nblk)]
    assert top_e[0].tolist() == [] and top_e[1].tolist() == [K, K + 3, K + 4, K + 6, K + 7, K + 8]
    assert top_e[2].tolist() == list(range(K, K + min(K + 2, rep_cap)))
    _decodes(orc, src[1], K, T, np.concatenate([got[1], top_e[1]]), "block 1 after the top-up")
    if rep_cap >= K + 2:
        _decodes(orc, src[2], K, T, top_e[2], "block 2 after the top-up")
    stream = np.concatenate([((sbn0 + b) << 24) | got[b].astype(np.uint32) for b in range(nblk)]).astype(np.uint32)
    rows = np.concatenate([_oracle_symbols(orc, src[b], K, T, got[b]) for b in range(nblk)])
    with nanorq_amd.Sender(ctx, K, T, nblk, _dev(torch, src), sbn0=sbn0) as tx, \
            nanorq_amd.Receiver(ctx, K, T, nblk, rep_cap=rep_cap, sbn0=sbn0) as rx:
        tx.encode()
        assert (_add(ctx, torch, rx, _dev(torch, rows), tags=stream) == ADDED).all()
        tags = rx.want(extra=2)
        assert np.array_equal(_u32(ctx, tags), top)
        pk, res = _emit(ctx, torch, tx, tags, T)
        assert (res == 0).all()
        assert (_add(ctx, torch, rx, pk, tags=tags) == ADDED).all()
        assert rx.want(extra=2).numel() == 0
        if rep_cap < K + 2:
            tags = rx.want(source=True)
            assert _u32(ctx, tags).tolist() == [((sbn0 + 1) << 24) | e for e in lost1] + [((sbn0 + 2) << 24) | e for e in range(K)]
            pk, res = _emit(ctx, torch, tx, tags, T)
            assert (res == 0).all() and (_add(ctx, torch, rx, pk, tags=tags) == ADDED).all()
            assert rx.want(source=True).numel() == 0
        st, _ = rx.decode()
        assert list(st) == [1] * nblk
        assert np.array_equal(_host(ctx, rx.source), src)
        assert rx.want(extra=2).numel() == 0 and rx.want(source=True).numel() == 0  # complete blocks want nothing


# ------------------------------------------------------------------------ 3. source mode against a parent that is not ready ----
def test_source_mode_against_a_parent_that_is_not_ready(ctx, torch, orc):
    K, T, nblk, sbn0 = 64, 16, 2, 3
    src = _blocks(K, T, nblk, seed=31)
    lost_r = [[5, 20, 40], [2, 3, 4]]                        # what the relay R lacks (it has no repair symbols: not ready)
    lost_c = [[1, 5, 9, 20, 33, 63], [0, 2, 4, 6, 8, 10]]    # what the child C lacks
    left = [np.intersect1d(lost_c[b], lost_r[b]) for b in range(nblk)]  # what R cannot give
    assert all(0 < len(left[b]) < len(lost_c[b]) for b in range(nblk))
    final = [np.concatenate([np.setdiff1d(np.arange(K), left[b]), np.arange(K, K + len(left[b]))]) for b in range(nblk)]
    for b in range(nblk):
        _decodes(orc, src[b], K, T, final[b], "block %d of C after both top-ups" % b)

    def stream(lost):
        es = [np.setdiff1d(np.arange(K), lost[b]).astype(np.uint32) for b in range(nblk)]
        return np.concatenate([((sbn0 + b) << 24) | es[b] for b in range(nblk)]).astype(np.uint32), np.concatenate([src[b][es[b]] for b in range(nblk)])

    with nanorq_amd.Sender(ctx, K, T, nblk, _dev(torch, src), sbn0=sbn0) as origin, \
            nanorq_amd.Receiver(ctx, K, T, nblk, rep_cap=16, sbn0=sbn0) as rx_r, rx_r.relay() as relay, \
            nanorq_amd.Receiver(ctx, K, T, nblk, rep_cap=16, sbn0=sbn0) as rx_c:
        origin.encode()
        for rx, lost in ((rx_r, lost_r), (rx_c, lost_c)):
            tg, rows = stream(lost)
            assert (_add(ctx, torch, rx, _dev(torch, rows), tags=tg) == ADDED).all()
        assert not relay.ready().any()
        tags = rx_c.want(source=True)
        th = _u32(ctx, tags)
        assert th.tolist() == [((sbn0 + b) << 24) | e for b in range(nblk) for e in lost_c[b]]
        pk, res = _emit(ctx, torch, relay, tags, T, held=True)
        holds = np.array([(int(t) & 0xFFFFFF) not in lost_r[(int(t) >> 24) - sbn0] for t in th])
        assert np.array_equal(res == 0, holds) and (res[~holds] == TX_NOT_READY).all()
        assert bool((pk[_dev(torch, ~holds)] == FILL).all()), "a packet the relay does not hold was written"
        m = _dev(torch, holds)
        assert (_add(ctx, torch, rx_c, pk[m].contiguous(), tags=tags[m].contiguous()) == ADDED).all()
        assert _u32(ctx, rx_c.want(source=True)).tolist() == [((sbn0 + b) << 24) | int(e) for b in range(nblk) for e in left[b]]
        # repair mode against the origin completes C
        tags = rx_c.want()
        assert _u32(ctx, tags).tolist() == [((sbn0 + b) << 24) | (K + i) for b in range(nblk) for i in range(len(left[b]))]
        pk, res = _emit(ctx, torch, origin, tags, T)
        assert (res == 0).all() and (_add(ctx, torch, rx_c, pk, tags=tags) == ADDED).all()
        assert rx_c.want().numel() == 0
        assert list(rx_c.decode()[0]) == [1] * nblk
        assert np.array_equal(_host(ctx, rx_c.source), src)


# ------------------------------------------------------------------------------------------------------------- 4. objects ----
@pytest.mark.parametrize("flags", [0, EXT_PER_BLOCK_KP])
def test_objects(ctx, torch, orc, flags):
    Kt, T, Z, nrep, rep_cap = 213, 16, 5, 3, 24  # two block classes: 3 blocks of K = 43, 2 of 42; F not a multiple of T
    data = payload(Kt * T - 5, seed=Kt + flags)
    rng = np.random.default_rng(7 + flags)
    with nanorq_amd.ObjectSender(ctx, _dev(torch, data), T, Z=Z, flags=flags) as tx:
        p = tx.params
        assert p.ZL and p.ZS and p.F % T and (p.KpL != p.KpS) == bool(flags & EXT_PER_BLOCK_KP)
        tx.encode()
        n = tx.count_all(nrep)
        t_o = torch.zeros(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        sent = tx.emit_all(nrep, inline=True, tags_out=t_o)
        tags = _u32(ctx, t_o)
        oti, blocks = tx.oti, tx.blocks
        sbn, esi = tags >> 24, tags & 0xFFFFFF
        drop = rng.random(n) < 0.15
        drop |= (sbn == 1) & ((esi >= 43) | (esi % 6 == 1))  # block 1: no repair symbol, a sixth of its source symbols gone
        drop &= ~(sbn == 3)                        # block 3 gets everything: complete
        drop |= (sbn == 0) & np.isin(esi, [0, 7, 42, 43])  # (43: block 0's first repair ESI)
        deliv = np.flatnonzero(~drop)
        rng.shuffle(deliv)
        got = [esi[deliv][sbn[deliv] == b] for b in range(Z)]

        def model(books, **kw):  # per block its class's K, in SBN order
            return np.concatenate([host_want(b, K, p.max_esi, rep_cap, *_books(K, p.max_esi, [books[b]]), **kw) for b, (K, _) in enumerate(blocks)])
        top = model(got, extra=2)
        sent_h = sent.cpu().numpy()
        src_rows = {}
        for b, (K, Kp) in enumerate(blocks):  # the oracle's verdict on the reception after the top-up
            es = np.concatenate([got[b], top[(top >> 24) == b] & 0xFFFFFF]).astype(np.uint32)
            if (got[b] < K).sum() < K:
                src_b = np.zeros((K, T), np.uint8)
                mine = np.flatnonzero((sbn == b) & (esi < K))
                src_b[esi[mine]] = sent_h[mine, 4:4 + T]
                _decodes(orc, src_b, K, T, es, "block %d after the top-up" % b, Kp=Kp, max_esi=p.max_esi)
        with nanorq_amd.ObjectReceiver(ctx, *oti, flags=flags, rep_cap=rep_cap) as rx:
            assert (_add(ctx, torch, rx, sent[_dev(torch, deliv)].contiguous(), inline=True) == ADDED).all()
            assert np.array_equal(rx.counts()[0] == 0, np.arange(Z) == 3)
            for kw in (dict(source=True), dict(), dict(extra=2), dict(extra=2, esi_from=50), dict(extra=40, esi_from=p.max_esi - 1)):
                assert np.array_equal(_u32(ctx, rx.want(**kw)), model(got, **kw)), kw
            rc, nw, buf = _want_raw(ctx, torch, rx, 0, 2, 0)
            assert rc == 0 and np.array_equal(buf[:nw], top) and (buf[nw:] == GUARD).all()
            lst = rx.want(extra=2)
            pk, res = _emit(ctx, torch, tx, lst, T, inline=True)
            assert (res == 0).all() and (_add(ctx, torch, rx, pk, inline=True) == ADDED).all()
            assert rx.want(extra=2).numel() == 0
            assert rx.decode()[0].all()
            assert rx.want(source=True).numel() == 0
            out, left = rx.write()
            assert left == 0 and hashlib.sha256(_host(ctx, out).tobytes()).hexdigest() == hashlib.sha256(data.tobytes()).hexdigest()


# ------------------------------------------------------------------------------------------------------------ 5. esi_from ----
def test_esi_from_keeps_requests_apart(ctx, torch):
    K, T, nblk, sbn0, rep_cap = 64, 16, 3, 1, 32
    src = _blocks(K, T, nblk, seed=5)
    lost = [[1, 2, 3], list(range(0, 20, 2)), [63]]
    es = [np.setdiff1d(np.arange(K), lost[b]).astype(np.uint32) for b in range(nblk)]
    tg = np.concatenate([((sbn0 + b) << 24) | es[b] for b in range(nblk)]).astype(np.uint32)
    with nanorq_amd.Sender(ctx, K, T, nblk, _dev(torch, src), sbn0=sbn0) as tx, \
            nanorq_amd.Receiver(ctx, K, T, nblk, rep_cap=rep_cap, sbn0=sbn0) as rx:
        tx.encode()
        assert (_add(ctx, torch, rx, _dev(torch, np.concatenate([src[b][es[b]] for b in range(nblk)])), tags=tg) == ADDED).all()
        a, b = rx.want(extra=2), rx.want(extra=2, esi_from=K + 32)  # (for two parents: the books are the same for both lists)
        ah, bh = _u32(ctx, a), _u32(ctx, b)
        assert len(ah) == len(bh) == sum(len(x) + 2 for x in lost) and not set(ah.tolist()) & set(bh.tolist())
        assert ((ah & 0xFFFFFF) < K + 32).all() and ((bh & 0xFFFFFF) >= K + 32).all()
        for lst in (a, b):
            pk, res = _emit(ctx, torch, tx, lst, T)
            assert (res == 0).all() and (_add(ctx, torch, rx, pk, tags=lst) == ADDED).all()  # no DUP


# -------------------------------------------------------------------------------------------------------- 6. enqueue order ----
def test_want_then_emit_without_a_host_wait(ctx, torch):
    K, T, nblk, sbn0 = 64, 16, 3, 4
    src = _blocks(K, T, nblk, seed=6)
    es = [np.setdiff1d(np.arange(K), np.arange(b, K, 5 + b)).astype(np.uint32) for b in range(nblk)]
    tg = np.concatenate([((sbn0 + b) << 24) | es[b] for b in range(nblk)]).astype(np.uint32)
    with nanorq_amd.Sender(ctx, K, T, nblk, _dev(torch, src), sbn0=sbn0) as tx, \
            nanorq_amd.Receiver(ctx, K, T, nblk, rep_cap=32, sbn0=sbn0) as rx:
        tx.encode()
        assert (_add(ctx, torch, rx, _dev(torch, np.concatenate([src[b][es[b]] for b in range(nblk)])), tags=tg) == ADDED).all()
        n = int(rx.want(extra=2).numel())
        assert n == sum(K - len(e) + 2 for e in es)
        got = []
        for wait in (False, True):
            tags = torch.full((n,), -1, dtype=torch.int32, device="cuda")  # (all ones: SBN 255, outside the transmission)
            pk = torch.full((n, T), FILL, dtype=torch.uint8, device="cuda")
            res = torch.full((n,), 77, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            cnt = C.c_uint32(0)
            ctx._chk(rx._L.nrq_rx_want(rx._h, 0, 2, 0, C.c_void_p(tags.data_ptr()), n, C.byref(cnt)))
            if wait:
                ctx.sync()
            tx.emit(tags, out=pk, results=res)
            assert (_host(ctx, res) == 0).all()
            got.append((tags.cpu().numpy(), pk.cpu().numpy()))
        assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
        assert not (got[0][1] == FILL).all(axis=1).any()
