"""GPU tier of the listings as runs (Receiver.want_syms / held_syms, ObjectReceiver's; nrq_rx_want_syms / nrq_rx_held_syms) and of the
held emit of packets of several symbols (emit_syms(held=True) on a relay): the device against the CPU emulation of the same bodies
(runs_emu.cpp) and against the ten-line packetisation of the one-symbol lists, word for word; the held emit on every payload path
against the emulation, the table of include/nanorq_hip.h and the one-symbol relay.emit(held=True) bytes; want -> emit -> add ->
decode closed on the device against a twin driven through the one-symbol calls; cut-through forwarding; the refusals."""
import ctypes as C

import numpy as np
import pytest

import nanorq_amd
import rx_support as R
import runs_support as U
import syms_support as S
from test_gpu_syms import ROWS, _stride
from tx_support import FILL
from want_support import NBLK, SBN0, WANT_SOURCE, case as case_of, model_want

pytestmark = pytest.mark.gpu

HI = (1 << 24) - 1
GS = (1, 5, 64)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available()
    return t


@pytest.fixture(scope="module")
def ctx(torch):
    import gpu_support as G
    return G.ctx()


# torch and the library each have a HIP runtime of their own, so nothing orders their streams: torch.cuda.synchronize() before
# the library reads what torch wrote, ctx.sync() before torch reads what the library wrote
def _dev(torch, a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _tags_dev(torch, tags):
    return _dev(torch, np.ascontiguousarray(tags, np.uint32).view(np.int32))


def _host(ctx, t):
    ctx.sync()
    return t.cpu().numpy()


def _u32(ctx, t):
    return _host(ctx, t).view(np.uint32)


def _pair(ctx, pair):
    return _u32(ctx, pair[0]), _host(ctx, pair[1])


def _same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def _list_raw(ctx, torch, rx, name, args, cap=None):
    """the C call itself, into outputs with guards behind them -> (rc, npkt, nsym, tags [cap + 4] uint32, counts [cap + 16] uint8);
    cap None: the counts, asked for first with NULL outputs"""
    fn = getattr(rx._L, rx._api + name)
    npkt, nsym = C.c_uint32(0), C.c_uint32(0)
    if cap is None:
        rc = fn(rx._h, *args, None, None, 0, C.byref(npkt), C.byref(nsym))
        if rc:
            return rc, npkt.value, nsym.value, None, None
        cap = npkt.value
    tg = torch.full((cap + 4,), int(np.uint32(U.GUARD).view(np.int32)), dtype=torch.int32, device="cuda")
    ns = torch.full((cap + 16,), U.GUARD_B, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = fn(rx._h, *args, C.c_void_p(tg.data_ptr()), C.c_void_p(ns.data_ptr()), cap, C.byref(npkt), C.byref(nsym))
    return rc, npkt.value, nsym.value, _u32(ctx, tg), _host(ctx, ns)


def _check_list(ctx, torch, rx, name, args, G, L, K_of, emu_list):
    """one listing of the device against the model (the packetisation of the one-symbol list L) and the emulation"""
    want = U.packetise(L, G, K_of)
    n = len(want[0])
    rc, npkt, nsym, tg, ns = _list_raw(ctx, torch, rx, name, args)
    assert rc == 0 and (npkt, nsym) == (n, len(L)), (name, args, npkt, n, nsym, len(L))
    assert _same((tg[:n], ns[:n]), want), (name, args)
    assert (tg[n:] == U.GUARD).all() and (ns[n:] == U.GUARD_B).all(), "guards behind the outputs"
    assert np.array_equal(U.expanded(tg[:n], ns[:n], G), L)
    if emu_list is not None:
        assert emu_list[0] == 0 and _same(emu_list[3:], want), (name, args)


def _feed(ctx, torch, rx, emu, mod, stream, T):
    for part in np.array_split(stream, 2):
        pay = R.payloads_for(part, T)
        res = torch.full((len(part),), 77, dtype=torch.int32, device="cuda")
        rx.add(_dev(torch, pay), tags=_tags_dev(torch, part), results=res)
        r = _host(ctx, res)
        assert np.array_equal(r, mod.add(pay, part)) and np.array_equal(r, emu.add(pay, tags=part))


# -------------------------------------------------------------------------------------------------------------- listings ----
@pytest.mark.parametrize("name", ["one_word", "boundary_K32", "rounds_source", "rounds_repair"])
def test_listings(ctx, torch, name):
    case, T = case_of(name), 16
    emu = R.EmuRx(case.K, T, NBLK, case.rep_cap, sbn0=SBN0, max_esi=case.max_esi, Kp=case.Kp)
    mod = R.ModelRx(case.K, T, NBLK, case.rep_cap, sbn0=SBN0, max_esi=case.max_esi, Kp=case.Kp)
    with nanorq_amd.Receiver(ctx, case.K, T, NBLK, rep_cap=case.rep_cap, sbn0=SBN0, max_esi=case.max_esi) as rx:
        _feed(ctx, torch, rx, emu, mod, case.stream, T)
        for G in GS:
            for source, extra, esi_from in case.queries:
                flags = WANT_SOURCE if source else 0
                L = model_want(mod, extra=extra, source=source, esi_from=esi_from)
                _check_list(ctx, torch, rx, "_want_syms", (flags, extra, esi_from, G), G, L, lambda sbn: case.K,
                            U.emu_want_syms(emu, G, flags, extra, esi_from))
            _check_list(ctx, torch, rx, "_held_syms", (G,), G, U.model_held(mod), lambda sbn: case.K, U.emu_held_syms(emu, G))
        source, extra, esi_from = case.queries[-1]
        got = _pair(ctx, rx.want_syms(5, extra=extra, source=source, esi_from=esi_from))
        assert _same(got, U.packetise(model_want(mod, extra=extra, source=source, esi_from=esi_from), 5, lambda sbn: case.K))
        assert np.array_equal(U.expanded(*_pair(ctx, rx.held_syms(5)), 5), _u32(ctx, rx.held()))


def test_listing_repair_runs_across_a_round_of_rows(ctx, torch):
    p = U.R600
    emu, mod = U.r600_filled()
    with nanorq_amd.Receiver(ctx, p["K"], p["T"], p["nblk"], rep_cap=p["rep_cap"], sbn0=p["sbn0"], max_esi=1000) as rx:
        e2 = R.EmuRx(p["K"], p["T"], p["nblk"], p["rep_cap"], sbn0=p["sbn0"], max_esi=1000, Kp=p["K"])
        m2 = R.ModelRx(p["K"], p["T"], p["nblk"], p["rep_cap"], sbn0=p["sbn0"], max_esi=1000, Kp=p["K"])
        _feed(ctx, torch, rx, e2, m2, U.r600_stream(), p["T"])
        assert np.array_equal(e2.rep_esi, emu.rep_esi) and np.array_equal(e2.seen, emu.seen)
        L = U.model_held(mod)
        assert np.array_equal(_u32(ctx, rx.held()), L)
        for G in GS:
            _check_list(ctx, torch, rx, "_held_syms", (G,), G, L, lambda sbn: p["K"], U.emu_held_syms(emu, G))
            _check_list(ctx, torch, rx, "_want_syms", (0, 3, 0, G), G, model_want(mod, extra=3), lambda sbn: p["K"], U.emu_want_syms(emu, G, 0, 3, 0))
        # the contract: cap one short, one output alone, G out of range, what nrq_rx_want refuses
        n = len(U.packetise(L, 5, lambda sbn: p["K"])[0])
        rc, npkt, nsym, tg, ns = _list_raw(ctx, torch, rx, "_held_syms", (5,), cap=n - 1)
        assert rc == -1 and (npkt, nsym) == (n, len(L)) and (tg == U.GUARD).all() and (ns == U.GUARD_B).all()
        Lb, one, cnt = rx._L, C.c_uint32(0), torch.zeros(8, dtype=torch.int32, device="cuda")
        ptr = C.c_void_p(cnt.data_ptr())
        for rc in (Lb.nrq_rx_held_syms(rx._h, 0, None, None, 0, C.byref(one), None), Lb.nrq_rx_held_syms(rx._h, 65, None, None, 0, C.byref(one), None),
                   Lb.nrq_rx_held_syms(rx._h, 5, ptr, None, 8, C.byref(one), None), Lb.nrq_rx_held_syms(rx._h, 5, None, ptr, 8, C.byref(one), None),
                   Lb.nrq_rx_held_syms(rx._h, 5, None, None, 0, None, None), Lb.nrq_rx_want_syms(rx._h, 2, 0, 0, 5, None, None, 0, C.byref(one), None),
                   Lb.nrq_rx_want_syms(rx._h, WANT_SOURCE, 1, 0, 5, None, None, 0, C.byref(one), None),
                   Lb.nrq_rx_want_syms(rx._h, 0, 0, 0, 0, None, None, 0, C.byref(one), None)):
            assert rc == -1 and Lb.nrq_ctx_error(ctx._h)
        assert not _host(ctx, cnt).any()


def test_object_listings_and_emit_behind_the_list(ctx, torch):
    """an object of two block classes (103, 102, 102; T = 48, G = 5): class L, then class S, each with its own K -- ESI 102 is a
    source symbol of block 0 and the first repair symbol of blocks 1 and 2, and follows ESI 101 in arrival order in all three; then
    the list enqueued and emit_syms behind it without a host wait"""
    T, G, Kt, Z, nrep = 48, 5, 307, 3, 7
    g = torch.Generator().manual_seed(3)
    obj = torch.randint(0, 256, (Kt * T,), dtype=torch.uint8, generator=g).cuda()
    torch.cuda.synchronize()
    with nanorq_amd.ObjectSender(ctx, obj, T, Z=Z) as tx:
        Ks = [k for k, _ in tx.blocks]
        assert Ks == [103, 102, 102]
        tx.encode()
        n = tx.count_all(nrep)
        t_o = torch.zeros(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        sent = tx.emit_all(nrep, interleave=False, inline=True, tags_out=t_o)
        tags = _u32(ctx, t_o)
        keep = np.ones(n, bool)
        keep[np.isin(tags & HI, [3, 4, 40, 97])] = False
        with nanorq_amd.ObjectReceiver(ctx, *tx.oti, rep_cap=16) as rx:
            rx.add(sent[_dev(torch, np.flatnonzero(keep))].contiguous(), inline=True)

            def K_of(sbn):
                return Ks[sbn]
            for name, args, one in (("_held_syms", (G,), rx.held()), ("_want_syms", (WANT_SOURCE, 0, 0, G), rx.want(source=True)),
                                    ("_want_syms", (0, 4, 0, G), rx.want(extra=4)), ("_want_syms", (0, 4, 105, G), rx.want(extra=4, esi_from=105))):
                _check_list(ctx, torch, rx, name, args, G, _u32(ctx, one), K_of, None)
            tg, ns = _pair(ctx, rx.held_syms(G))
            pk = {int(t): int(c) for t, c in zip(tg, ns)}
            assert pk[R.tag(0, 98)] == 5 and pk[R.tag(0, 103)] == 5 and pk[R.tag(1, 98)] == 4 and pk[R.tag(1, 102)] == 5 and pk[R.tag(2, 102)] == 5
            assert _same(_pair(ctx, rx.want_syms(G, source=True)), ([R.tag(b, e) for b in range(3) for e in (3, 40, 97)], [2, 1, 1] * 3))
            # the list enqueued, the emit behind it on the same stream, no host wait between the two
            rc, npkt, _, _, _ = _list_raw(ctx, torch, rx, "_want_syms", (0, 4, 0, G))
            wt = torch.zeros(npkt, dtype=torch.int32, device="cuda")
            wn = torch.zeros(npkt, dtype=torch.uint8, device="cuda")
            res = torch.full((npkt,), 77, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            got = C.c_uint32(0)
            assert rx._L.nrq_orx_want_syms(rx._h, 0, 4, 0, G, C.c_void_p(wt.data_ptr()), C.c_void_p(wn.data_ptr()), npkt, C.byref(got), None) == 0
            out = tx.emit_syms(wt, G, nsym=wn, inline=True, results=res)
            assert npkt > 0 and got.value == npkt and not _host(ctx, res).any()
            one = tx.emit(_tags_dev(torch, U.expanded(_u32(ctx, wt), _host(ctx, wn), G)), inline=False)
            want = U.from_one_symbol(_host(ctx, one), _u32(ctx, wt), _host(ctx, wn).tolist(), np.zeros(npkt, np.int32), G, T, True, out.shape[1])
            o = _host(ctx, out)
            for k, c in enumerate(_host(ctx, wn)):
                assert np.array_equal(o[k, :4 + c * T], want[k, :4 + c * T]), k


# ------------------------------------------------------------------------------------------------------------ held emit ----
def _mixed_relay(ctx, torch, T, G, rep_cap=5 * 64 + 8):
    """the relay in three states over K = 100, nblk = 3 at SBN 9 (block 0 ready, block 1 complete but not ready, block 2 partial)
    and its mirror in the emulation -> (sender, receiver, relay, emu, held sets per block, intermediate symbols as the device has them)"""
    K, nblk, sbn0 = U.K3, U.NB3, U.S3
    g = torch.Generator().manual_seed(T * 100 + G)
    src = torch.randint(0, 256, (nblk, K, T), dtype=torch.uint8, generator=g).cuda()
    torch.cuda.synchronize()
    Kp = nanorq_amd.params(K)["Kp"]
    tx = nanorq_amd.Sender(ctx, K, T, nblk, src, sbn0=sbn0)
    tx.encode()
    rx = nanorq_amd.Receiver(ctx, K, T, nblk, rep_cap=rep_cap, sbn0=sbn0, max_esi=U.MAXE3)
    emu = R.EmuRx(K, T, nblk, rep_cap, sbn0=sbn0, max_esi=U.MAXE3, Kp=Kp)
    stream = U.mixed_stream(G)

    def add(b):
        tags = np.array([R.tag(sbn0 + b, e) for e in stream[b]], np.uint32)
        pk = tx.emit(_tags_dev(torch, tags))
        res = torch.full((len(tags),), 77, dtype=torch.int32, device="cuda")
        ctx.sync()
        rx.add(pk, tags=_tags_dev(torch, tags), results=res)
        assert not _host(ctx, res).any()
        assert not emu.add(_host(ctx, pk), tags=tags).any()
    add(1)
    assert list(rx.decode()[0]) == [0, 1, 0]
    relay = rx.relay()
    add(0)
    assert list(rx.decode()[0]) == [1, 1, 0] and list(relay.ready()) == [True, False, False]
    add(2)  # (its symbols would decode: nobody asks)
    src_h = _host(ctx, src)
    for b in (0, 1):  # what the decode did to the rows and the books
        emu.src[b, U.LOST3[b]] = src_h[b, U.LOST3[b]]
        emu.mark_complete(b)
    got2 = [e for e in range(K) if e not in U.LOST3[2]]  # (rows nothing was written to hold whatever the pool left there)
    src_d = _host(ctx, rx.source)
    assert np.array_equal(src_d[:2], emu.src[:2]) and np.array_equal(src_d[2, got2], emu.src[2, got2])
    Lr = nanorq_amd.params(Kp)["L"]
    inter = ctx.download(relay.inter_ptr, nblk * Lr * T).reshape(nblk, Lr, T)
    held = [set(range(K)) | set(stream[b]) if b < 2 else set(stream[b]) for b in range(nblk)]
    return tx, rx, relay, emu, held, inter


@pytest.mark.parametrize("T,G,inline,stride_kind,path,_w", [r for r in ROWS if r[1] != 1])
def test_held_emit_payload_paths(ctx, torch, T, G, inline, stride_kind, path, _w):
    tx, rx, relay, emu, held, inter = _mixed_relay(ctx, torch, T, G)
    try:
        Kp = nanorq_amd.params(U.K3)["Kp"]
        span, ready = (U.S3, U.NB3, U.NB3), np.array([True, False, False])
        stride = _stride(stride_kind, T, G, inline)
        packets = U.mixed_packets(G)
        tags = np.array([a for a, _ in packets], np.uint32)
        tg_d = _tags_dev(torch, tags)
        for given in (True, False):
            counts = U.counts_of(packets, G) if given else [S.rule(U.K3, int(a) & HI, G) for a in tags]
            nsym = np.array(counts, np.uint8) if given else None
            buf = torch.full((len(tags) + 2, stride), FILL, dtype=torch.uint8, device="cuda")
            out = buf[1:-1]
            res = torch.full((len(tags),), 77, dtype=torch.int32, device="cuda")
            rows = [(rx.src_ptr, U.K3 * T), (relay.inter_ptr, nanorq_amd.params(Kp)["L"] * T), (rx.rep_ptr, emu.rep_cap * T)]
            assert S.emit_path(out.data_ptr(), stride, T, inline, rows) == path
            ns_d = _dev(torch, nsym) if given else None
            torch.cuda.synchronize()
            relay.emit_syms(tg_d, G, nsym=ns_d, out=out, inline=inline, results=res, held=True)
            pk_d, res_d = _host(ctx, out), _host(ctx, res)
            assert bool((buf[0] == FILL).all()) and bool((buf[-1] == FILL).all()), "guard rows"
            assert np.array_equal(res_d, U.table(tags, counts, G, lambda b: held[b], ready))
            if given:
                assert set(res_d.tolist()) == {0, U.FOREIGN, U.NOT_READY, U.BAD_RANGE}
            pk_e, res_e = U.emu_emit_held_syms([emu], [Kp], [inter], span, ready, tags, nsym, G, inline, stride)
            assert np.array_equal(res_d, res_e)
            bad = np.flatnonzero((pk_d != pk_e).any(1))
            assert len(bad) == 0, (given, bad[:8], tags[bad[:8]])
            # the one-symbol held emit of the expansion of what was written: the same bytes, everything else keeps its fill
            one_tags = U.expanded(tags[res_d == 0], [c for c, r in zip(counts, res_d) if r == 0], G)
            one_res = torch.full((len(one_tags),), 77, dtype=torch.int32, device="cuda")
            one = relay.emit(_tags_dev(torch, one_tags), results=one_res, held=True)
            assert not _host(ctx, one_res).any()
            assert np.array_equal(pk_d, U.from_one_symbol(_host(ctx, one), tags, counts, res_d, G, T, inline, stride))
        # without the flag the call gives what it gave: the several-symbol emit's own emulation under the same ready mask
        counts = U.counts_of(packets, G)
        out0 = torch.full((len(tags), stride), FILL, dtype=torch.uint8, device="cuda")
        res0 = torch.full((len(tags),), 77, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        relay.emit_syms(tg_d, G, nsym=_dev(torch, np.array(counts, np.uint8)), out=out0, inline=inline, results=res0)
        seg = [(U.K3, Kp, U.S3, emu.src.reshape(U.NB3, -1), inter)]
        pk0, r0 = S.emu_emit_table(seg, span, T, G, inline, stride, tags=tags, nsym=np.array(counts, np.uint8), ready=U.mask_words(ready))
        assert np.array_equal(_host(ctx, res0), r0) and np.array_equal(_host(ctx, out0), pk0)
    finally:
        relay.close()
        rx.close()
        tx.close()


@pytest.mark.parametrize("inline,slack,mode", [(False, 0, "TX_V16"), (True, 12, "TX_V16_SHIFT"), (True, 0, "TX_DWORD"), (False, 3, "TX_BYTE")])
def test_object_relay_held_emit_modes(ctx, torch, inline, slack, mode):
    """nrq_emit_held_syms_kernel<MODE, true> (an object relay's table of two block classes) in each of its four modes: what
    held_syms lists comes back whole and byte for byte as the one-symbol held emit of its expansion; a packet with a symbol the
    reception lacks stays untouched"""
    from tx_support import emit_mode
    Kt, T, Z, nrep, G = 213, 64, 5, 8, 5
    rng = np.random.default_rng(slack + int(inline))
    obj = _dev(torch, rng.integers(0, 256, Kt * T - 37, dtype=np.uint8))
    with nanorq_amd.ObjectSender(ctx, obj, T, Z=Z) as tx:
        assert tx.params.ZL and tx.params.ZS
        tx.encode()
        n = tx.count_all(nrep)
        t_o = torch.zeros(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        sent = tx.emit_all(nrep, interleave=False, inline=True, tags_out=t_o)
        tags = _u32(ctx, t_o)
        oti = tx.oti
    got = rng.random(n) >= 0.3
    got[(tags & HI) == 0] = False  # (no block is complete)
    with nanorq_amd.ObjectReceiver(ctx, *oti, rep_cap=nrep) as rx, rx.relay() as relay:
        rx.add(sent[_dev(torch, np.flatnonzero(got))].contiguous(), inline=True)
        assert not relay.ready().any()
        tg, ns = rx.held_syms(G)
        lt, ln = _pair(ctx, (tg, ns))
        assert np.array_equal(U.expanded(lt, ln, G), tags[got]) and ((lt & HI) >= 43).any() and (ln > 1).any()
        # behind the list: packets that reach one symbol past a run (not held), a foreign SBN
        over = [(int(t), int(c) + 1) for t, c in zip(lt, ln) if c < G and (int(t) & HI) + c not in (42, 43)][:6]
        ask_t = np.concatenate([lt, [a for a, _ in over], [R.tag(Z, 0)]]).astype(np.uint32)
        ask_n = np.concatenate([ln, [c for _, c in over], [1]]).astype(np.uint8)
        off = 4 if inline else 0
        stride = G * T + off + slack
        buf = torch.full((len(ask_t) + 2, stride), FILL, dtype=torch.uint8, device="cuda")
        out = buf[1:-1]
        res = torch.full((len(ask_t),), 77, dtype=torch.int32, device="cuda")
        assert emit_mode(out.data_ptr(), stride, T, off) == mode
        torch.cuda.synchronize()
        relay.emit_syms(_tags_dev(torch, ask_t), G, nsym=_dev(torch, ask_n), out=out, inline=inline, results=res, held=True)
        r, pk = _host(ctx, res), _host(ctx, out)
        nl = len(lt)
        assert not r[:nl].any() and len(over) and (r[nl:-1] == nanorq_amd.TX_NOT_READY).all() and r[-1] == -1
        assert bool((buf[0] == FILL).all()) and bool((buf[-1] == FILL).all()), "guard rows"
        one = relay.emit(_tags_dev(torch, tags[got]), held=True)
        assert np.array_equal(pk, U.from_one_symbol(_host(ctx, one), ask_t, ask_n.tolist(), r, G, T, inline, stride))
        sent_h = _host(ctx, sent)
        assert np.array_equal(_host(ctx, one), sent_h[got, 4:4 + T])


# ------------------------------------------------------------------------------------------------------------- the loop ----
def _books(ctx, rx, T):
    """the lists and the rows that hold a symbol (the others hold whatever the pool left there: zeroed here)"""
    lost, reps = rx.lists()
    src = _host(ctx, rx.source).copy()
    rows = ctx.download(rx.rep_ptr, rx.nblk * rx.rep_cap * T).reshape(rx.nblk, rx.rep_cap, T).copy()
    for b in range(rx.nblk):
        src[b, lost[b].astype(np.int64)] = 0
        rows[b, len(reps[b]):] = 0
    return [x.tolist() for x in lost], [x.tolist() for x in reps], src, rows


@pytest.mark.parametrize("K,T,G", [(100, 64, 16), (1000, 256, 5)])
def test_the_loop_closes_in_packets(ctx, torch, K, T, G):
    """parent: a relay with partial blocks (whole packets of G lost on its way in); child: an empty reception.
    want_syms(source) -> emit_syms(held) -> add_syms, then repair mode with extra = 1 against the parent once it is ready -> decode;
    a twin child goes through want -> emit(held) -> add.  Books, rows, verdicts and the final held() are equal."""
    nblk, rep_cap = 2, K // 5 + 2 * G
    g = torch.Generator().manual_seed(K + G)
    src = torch.randint(0, 256, (nblk, K, T), dtype=torch.uint8, generator=g).cuda()
    torch.cuda.synchronize()
    with nanorq_amd.Sender(ctx, K, T, nblk, src) as tx, nanorq_amd.Receiver(ctx, K, T, nblk, rep_cap) as parent, \
            nanorq_amd.Receiver(ctx, K, T, nblk, rep_cap) as child, nanorq_amd.Receiver(ctx, K, T, nblk, rep_cap) as twin:
        tx.encode()
        pk, tg, ns = tx.emit_range_syms(0, K, G, interleave=True, inline=True)
        ctx.sync()
        keep = torch.rand(pk.shape[0], generator=g) >= 0.15
        keep[[0, 1]] = False  # (interleaved: the first packet of either block, so that both are partial and both get decoded)
        idx = torch.nonzero(keep).flatten().cuda()
        torch.cuda.synchronize()
        parent.add_syms(pk[idx].contiguous(), G, nsym=ns[idx].contiguous(), inline=True)
        with parent.relay() as relay:
            assert not relay.ready().any()

            def by_packets(rx, frm, **kw):
                t, c = rx.want_syms(G, **kw)
                res = torch.full((t.shape[0],), 77, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                out = frm.emit_syms(t, G, nsym=c, results=res, held=True)
                ctx.sync()
                ok = torch.nonzero(res == 0).flatten()
                torch.cuda.synchronize()
                rx.add_syms(out[ok].contiguous(), G, tags=t[ok].contiguous(), nsym=c[ok].contiguous())
                return _host(ctx, res)

            def by_symbols(rx, frm, **kw):
                t = rx.want(**kw)
                res = torch.full((t.shape[0],), 77, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                out = frm.emit(t, results=res, held=True)
                ctx.sync()
                ok = torch.nonzero(res == 0).flatten()
                torch.cuda.synchronize()
                rx.add(out[ok].contiguous(), tags=t[ok].contiguous())
                return _host(ctx, res)
            r1, r2 = by_packets(child, relay, source=True), by_symbols(twin, relay, source=True)
            assert set(r1.tolist()) == {0, nanorq_amd.TX_NOT_READY} and (r2 == 0).sum() == int(_host(ctx, ns)[keep.numpy()].sum())
            a, b = _books(ctx, child, T), _books(ctx, twin, T)
            assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]) and any(a[0])
            # the parent tops itself up at the origin and decodes with the relay attached: ready
            t, c = parent.want_syms(G, extra=1)
            torch.cuda.synchronize()
            parent.add_syms(tx.emit_syms(t, G, nsym=c), G, tags=t, nsym=c)
            assert parent.decode()[0].all() and relay.ready().all()
            r1, r2 = by_packets(child, relay, extra=1), by_symbols(twin, relay, extra=1)
            assert len(r1) and not r1.any() and not r2.any()
            (st, used), (st1, used1) = child.decode(), twin.decode()
            assert np.array_equal(st, st1) and np.array_equal(used, used1) and st.all()
            a, b = _books(ctx, child, T), _books(ctx, twin, T)
            assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
            assert np.array_equal(a[2], _host(ctx, src))
            assert np.array_equal(_u32(ctx, child.held()), _u32(ctx, twin.held()))


def test_cut_through(ctx, torch):
    """held_syms(G) after each of two ingest batches, forwarded with emit_syms(held=True): every result is 0 and the grandchild ends
    up holding what the relay holds, in the relay's order"""
    K, T, G, nblk, rep_cap = 100, 64, 16, 2, 48
    g = torch.Generator().manual_seed(5)
    src = torch.randint(0, 256, (nblk, K, T), dtype=torch.uint8, generator=g).cuda()
    torch.cuda.synchronize()
    with nanorq_amd.Sender(ctx, K, T, nblk, src) as tx, nanorq_amd.Receiver(ctx, K, T, nblk, rep_cap) as rx, \
            nanorq_amd.Receiver(ctx, K, T, nblk, rep_cap) as grand, rx.relay() as relay:
        tx.encode()
        pk, tg, ns = tx.emit_range_syms(0, K + 24, G, interleave=True, inline=True)
        ctx.sync()
        keep = torch.ones(pk.shape[0], dtype=torch.bool)
        keep[[0, 1, 2, 3, 6, 9]] = False  # (neither block completes: more source symbols are lost than repair symbols sent)
        idx = torch.nonzero(keep).flatten()
        for part in (idx[: len(idx) // 2], idx[len(idx) // 2:]):
            part = part.cuda()
            torch.cuda.synchronize()
            rx.add_syms(pk[part].contiguous(), G, nsym=ns[part].contiguous(), inline=True)
            t, c = rx.held_syms(G)
            res = torch.full((t.shape[0],), 77, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            out = relay.emit_syms(t, G, nsym=c, results=res, held=True)
            grand.add_syms(out, G, tags=t, nsym=c)
            assert t.shape[0] and not _host(ctx, res).any()
        assert not relay.ready().any()
        assert np.array_equal(_u32(ctx, grand.held()), _u32(ctx, rx.held()))
        a, b = _books(ctx, rx, T), _books(ctx, grand, T)
        assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and all(a[0]) and all(a[1])


# ------------------------------------------------------------------------------------------------------------- refusals ----
def test_refusals(ctx, torch):
    """a plain sender and an object sender refuse the flag with a text that names it, the range forms refuse it on a relay too, and
    nothing is enqueued"""
    K, T, G, nblk = 10, 16, 4, 2
    src = torch.zeros((nblk, K, T), dtype=torch.uint8, device="cuda")
    tags = torch.zeros((4,), dtype=torch.int32, device="cuda")
    out = torch.full((8, 80), FILL, dtype=torch.uint8, device="cuda")
    res = torch.full((8,), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    L = ctx._L
    p = C.c_void_p(out.data_ptr())

    def refused(rc):
        assert rc == -1 and "NRQ_TX_HELD" in L.nrq_ctx_error(ctx._h).decode()
    with nanorq_amd.Sender(ctx, K, T, nblk, src) as tx, nanorq_amd.ObjectSender(ctx, src.view(-1), T, Z=2) as otx:
        tx.encode()
        otx.encode()
        for s in (tx, otx):
            with pytest.raises(nanorq_amd.NrqError, match="NRQ_TX_HELD"):
                s.emit_syms(tags, G, out=out, results=res, held=True)
        refused(L.nrq_tx_emit_range_syms(tx._h, 0, 2, G, 0, p, 80, 2, None, None, None))
        refused(L.nrq_otx_emit_all_syms(otx._h, 1, G, 0, p, 80, 2, None, None, None))
        with nanorq_amd.Receiver(ctx, K, T, nblk, 4) as rx, rx.relay() as relay:
            pk = tx.emit_range(0, K, interleave=False)
            ctx.sync()
            rx.add(pk, tags=_tags_dev(torch, np.array([R.tag(b, e) for b in range(nblk) for e in range(K)], np.uint32)))
            relay.encode()
            assert relay.ready().all()
            refused(L.nrq_tx_emit_range_syms(relay._h, 0, 2, G, 0, p, 80, 2, None, None, None))
            ctx.sync()
            assert bool((out == FILL).all()) and bool((res == 77).all())
            relay.emit_syms(tags, G, out=out, results=res, held=True)  # (a ready relay takes the flag: the packets of a plain emit)
            ref = tx.emit_syms(tags, G)
            assert not _host(ctx, res)[:4].any() and np.array_equal(_host(ctx, out)[:4, :G * T], _host(ctx, ref)[:, :G * T])
