"""GPU tier of the packets of several symbols (nrq_*_syms; Sender.emit_syms / emit_range_syms, ObjectSender.emit_all_syms,
Receiver.add_syms, ObjectReceiver.add_syms): the device against the CPU emulation of the same bodies and against the oracle,
byte for byte, on every payload path (asserted through the exported path rule); an object of two block classes; device-only
round trips against the same symbols through the one-symbol calls; a relay; and the arguments the calls refuse."""
import ctypes as C

import numpy as np
import pytest

import nanorq_amd
import rx_support as R
import syms_support as S
import tx_support as X
from tx_support import FILL

pytestmark = pytest.mark.gpu

HI = (1 << 24) - 1


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
    torch.cuda.synchronize()
    return t


# torch and the library each have a HIP runtime of their own, so nothing orders their streams: torch.cuda.synchronize() before
# the library reads what torch wrote, ctx.sync() before torch reads what the library wrote


def _stride(kind, T, G, inline):
    need = G * T + (4 if inline else 0)
    return {"tight": need, "pad4": need + 4, "r16": (need + 15) // 16 * 16}[kind]


def _guarded(torch, n, stride):
    buf = torch.full((n + 2, stride), FILL, dtype=torch.uint8, device="cuda")
    return buf, buf[1:n + 1]


def _guards_whole(buf):
    return bool((buf[0] == FILL).all()) and bool((buf[-1] == FILL).all())


# (T, G, inline, stride kind, emit path, ingest copy word)
ROWS = [
    (64, 16, False, "tight", "TX_V16", 16),        # 16-byte, exactly one trip of the wave per packet
    (48, 3, True, "r16", "TX_V16_SHIFT", 4),       # shifted 16-byte, symbol boundaries inside the run
    (16, 64, True, "r16", "TX_V16_SHIFT", 4),      # one lane per symbol, G at its maximum
    (1040, 2, True, "r16", "TX_V16_SHIFT", 4),     # the boundary in the second trip, the carry across trips
    (1024, 2, False, "tight", "TX_V16", 16),       # two full trips
    (20, 4, False, "tight", "TX_DWORD", 4),        # dwords
    (260, 2, True, "pad4", "TX_DWORD", 4),         # dwords, second trip
    (13, 5, True, "tight", "TX_BYTE", 1),          # bytes
    (65, 2, False, "tight", "TX_BYTE", 1),         # bytes, second trip
    (1280, 1, True, "r16", "TX_V16_SHIFT", 4),     # G = 1: equals emit() byte for byte
]


def _list_cases(K, nblk, sbn0, G, rng):
    """first tags and counts (None: by the rule) of a tag-list emit: full and short packets, every result code"""
    c2 = min(2, G)
    cases = [(R.tag(sbn0, 0), None), (R.tag(sbn0, K - (G + 1) // 2), None), (R.tag(sbn0 + 1, K - 1), None), (R.tag(sbn0 + 1, K), None),
             (R.tag(sbn0, 50), 1), (R.tag(sbn0, K - c2), c2), (R.tag(sbn0 + 1, K + 3), G), (R.tag(sbn0, HI - G + 1), G),
             (R.tag(sbn0, 5), 0), (R.tag(sbn0, 5), G + 1), (R.tag(sbn0, K - 1), 2), (R.tag(sbn0, HI), 2),
             (R.tag(sbn0 + nblk, 1), 1), (R.tag(sbn0 - 1, 1), 1)]
    for _ in range(70):  # more than one wave at any G
        b = int(rng.integers(0, nblk))
        if rng.random() < 0.5:
            e = int(rng.integers(0, K))
            c = int(rng.integers(1, min(G, K - e) + 1))
        else:
            e = int(rng.integers(K, K + 40 - G + 1)) if G <= 40 else K
            c = int(rng.integers(1, G + 1))
        cases.append((R.tag(sbn0 + b, e), c))
    return cases


@pytest.mark.parametrize("T,G,inline,stride_kind,path,_w", ROWS)
def test_device_emit_matches_emulation_and_oracle(ctx, torch, orc, T, G, inline, stride_kind, path, _w):
    K, nblk, sbn0 = 100, 2, 3
    Kp = nanorq_amd.params(K)["Kp"]
    rng = np.random.default_rng(T * 100 + G)
    src = rng.integers(0, 256, (nblk, K * T), dtype=np.uint8)
    reps = list(range(K, K + 64 + 40)) + list(range(HI - G, HI + 1))
    blocks = X.oracle_blocks(orc, src, K, T, Kp, [reps] * nblk)
    inter = np.stack([b[0] for b in blocks])
    seg = [(K, Kp, sbn0, src, inter)]
    hdr = 4 if inline else 0
    stride = _stride(stride_kind, T, G, inline)
    cases = _list_cases(K, nblk, sbn0, G, rng)
    tags = np.array([c[0] for c in cases], np.uint32)
    src_d = _dev(torch, src)
    with nanorq_amd.Sender(ctx, K, T, nblk, src_d, sbn0=sbn0, Kp=Kp) as tx:
        tx.encode()
        rows = [(src_d.data_ptr(), K * T), (tx.inter_ptr, X.params_L(Kp) * T)]
        tg_d = _dev(torch, tags.view(np.int32))
        for given in (True, False):
            nsym = np.array([S.rule(K, int(t) & HI, G) if c is None else c for t, (_, c) in zip(tags, cases)], np.uint8) if given else None
            buf, out = _guarded(torch, len(tags), stride)
            assert S.emit_path(out.data_ptr(), stride, T, inline, rows) == path
            res = torch.full((len(tags),), 77, dtype=torch.int32, device="cuda")
            ns_d = _dev(torch, nsym) if given else None
            tx.emit_syms(tg_d, G, nsym=ns_d, out=out, inline=inline, results=res)
            ctx.sync()
            assert _guards_whole(buf), "guard rows"
            pk_e, res_e = S.emu_emit_table(seg, (sbn0, nblk, nblk), T, G, inline, stride, tags=tags, nsym=nsym)
            pk_d, res_d = out.cpu().numpy(), res.cpu().numpy()
            assert np.array_equal(res_d, res_e)
            if given:
                assert set(res_d.tolist()) == {0, -1, nanorq_amd.TX_BAD_RANGE}
            bad = np.flatnonzero((pk_d != pk_e).any(1))
            assert len(bad) == 0, (bad[:8], tags[bad[:8]])
            for k, t in enumerate(tags):  # the oracle, symbol by symbol
                if res_d[k] != 0:
                    assert (pk_d[k] == FILL).all(), k
                    continue
                c = int(nsym[k]) if given else S.rule(K, int(t) & HI, G)
                b, e = (int(t) >> 24) - sbn0, int(t) & HI
                if inline:
                    assert bytes(pk_d[k, :4]) == int(t).to_bytes(4, "big")
                for i in range(c):
                    assert np.array_equal(pk_d[k, hdr + i * T: hdr + (i + 1) * T], X.expected_payload(src, blocks, K, T, b, e + i)), (k, i)
                assert (pk_d[k, hdr + c * T:] == FILL).all(), k
            if G == 1 and not given:  # emit() byte for byte
                buf1, out1 = _guarded(torch, len(tags), stride)
                res1 = torch.full((len(tags),), 77, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                tx.emit(tg_d, out=out1, inline=inline, results=res1)
                ctx.sync()
                ok = res_d == 0
                assert np.array_equal(out1.cpu().numpy()[ok], pk_d[ok]) and np.array_equal(res1.cpu().numpy()[ok], res_d[ok])
        for interleave in (False, True):
            esi0, n = K - G - 3 if K > G + 3 else 0, 2 * G + 9 + (K if K <= G + 3 else 0)
            npkt = nanorq_amd.pkt_count(K, esi0, n, G) * nblk
            buf, out = _guarded(torch, npkt, stride)
            assert S.emit_path(out.data_ptr(), stride, T, inline, rows) == path
            torch.cuda.synchronize()
            _, tg, ns = tx.emit_range_syms(esi0, n, G, interleave=interleave, inline=inline, out=out)
            ctx.sync()
            assert _guards_whole(buf), "guard rows"
            pk_e, tg_e, ns_e, back = S.emu_emit_table(seg, (sbn0, nblk, nblk), T, G, inline, stride, rng=(esi0, n, n, int(interleave)))
            w_tags, w_cnt = S.range_list([K] * nblk, sbn0, esi0, [n] * nblk, G, interleave)
            assert np.array_equal(tg_e, w_tags) and np.array_equal(ns_e, w_cnt) and np.array_equal(back, np.arange(npkt))
            assert np.array_equal(tg.cpu().numpy().view(np.uint32), tg_e) and np.array_equal(ns.cpu().numpy(), ns_e)
            assert np.array_equal(out.cpu().numpy(), pk_e)


def test_object_of_two_block_classes(ctx, torch):
    """emit_all_syms of an object with KL = KS + 1 (103, 102, 102), T = 48, G = 5, N = 1: the last source packet of each class is
    short; first tags and counts against the restatement, payloads against emit() of the expansion; then ObjectReceiver.add_syms
    with packets of SBN >= Z mixed in, against emit-order expectations, and a decode"""
    T, G, Kt, Z, nrep = 48, 5, 307, 3, 7
    g = torch.Generator().manual_seed(3)
    obj = torch.randint(0, 256, (Kt * T,), dtype=torch.uint8, generator=g).cuda()
    torch.cuda.synchronize()
    with nanorq_amd.ObjectSender(ctx, obj, T, Z=Z) as tx:
        Ks = [k for k, _ in tx.blocks]
        assert Ks == [103, 102, 102]
        tx.encode()
        for interleave in (False, True):
            for inline in (False, True):
                out, tg, ns = tx.emit_all_syms(nrep, G, interleave=interleave, inline=inline)
                ctx.sync()
                w_tags, w_cnt = S.range_list(Ks, 0, 0, [k + nrep for k in Ks], G, interleave)
                tags, cnt = tg.cpu().numpy().view(np.uint32), ns.cpu().numpy()
                assert np.array_equal(tags, w_tags) and np.array_equal(cnt, w_cnt)
                assert len(tags) == tx.count_all_syms(nrep, G) == sum(21 + 2 for _ in Ks)
                slots, sbn, esi = S.expansion(tags, cnt.tolist(), G)
                one = tx.emit(_dev(torch, np.array([R.tag(b, e) for b, e in zip(sbn, esi)], np.uint32).view(np.int32)), inline=inline)
                ctx.sync()
                hdr = 4 if inline else 0
                pk, one = out.cpu().numpy(), one.cpu().numpy()
                for q, s in enumerate(slots):
                    k, i = divmod(int(s), G)
                    assert np.array_equal(pk[k, hdr + i * T: hdr + (i + 1) * T], one[q, hdr:hdr + T]), (k, i)
                    if i == 0 and inline:
                        assert np.array_equal(pk[k, :4], one[q, :4])
        # the receiver: the interleaved inline packets, some whole packets dropped, foreign packets added
        common, specific = tx.oti
        with nanorq_amd.ObjectReceiver(ctx, common, specific, rep_cap=16) as rx:
            p = rx.params
            keep = np.ones(len(tags), bool)
            keep[[1, 30]] = False  # (block 1 and block 0 lose five source symbols each)
            pk_h, tg_h, ns_h = pk[keep], tags[keep], cnt[keep]
            extra_t = np.array([R.tag(Z, 3), R.tag(Z + 1, p.max_esi - 1), R.tag(200, 0)], np.uint32)
            extra_n = np.array([2, 4, 0], np.uint8)
            ex = np.zeros((3, pk_h.shape[1]), np.uint8)
            for j, t in enumerate(extra_t):
                ex[j, :4] = np.frombuffer(int(t).to_bytes(4, "big"), np.uint8)
            pk_h, tg_h, ns_h = np.concatenate([pk_h, ex]), np.concatenate([tg_h, extra_t]), np.concatenate([ns_h, extra_n])
            n0 = len(tg_h) - 3
            emus = [S.EmuRxSyms(p.KL, T, p.ZL, 16, 0, max_esi=p.max_esi), S.EmuRxSyms(p.KS, T, p.ZS, 16, p.ZL, max_esi=p.max_esi)]
            for given in (True, False):
                res = torch.full((len(tg_h) * G,), R.UNTOUCHED, dtype=torch.int32, device="cuda")
                pk_d = _dev(torch, pk_h)
                rx.add_syms(pk_d, G, nsym=_dev(torch, ns_h) if given else None, inline=True, results=res)
                ctx.sync()
                r = res.cpu().numpy().reshape(len(tg_h), G)
                r_emu = np.full(len(tg_h) * G, R.UNTOUCHED, np.int32)
                for e in emus:  # each class's reception over the same packets and results, as the device runs them
                    e.add_syms(pk_h, G, nsym=ns_h if given else None, results=r_emu)
                assert np.array_equal(r[:n0], r_emu.reshape(-1, G)[:n0])
                assert {R.ADDED, R.IGN, R.UNTOUCHED} <= set(r[:n0].reshape(-1).tolist()) if given else R.DUP in r[:n0]
                if given:
                    assert r[n0].tolist() == [R.IGN, R.IGN] + [R.UNTOUCHED] * 3
                    assert r[n0 + 1].tolist() == [R.IGN, R.IGN, R.ERR, R.ERR, R.UNTOUCHED]
                    assert r[n0 + 2].tolist() == [R.ERR] + [R.UNTOUCHED] * 4
                else:
                    assert r[n0].tolist() == [R.IGN] * 5 and r[n0 + 1].tolist() == [R.IGN, R.IGN, R.ERR, R.ERR, R.ERR]
                    assert r[n0 + 2].tolist() == [R.IGN] * 5
            st, _ = rx.decode()
            assert st.all()
            got, left = rx.write()
            ctx.sync()
            assert left == 0 and torch.equal(got, obj)


def _guarded_rows(torch, nblk, rows, T):
    whole = torch.full((nblk * rows + 2, T), FILL, dtype=torch.uint8, device="cuda")
    return whole, whole[1:-1].view(nblk, rows, T)


def _ingest_packets(rng, K, nblk, sbn0, max_esi, n, G, T, hdr, stride, salt, edges):
    tags = R.random_stream(rng, K, nblk, sbn0, max_esi, n, sbn_span=2)
    nsym = rng.integers(1, G + 1, len(tags)).astype(np.uint8)
    if edges:
        c4, c3 = min(4, G), min(3, G)
        edge = [(R.tag(sbn0, 10), c4), (R.tag(sbn0, 12), c4), (R.tag(sbn0 + 1, K - 2), c4), (R.tag(sbn0 + 1, max_esi - 1), c4),
                (R.tag(sbn0 + nblk - 1, HI - 1), c3), (R.tag(sbn0, 20), 0), (R.tag(sbn0, 30), G + 1)]
        tags = np.concatenate([np.array([e[0] for e in edge], np.uint32), tags])
        nsym = np.concatenate([np.array([e[1] for e in edge], np.uint8), nsym])
    pay = []
    for t, c in zip(tags, nsym):
        c = int(c) if 1 <= int(c) <= G else G
        sym = np.array([R.tag(int(t) >> 24, min((int(t) & HI) + i, HI)) for i in range(c)], np.uint32)
        pay.append(R.payloads_for(sym, T, salt).reshape(-1))
    return S.pack(pay, tags, G, T, hdr, stride, fill=0x5A), tags, nsym


def _ingest_against_emulation(ctx, torch, K, T, G, nblk, sbn0, rep_cap, n, inline, stride, word):
    """three add_syms calls of a messy stream (given counts, the rule, given counts) against the emulated ingest: codes, lists,
    and the source and repair tables whole, guard rows included"""
    Kp = nanorq_amd.params(K)["Kp"]
    rng = np.random.default_rng(n + T + G)
    hdr = 4 if inline else 0
    emu = S.EmuRxSyms(K, T, nblk, rep_cap, sbn0, Kp=Kp)
    emu.src[:] = FILL
    emu.rep[:] = FILL
    src_w, src_t = _guarded_rows(torch, nblk, K, T)
    rep_w, rep_t = _guarded_rows(torch, nblk, rep_cap, T)
    with nanorq_amd.Receiver(ctx, K, T, nblk, rep_cap, sbn0=sbn0, src=src_t, src_stride=K * T, rep=rep_t, rep_stride=rep_cap * T) as rx:
        codes = set()
        for call in range(3):
            pk, tags, nsym = _ingest_packets(rng, K, nblk, sbn0, 2 * Kp, n, G, T, hdr, stride, call, edges=call == 0)
            ns = nsym if call != 1 else None
            res_d = torch.full((len(tags) * G,), R.UNTOUCHED, dtype=torch.int32, device="cuda")
            pk_d = _dev(torch, pk)
            assert S.copy_word(pk_d.data_ptr(), stride, hdr, T, [(src_t.data_ptr(), K * T), (rep_t.data_ptr(), rep_cap * T)]) == word
            tg_d = None if inline else _dev(torch, tags.view(np.int32))
            ns_d = None if ns is None else _dev(torch, ns)
            torch.cuda.synchronize()
            rx.add_syms(pk_d, G, tags=tg_d, nsym=ns_d, inline=inline, results=res_d)
            ctx.sync()
            r_emu = emu.add_syms(pk, G, tags=None if inline else tags, nsym=ns)
            r_dev = res_d.cpu().numpy()
            assert np.array_equal(r_dev, r_emu), np.flatnonzero(r_dev != r_emu)[:10]
            codes |= set(r_dev.tolist())
            lost, reps = rx.lists()
            for b in range(nblk):
                assert np.array_equal(lost[b], emu.lost(b)) and np.array_equal(reps[b], emu.rep_list(b)), b
            assert np.array_equal(src_t.cpu().numpy(), emu.src) and np.array_equal(rep_t.cpu().numpy(), emu.rep)
            for w in (src_w, rep_w):
                assert bool((w[0] == FILL).all()) and bool((w[-1] == FILL).all()), "guard rows"
        assert {R.ADDED, R.DUP, R.ERR, R.UNTOUCHED} <= codes


@pytest.mark.parametrize("T,G,inline,stride_kind,_p,word", ROWS)
def test_device_ingest_matches_emulation(ctx, torch, T, G, inline, stride_kind, _p, word):
    _ingest_against_emulation(ctx, torch, 100, T, G, 3, 2, 12, 60, inline, _stride(stride_kind, T, G, inline), word)


def test_device_ingest_three_blocks_and_foreign_sbns(ctx, torch):
    _ingest_against_emulation(ctx, torch, 300, 64, 16, 3, 5, 40, 400, False, 16 * 64, 16)


@pytest.mark.parametrize("K,T,G,nblk", [(100, 64, 16, 3), (1000, 256, 5, 2)])
def test_device_only_round_trip(ctx, torch, K, T, G, nblk):
    """emit_range_syms -> whole packets dropped by a seeded mask -> add_syms -> decode, against the same symbols in the same
    order through emit / add: status, used and source rows are equal"""
    g = torch.Generator().manual_seed(K + G)
    src = torch.randint(0, 256, (nblk, K, T), dtype=torch.uint8, generator=g).cuda()
    nrep = K // 5 + 2 * G
    with nanorq_amd.Sender(ctx, K, T, nblk, src) as tx:
        torch.cuda.synchronize()
        tx.encode()
        pk, tg, ns = tx.emit_range_syms(0, K + nrep, G, interleave=True, inline=True)
        ctx.sync()
        keep = torch.rand(pk.shape[0], generator=g) >= 0.1
        idx = torch.nonzero(keep).flatten().cuda()
        recv, ns_k = pk[idx].contiguous(), ns[idx].contiguous()
        tags, cnt = tg.cpu().numpy().view(np.uint32)[keep.numpy()], ns.cpu().numpy()[keep.numpy()]
        _, sbn, esi = S.expansion(tags, cnt.tolist(), G)
        one_tags = _dev(torch, ((sbn << 24) | esi).astype(np.uint32).view(np.int32))
        one = tx.emit(one_tags, inline=True)
        ctx.sync()
        with nanorq_amd.Receiver(ctx, K, T, nblk, nrep) as rx, nanorq_amd.Receiver(ctx, K, T, nblk, nrep) as rx1:
            rx.add_syms(recv, G, nsym=ns_k, inline=True)
            rx1.add(one, inline=True)
            a, b = rx.lists(), rx1.lists()
            for x, y in zip(a[0] + a[1], b[0] + b[1]):
                assert np.array_equal(x, y)
            st, used = rx.decode()
            st1, used1 = rx1.decode()
            ctx.sync()
            assert np.array_equal(st, st1) and np.array_equal(used, used1)
            assert torch.equal(rx.source, rx1.source)
            assert st.any()
            for blk in np.flatnonzero(st):
                assert torch.equal(rx.source[blk], src[blk])


def test_relay_emits_packets_of_several_symbols(ctx, torch):
    """add_syms -> decode -> relay().emit_syms, fresh repair ESIs included, equal to the original sender's packets; before the
    decode a block that is not ready gives TX_NOT_READY and leaves its packets untouched"""
    K, T, G, nblk = 100, 64, 16, 2
    g = torch.Generator().manual_seed(8)
    src = torch.randint(0, 256, (nblk, K, T), dtype=torch.uint8, generator=g).cuda()
    with nanorq_amd.Sender(ctx, K, T, nblk, src) as tx, nanorq_amd.Receiver(ctx, K, T, nblk, 48) as rx:
        torch.cuda.synchronize()
        tx.encode()
        pk, tg, ns = tx.emit_range_syms(0, K + 32, G, interleave=True, inline=True)
        ctx.sync()
        keep = torch.ones(pk.shape[0], dtype=torch.bool)
        keep[[0, 3]] = False  # a source packet of each block is lost
        idx = torch.nonzero(keep).flatten().cuda()
        recv, ns_k = pk[idx].contiguous(), ns[idx].contiguous()
        torch.cuda.synchronize()
        rx.add_syms(recv, G, nsym=ns_k, inline=True)
        relay = rx.relay()
        want = np.array([R.tag(0, 0), R.tag(1, 96), R.tag(0, K + 200), R.tag(1, K + 500), R.tag(0, K), R.tag(5, 0)], np.uint32)
        want_d = _dev(torch, want.view(np.int32))
        stride = relay.stride_syms(G, True)
        buf, out = _guarded(torch, len(want), stride)
        res = torch.full((len(want),), 77, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        relay.emit_syms(want_d, G, out=out, inline=True, results=res)
        ctx.sync()
        assert res.cpu().tolist() == [nanorq_amd.TX_NOT_READY] * 5 + [-1]
        assert bool((buf == FILL).all())
        with pytest.raises(nanorq_amd.NrqError, match="not ready"):
            relay.emit_range_syms(0, K, G)
        st, _ = rx.decode()
        assert st.all()
        relay.emit_syms(want_d, G, out=out, inline=True, results=res)
        ref = tx.emit_syms(want_d, G, inline=True)
        ctx.sync()
        assert res.cpu().tolist() == [0] * 5 + [-1]
        o, r = out.cpu().numpy(), ref.cpu().numpy()
        for k, c in enumerate([16, 4, 16, 16, 16]):  # ((1, 96): the rule ends the packet at K)
            assert np.array_equal(o[k, :4 + c * T], r[k, :4 + c * T]) and (o[k, 4 + c * T:] == FILL).all(), k
        assert (o[5] == FILL).all()
        assert _guards_whole(buf)
        a, _, _ = relay.emit_range_syms(K - 8, 40, G, inline=True)
        b, _, _ = tx.emit_range_syms(K - 8, 40, G, inline=True)
        ctx.sync()
        am, bm = a.cpu().numpy(), b.cpu().numpy()
        assert np.array_equal(am[:, :4 + 8 * T], bm[:, :4 + 8 * T])
        relay.close()


def test_refusals(ctx, torch):
    """every refusal returns -1 with a text and enqueues nothing (the buffers keep their fill)"""
    K, T, G, nblk = 10, 16, 4, 2
    src = torch.zeros((nblk, K, T), dtype=torch.uint8, device="cuda")
    tags = torch.zeros((4,), dtype=torch.int32, device="cuda")
    out = torch.full((8, 80), FILL, dtype=torch.uint8, device="cuda")
    res = torch.full((16,), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    L = ctx._L
    p, tp, rp = C.c_void_p(out.data_ptr()), C.c_void_p(tags.data_ptr()), C.c_void_p(res.data_ptr())

    def refused(rc, word):
        assert rc == -1
        text = L.nrq_ctx_error(ctx._h).decode()
        assert word in text, text

    with nanorq_amd.Sender(ctx, K, T, nblk, src) as tx:
        with pytest.raises(nanorq_amd.NrqError, match="not encoded"):
            tx.emit_syms(tags, G, out=out)
        tx.encode()
        refused(L.nrq_tx_emit_syms(tx._h, tp, 4, 0, None, p, 80, 0, rp), "G=0")
        refused(L.nrq_tx_emit_syms(tx._h, tp, 4, 65, None, p, 80, 0, rp), "G=65")
        refused(L.nrq_tx_emit_syms(tx._h, tp, 4, G, None, p, G * T - 1, 0, rp), "pkt_stride")
        refused(L.nrq_tx_emit_syms(tx._h, tp, 4, G, None, p, G * T + 3, 1, rp), "pkt_stride")
        refused(L.nrq_tx_emit_syms(tx._h, tp, 4, G, None, p, 80, 8, rp), "unknown flags")
        refused(L.nrq_tx_emit_syms(tx._h, tp, 4, G, None, p, 80, 2, rp), "NRQ_TX_HELD")
        refused(L.nrq_tx_emit_syms(tx._h, tp, 0x7FFFFFFF, G, None, p, 80, 0, rp), "bad tags")
        refused(L.nrq_tx_emit_range_syms(tx._h, 0, 2, G, 2, p, 80, 0, None, None, None), "order")
        refused(L.nrq_tx_emit_range_syms(tx._h, HI, 2, G, 0, p, 80, 0, None, None, None), "2^24")
        refused(L.nrq_tx_emit_range_syms(tx._h, 0, 2, G, 0, p, 80, 2, None, None, None), "NRQ_TX_HELD")
        refused(L.nrq_tx_emit_range_syms(tx._h, 0, 2, 0, 0, p, 80, 0, None, None, None), "G=0")
        assert nanorq_amd.pkt_count(K, 8, 6, G) == 2 and nanorq_amd.pkt_count(K, 0, 0, G) == 0
        with nanorq_amd.Receiver(ctx, K, T, nblk, 4) as rx:
            refused(L.nrq_rx_add_syms(rx._h, p, 80, tp, 4, 0, None, 0, rp), "G=0")
            refused(L.nrq_rx_add_syms(rx._h, p, 80, tp, 4, 65, None, 0, rp), "G=65")
            refused(L.nrq_rx_add_syms(rx._h, p, G * T - 1, tp, 4, G, None, 0, rp), "pkt_stride")
            refused(L.nrq_rx_add_syms(rx._h, p, G * T + 3, None, 4, G, None, 1, rp), "pkt_stride")
            refused(L.nrq_rx_add_syms(rx._h, p, 80, tp, 0x20000000, G, None, 0, rp), "bad packets")
            refused(L.nrq_rx_add_syms(rx._h, p, 80, tp, 4, G, None, 2, rp), "unknown flags")
            refused(L.nrq_rx_add_syms(rx._h, p, 80, tp, 4, G, None, 1, rp), "either")
            refused(L.nrq_rx_add_syms(rx._h, p, 80, None, 4, G, None, 0, rp), "either")
            with pytest.raises(nanorq_amd.NrqError, match="either"):
                rx.add_syms(out, G, tags=tags, inline=True)
            ctx.sync()
            assert bool((out == FILL).all()) and bool((res == 77).all())
            nl, nr = rx.counts()
            assert list(nl) == [K] * nblk and list(nr) == [0] * nblk
            rx.add_syms(out[:4], G, tags=tags, results=res)  # still usable after the refusals
            tx.emit_syms(tags, G, out=out)
            ctx.sync()
            assert res[:4].cpu().tolist() == [R.ADDED] * 4 and res[4:8].cpu().tolist() == [R.DUP] * 4
