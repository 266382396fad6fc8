"""GPU tier of the device-resident receiver (nrq_rx_*, nanorq_amd.Receiver): the ingest kernels against their CPU emulation,
byte for byte (the row tables prefilled and between guard rows, compared whole; nrq_ing_copy_kernel's three forms also at the
symbol sizes that fill a trip of its loop and start the next, each case asserting the form from the addresses it hands over); round trips from packets built on the device to recovered blocks, against the object layer
(nanorq_decoder_add_symbols + nanorq_repair_all) on the same packets in the same order and against the oracle."""
import ctypes as C

import numpy as np
import pytest

import nanorq_amd
from capi import api, mem_io
from rx_support import UNTOUCHED, EmuRx, inline_packets, payloads_for, random_stream
from tx_support import FILL, copy_forms

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
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _state(rx, torch, K, T, nblk, rep_cap, src_t, rep_t):
    lost, reps = rx.lists()
    nl, nr = rx.counts()
    assert list(nl) == [len(x) for x in lost] and list(nr) == [len(x) for x in reps]
    return lost, reps, src_t.cpu().numpy(), rep_t.cpu().numpy()


@pytest.mark.parametrize("inline", [False, True])
@pytest.mark.parametrize("K,T,nblk,sbn0,rep_cap,n", [
    (100, 16, 3, 1, 40, 1), (100, 16, 3, 1, 40, 255), (100, 16, 3, 1, 40, 256), (100, 16, 3, 1, 40, 257),
    (100, 36, 5, 0, 30, 3000),            # 4-byte copies
    (1000, 13, 4, 2, 500, 9000),          # byte copies
    (1000, 64, 2, 0, 20, 70000),          # many tiles, rep_cap overflow, heavy duplication
    (8200, 16, 2, 0, 40, 20000),          # 257 seen words per block: the list fill's second round (one live lane, the offset carried over)
])
def test_device_ingest_matches_emulation(ctx, torch, K, T, nblk, sbn0, rep_cap, n, inline):
    _ingest_against_emulation(ctx, torch, K, T, nblk, sbn0, rep_cap, n, inline,
                              lambda call: T + 4 + 8 * call if inline else T + 16 * call)


def _guarded_rows(torch, nblk, rows, T):
    """[nblk, rows, T] row tables prefilled with FILL, a slice of one tensor with a guard row of FILL before and after it ->
    (the whole tensor, the table)"""
    whole = torch.full((nblk * rows + 2, T), FILL, dtype=torch.uint8, device="cuda")
    return whole, whole[1:-1].view(nblk, rows, T)


def _ingest_against_emulation(ctx, torch, K, T, nblk, sbn0, rep_cap, n, inline, stride_of, forms=None):
    """two Receiver.add calls of a messy stream against the emulated ingest: codes, lists, and the source and repair tables whole,
    rows no packet landed in and the guard rows around the tables included.  forms: the forms of nrq_ing_copy_kernel the packets
    must take, by its rule on the addresses handed over (tx_support.copy_forms)"""
    Kp = nanorq_amd.params(K)["Kp"]
    rng = np.random.default_rng(n + T)
    emu = EmuRx(K, T, nblk, rep_cap, sbn0, Kp=Kp)
    emu.src[:] = FILL
    emu.rep[:] = FILL
    src_w, src_t = _guarded_rows(torch, nblk, K, T)
    rep_w, rep_t = _guarded_rows(torch, nblk, rep_cap, T)
    with nanorq_amd.Receiver(ctx, K, T, nblk, rep_cap, sbn0=sbn0, src=src_t, src_stride=K * T, rep=rep_t, rep_stride=rep_cap * T) as rx:
        for call in range(2):
            tags = random_stream(rng, K, nblk, sbn0, 2 * Kp, n, sbn_span=2)
            pl = payloads_for(tags, T, salt=call)
            stride = stride_of(call)
            if inline:
                pk = inline_packets(pl, tags, stride)
            else:
                pk = np.concatenate([pl, np.zeros((len(tags), stride - T), np.uint8)], axis=1)
            res_d = torch.full((len(tags),), UNTOUCHED, dtype=torch.int32, device="cuda")
            pk_d = _dev(torch, pk)
            if forms is not None:
                assert copy_forms(pk_d.data_ptr(), stride, 4 if inline else 0, len(tags), T, [src_t.data_ptr(), rep_t.data_ptr()]) == forms
            tg_d = None if inline else _dev(torch, tags.view(np.int32))
            torch.cuda.synchronize()
            rx.add(pk_d, tags=tg_d, inline=inline, results=res_d)
            ctx.sync()
            r_emu = emu.add(pk, None if inline else tags)
            if K > 8192:  # (the second round has ESIs to place, behind those of the first)
                assert all(emu.lost(b).min() < 32 and emu.lost(b).max() >= 8192 for b in range(nblk))
            r_dev = res_d.cpu().numpy()
            assert np.array_equal(r_dev, r_emu), np.flatnonzero(r_dev != r_emu)[:10]
            lost, reps, s, r = _state(rx, torch, K, T, nblk, rep_cap, src_t, rep_t)
            for b in range(nblk):
                assert np.array_equal(lost[b], emu.lost(b)) and np.array_equal(reps[b], emu.rep_list(b)), b
            assert np.array_equal(s, emu.src) and np.array_equal(r, emu.rep)
            for w in (src_w, rep_w):
                assert bool((w[0] == FILL).all()) and bool((w[-1] == FILL).all()), "guard rows"
    return emu


# the sizes at which a form of nrq_ing_copy_kernel fills a trip of its loop or starts the next (64 lanes, two accesses in flight:
# 16-byte form 1024 + 1024 bytes a trip, dword form 256 + 256, byte form 64): (T, inline, stride, forms)
COPY_EDGES = [
    (1024, False, 1040, {"v16"}),   # no lane has a second access
    (1040, False, 1056, {"v16"}),   # lane 0 alone has one
    (2048, False, 2064, {"v16"}),   # every lane has one: one whole trip
    (2064, False, 2080, {"v16"}),   # a second trip
    (256, True, 272, {"dword"}),    # behind the 4-byte header (the payload at 4 mod 16): no second access
    (260, True, 264, {"dword"}),    # lane 0 alone
    (512, True, 528, {"dword"}),    # one whole trip
    (516, True, 520, {"dword"}),    # a second trip
    (63, False, 63, {"byte"}),      # 63 lanes
    (65, True, 69, {"byte"}),       # a second trip
    (64, False, 67, {"byte", "dword", "v16"}),  # an odd stride: three packets in four by bytes, exactly one trip; the others land on
                                                # a 4- or 16-byte boundary and take that form (the kernel decides packet by packet)
]


@pytest.mark.parametrize("T,inline,stride,forms", COPY_EDGES, ids=["%d-%s-%d" % c[:3] for c in COPY_EDGES])
def test_device_ingest_copy_at_trip_edges(ctx, torch, T, inline, stride, forms):
    emu = _ingest_against_emulation(ctx, torch, 100, T, 2, 1, 20, 300, inline, lambda call: stride, forms=forms)
    assert (emu.nrep > 0).all() and (emu.gaps < 100).all()  # (source and repair rows were written in every block)


def _packets_on_device(torch, ctx, K, T, nblk, loss, seed, dup=0.03, late=0.01):
    """Encode on the device, drop `loss` of every block's source symbols, send as many repair symbols as were dropped (overhead 0),
    shuffle, duplicate a few per cent and append a few packets after completion.  Returns (src, payload [n, T] tensor, tags)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    src = torch.randint(0, 256, (nblk, K, T), dtype=torch.uint8, generator=g).cuda()
    keep = torch.rand((nblk, K), generator=g) >= loss
    nlost = (~keep).sum(1)
    R = int(nlost.max()) + 4
    rep = torch.empty((nblk, R, T), dtype=torch.uint8, device="cuda")
    ctx.encode_blocks(K, T, nblk, src.data_ptr(), K * T, rep.data_ptr(), R * T, np.arange(K, K + R, dtype=np.uint32))
    ctx.sync()
    bi, ei = torch.nonzero(keep, as_tuple=True)
    rb = torch.repeat_interleave(torch.arange(nblk), nlost)
    rq = torch.cat([torch.arange(int(x)) for x in nlost]) if int(nlost.sum()) else torch.zeros(0, dtype=torch.long)
    # rows of one flat table: source rows first, then repair rows
    flat = torch.cat([src.reshape(-1, T), rep.reshape(-1, T)])
    rows = torch.cat([bi * K + ei, nblk * K + rb * R + rq])
    tags = torch.cat([(bi << 24) | ei, (rb << 24) | (K + rq)])
    perm = torch.randperm(len(rows), generator=g)
    rows, tags = rows[perm], tags[perm]
    nd = int(len(rows) * dup)
    pick = torch.randint(0, len(rows), (nd,), generator=g)
    at = torch.sort(torch.randint(0, len(rows), (nd,), generator=g)).values
    rows = torch.cat([rows, rows[pick]])
    tags = torch.cat([tags, tags[pick]])
    order = torch.argsort(torch.cat([torch.arange(len(perm)) * 2, at * 2 + 1]))  # duplicates after random earlier positions
    rows, tags = rows[order], tags[order]
    nl = max(1, int(len(rows) * late))  # after completion: source ESIs again, and repair ESIs beyond those sent
    lb = torch.randint(0, nblk, (nl,), generator=g)
    le = torch.randint(0, K, (nl,), generator=g)
    rows = torch.cat([rows, lb * K + le])
    tags = torch.cat([tags, (lb << 24) | le])
    payload = flat[rows.cuda()]
    return src, payload, tags.to(torch.int64).numpy().astype(np.uint32)


def _object_decode(K, T, nblk, payload_np, tags):
    """nanorq_decoder_add_symbols + nanorq_repair_all on the same packets: (per-block complete, out [nblk, K, T], results)"""
    L = api()
    enc = L.nanorq_encoder_new_ex(nblk * K * T, T, K, nblk, 8)
    assert enc and L.nanorq_blocks(enc) == nblk and all(L.nanorq_block_symbols(enc, b) == K for b in range(nblk))
    dq = L.nanorq_decoder_new(L.nanorq_oti_common(enc), L.nanorq_oti_scheme_specific(enc))
    L.nanorq_free(enc)
    out = np.zeros(nblk * K * T, np.uint8)
    io = mem_io(out)
    blob = np.ascontiguousarray(payload_np)
    tg = np.ascontiguousarray(tags, np.uint32)
    res = np.zeros(len(tg), np.int32)
    L.nanorq_decoder_add_symbols(dq, blob.ctypes.data_as(C.c_void_p), tg.ctypes.data_as(C.POINTER(C.c_uint32)), len(tg),
                                 res.ctypes.data_as(C.POINTER(C.c_int)), io)
    L.nanorq_repair_all(dq, io)
    done = np.array([L.nanorq_num_missing(dq, b) == 0 for b in range(nblk)])
    L.nanorq_free(dq)
    io.contents.destroy(io)
    return done, out.reshape(nblk, K, T), res


@pytest.mark.parametrize("K,T,nblk,inline", [(100, 64, 6, False), (1000, 48, 4, True), (8192, 1280, 256, False)])
def test_round_trip(ctx, torch, orc, K, T, nblk, inline):
    src, payload, tags = _packets_on_device(torch, ctx, K, T, nblk, 0.1, seed=K)
    n = len(tags)
    rtags = np.unique(tags[(tags & 0xFFFFFF) >= K])
    rep_cap = int(np.bincount(rtags >> 24, minlength=nblk).max()) + 8  # room for every repair symbol sent (the object layer has no cap)
    if inline:
        pk = torch.zeros((n, T + 4), dtype=torch.uint8, device="cuda")
        pk[:, :4] = _dev(torch, tags.astype(">u4").view(np.uint8).reshape(n, 4))
        pk[:, 4:] = payload
    res_d = torch.full((n,), UNTOUCHED, dtype=torch.int32, device="cuda")
    with nanorq_amd.Receiver(ctx, K, T, nblk, rep_cap) as rx:
        if inline:
            rx.add(pk, inline=True, results=res_d)
        else:
            rx.add(payload, tags=_dev(torch, tags.view(np.int32)), results=res_d)
        st, used = rx.decode()
        got = rx.source.cpu().numpy()
        lost_after = rx.counts()[0]
    want = src.cpu().numpy()
    done, o_out, o_res = _object_decode(K, T, nblk, payload.cpu().numpy(), tags)
    assert np.array_equal(res_d.cpu().numpy(), o_res)
    assert np.array_equal(st.astype(bool), done)
    assert st.sum() >= nblk - max(2, nblk // 32), st  # overhead 0: a block is rank deficient with probability ~1/256
    for b in range(nblk):
        if st[b]:
            assert np.array_equal(got[b], want[b]), b
            assert np.array_equal(got[b], o_out[b]), b
            assert lost_after[b] == 0
    # two blocks against the oracle, from the packets each took, in arrival order
    added = o_res == 0
    for b in [int(x) for x in np.flatnonzero(st)[:2]]:
        mine = added & ((tags >> 24) == b)
        esis = tags[mine] & 0xFFFFFF
        ok, r_out, _ = orc.decode_block(esis, payload.cpu().numpy()[mine], K, T)
        assert ok and np.array_equal(r_out, want[b])


def test_round_trip_on_a_default_context(torch, orc):
    """test_round_trip at the product shape on a context with no option set: the launch choices a Receiver user gets"""
    import gpu_support as G
    test_round_trip(G.default_ctx(), torch, orc, 8192, 1280, 256, False)


def _singular_case(K, seed0=1):
    """a loss pattern and as many repair ESIs whose system is rank deficient (host planner), and one more repair ESI"""
    kc = nanorq_amd.host_kconst(K)
    p = nanorq_amd.params(K)
    rng = np.random.default_rng(seed0)
    for _ in range(20000):
        lost = np.sort(rng.choice(K, int(rng.integers(2, 12)), replace=False)).astype(np.uint32)
        r0 = int(rng.integers(K, 2 * K))
        reps = np.arange(r0, r0 + len(lost), dtype=np.uint32)
        isis = np.arange(p["Kp"], dtype=np.uint32)
        isis[lost] = reps + (p["Kp"] - K)
        if nanorq_amd.plan_header(nanorq_amd.host_plan(K, isis, kc))["status"] == 0:
            continue
        extra = r0 + len(lost)
        if nanorq_amd.plan_header(nanorq_amd.host_plan(K, np.append(isis, extra + p["Kp"] - K).astype(np.uint32), kc))["status"] == 0:
            return lost, reps, np.uint32(extra)
    pytest.skip("no rank deficient pattern found")


def test_rank_deficient_then_one_more_packet(ctx, torch):
    K, T = 100, 32
    lost, reps, extra = _singular_case(K)
    src = np.random.default_rng(3).integers(0, 256, (1, K, T), dtype=np.uint8)
    allr = np.concatenate([reps, [extra]]).astype(np.uint32)
    d_src = _dev(torch, src)
    d_rep = torch.empty((1, len(allr), T), dtype=torch.uint8, device="cuda")
    ctx.encode_blocks(K, T, 1, d_src.data_ptr(), K * T, d_rep.data_ptr(), len(allr) * T, allr)
    ctx.sync()
    keep = np.setdiff1d(np.arange(K), lost)
    tags = np.concatenate([keep, reps]).astype(np.uint32)
    payload = torch.cat([d_src[0][torch.from_numpy(keep).cuda()], d_rep[0][:len(reps)]])
    with nanorq_amd.Receiver(ctx, K, T, 1, 32) as rx:
        rx.add(payload, tags=_dev(torch, tags.view(np.int32)))
        st, _ = rx.decode()
        assert st[0] == 0 and rx.counts()[0][0] == len(lost)
        rx.add(d_rep[0][len(reps):], tags=_dev(torch, np.array([extra], np.uint32).view(np.int32)))
        st, used = rx.decode()
        assert st[0] == 1 and used[0] == len(lost) + 1
        assert np.array_equal(rx.source.cpu().numpy(), src)
        res = torch.full((1,), UNTOUCHED, dtype=torch.int32, device="cuda")  # complete now: a late packet is IGN
        rx.add(d_rep[0][:1], tags=_dev(torch, reps[:1].view(np.int32)), results=res)
        assert int(res.cpu()[0]) == 1


def test_several_calls_equal_one(ctx, torch):
    K, T, nblk = 1000, 48, 3
    src, payload, tags = _packets_on_device(torch, ctx, K, T, nblk, 0.1, seed=7, dup=0.05)
    n = len(tags)
    tg = _dev(torch, tags.view(np.int32))
    cuts = [0, 1, 300, 301, n // 2, n - 5, n]
    out = []
    for pieces in ([0, n], cuts):
        res = torch.full((n,), UNTOUCHED, dtype=torch.int32, device="cuda")
        with nanorq_amd.Receiver(ctx, K, T, nblk, 200) as rx:
            for a, b in zip(pieces[:-1], pieces[1:]):
                rx.add(payload[a:b], tags=tg[a:b], results=res[a:b])
            lost, reps = rx.lists()
            src_rows = rx.source.cpu().numpy()
            ctx.sync()
            rr = ctx.download(rx.rep_ptr, nblk * 200 * T).reshape(nblk, 200, T)
            out.append((res.cpu().numpy(), lost, reps, src_rows, [rr[b, :len(reps[b])] for b in range(nblk)]))
    a, b = out
    assert np.array_equal(a[0], b[0])
    for blk in range(nblk):
        assert np.array_equal(a[1][blk], b[1][blk]) and np.array_equal(a[2][blk], b[2][blk])
        assert np.array_equal(a[4][blk], b[4][blk])
        keep = np.setdiff1d(np.arange(K), a[1][blk])
        assert np.array_equal(a[3][blk][keep], b[3][blk][keep])
