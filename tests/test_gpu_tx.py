"""GPU tier of the device-resident sender (nrq_tx_*, nanorq_amd.Sender): packets written on the device against the CPU emulation
of the same kernel bodies and against the oracle, byte for byte; against nanorq_encode of the object layer for an object with
two block classes; device-only round trips Sender -> loss -> Receiver -> decode up to the headline size; a per-block fountain
top-up built in torch; and the arguments the calls refuse."""
import ctypes as C

import numpy as np
import pytest

import nanorq_amd
from capi import api, mem_io
from tx_support import FILL, check_packets, emit_mode, emu_emit, emu_emit_range, oracle_blocks, params_L, random_tags, range_tags

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
    torch.cuda.synchronize()
    return t


# torch and the library each have a HIP runtime of their own, so nothing orders their streams: torch.cuda.synchronize() before
# the library reads what torch wrote, ctx.sync() before torch reads what the library wrote


def _stride(kind, T, inline):
    need = T + (4 if inline else 0)
    return {"tight": need, "pad4": need + 4, "r16": (need + 15) // 16 * 16, "odd": need + 3 if need % 2 == 0 else need + 2}[kind]


def _guarded(torch, n, stride):
    """n packet rows prefilled with FILL between two guard rows of one tensor -> (the whole tensor, the rows)"""
    buf = torch.full((n + 2, stride), FILL, dtype=torch.uint8, device="cuda")
    return buf, buf[1:n + 1]


def _guards_whole(buf):
    return bool((buf[0] == FILL).all()) and bool((buf[-1] == FILL).all())


# the instance nrq_emit_kernel<MODE, false> each case below is listed for, by (T, stride kind, inline)
MODES = {(48, "tight", False): "TX_V16", (48, "r16", True): "TX_V16_SHIFT", (1280, "r16", True): "TX_V16_SHIFT",
         (1280, "pad4", True): "TX_DWORD", (16, "r16", True): "TX_V16_SHIFT", (20, "tight", False): "TX_DWORD",
         (13, "tight", True): "TX_BYTE", (48, "odd", False): "TX_BYTE",
         (1024, "r16", True): "TX_V16_SHIFT", (1040, "r16", True): "TX_V16_SHIFT", (1024, "tight", False): "TX_V16",
         (2064, "tight", False): "TX_V16", (256, "pad4", True): "TX_DWORD", (260, "tight", False): "TX_DWORD",
         (65, "tight", False): "TX_BYTE", (64, "odd", False): "TX_BYTE"}


# (T, stride kind, inline): the 16-byte path (tag mode and under an inline header), the 4-byte path, the byte path
@pytest.mark.parametrize("K,T,nblk,sbn0,kp_of,stride_kind,inline", [
    (100, 48, 3, 5, None, "tight", False),   # 16-byte
    (100, 48, 3, 5, None, "r16", True),      # 16-byte, payload shifted across the lanes
    (1000, 1280, 2, 0, None, "r16", True),   # two rounds of the wave per packet (the carry of lane 63)
    (1000, 1280, 2, 0, None, "pad4", True),  # 4-byte
    (100, 16, 2, 1, 1000, "r16", True),      # an object's larger K'
    (100, 20, 4, 254 - 3, None, "tight", False),  # 4-byte, T not a multiple of 16, SBNs up to 255
    (300, 13, 3, 0, None, "tight", True),    # bytes: T odd
    (300, 48, 3, 0, None, "odd", False),     # bytes: odd stride
    # the edges of a wave's round (64 lanes of 16, 4 or 1 bytes)
    (100, 1024, 2, 0, None, "r16", True),    # shifted 16-byte: a full wave, the tail from lane 63, a carry computed and never used
    (100, 1040, 2, 0, None, "r16", True),    # a second round of one live lane whose left neighbour is the carry
    (100, 1024, 2, 0, None, "tight", False),  # 16-byte: exactly one round
    (100, 2064, 2, 0, None, "tight", False),  # a third round of one lane
    (100, 256, 2, 0, None, "pad4", True),    # 4-byte: exactly one round
    (100, 260, 2, 0, None, "tight", False),  # a second round of one lane
    (100, 65, 2, 0, None, "tight", False),   # bytes: a second round
    (100, 64, 2, 0, None, "odd", False),     # exactly one round
])
def test_device_emit_matches_emulation(ctx, torch, orc, K, T, nblk, sbn0, kp_of, stride_kind, inline):
    Kp = nanorq_amd.params(kp_of or K)["Kp"]
    rng = np.random.default_rng(K + T)
    src = rng.integers(0, 256, (nblk, K * T), dtype=np.uint8)
    tags = random_tags(rng, K, nblk, sbn0, 700)
    reps = [[int(t) & 0xFFFFFF for t in tags if (int(t) >> 24) == sbn0 + b and (int(t) & 0xFFFFFF) >= K] for b in range(nblk)]
    # the range calls' ESIs too: 0 .. K+9 of every block
    reps = [r + list(range(K, K + 10)) for r in reps]
    blocks = oracle_blocks(orc, src, K, T, Kp, reps)
    inter = np.stack([b[0] for b in blocks])
    stride = _stride(stride_kind, T, inline)
    src_d = _dev(torch, src)
    with nanorq_amd.Sender(ctx, K, T, nblk, src_d, sbn0=sbn0, Kp=Kp) as tx:
        tx.encode()
        buf, out = _guarded(torch, len(tags), stride)
        rows = [(src_d.data_ptr(), K * T), (tx.inter_ptr, params_L(Kp) * T)]
        assert emit_mode(out.data_ptr(), stride, T, 4 if inline else 0, rows) == MODES[T, stride_kind, inline]
        res = torch.full((len(tags),), 77, dtype=torch.int32, device="cuda")
        tg_d = _dev(torch, tags.view(np.int32))
        tx.emit(tg_d, out=out, inline=inline, results=res)
        ctx.sync()
        assert _guards_whole(buf), "guard rows"
        pk_e, res_e = emu_emit(K, Kp, T, src, inter, tags, inline, stride, sbn0=sbn0)
        pk_d, res_d = out.cpu().numpy(), res.cpu().numpy()
        assert np.array_equal(res_d, res_e)
        bad = np.flatnonzero((pk_d != pk_e).any(1))
        assert len(bad) == 0, (bad[:8], tags[bad[:8]])
        check_packets(pk_d, tags, src, blocks, K, T, nblk, sbn0, inline, res_d)
        d_inter = ctx.download(tx.inter_ptr, inter.nbytes).reshape(inter.shape)
        assert np.array_equal(d_inter, inter)
        for interleave in (False, True):
            n = K + 10
            buf, out = _guarded(torch, n * nblk, stride)
            assert emit_mode(out.data_ptr(), stride, T, 4 if inline else 0, rows) == MODES[T, stride_kind, inline]
            tg = torch.zeros((n * nblk,), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            tx.emit_range(0, n, interleave=interleave, inline=inline, out=out, tags_out=tg)
            ctx.sync()
            assert _guards_whole(buf), "guard rows"
            pk_r, tg_r = emu_emit_range(K, Kp, T, src, inter, 0, n, interleave, inline, stride, sbn0=sbn0)
            assert np.array_equal(tg.cpu().numpy().view(np.uint32), tg_r)
            assert np.array_equal(tg_r, range_tags(nblk, sbn0, 0, n, interleave))
            assert np.array_equal(out.cpu().numpy(), pk_r)


def test_default_output_and_stride(ctx, torch):
    K, T, nblk = 10, 24, 2
    src = _dev(torch, np.random.default_rng(1).integers(0, 256, (nblk, K, T), dtype=np.uint8))
    with nanorq_amd.Sender(ctx, K, T, nblk, src) as tx:
        tx.encode()
        torch.cuda.synchronize()
        a = tx.emit_range(0, 12, inline=True)
        b = tx.emit_range(0, 12)
        assert tuple(a.shape) == (24, 32) and tuple(b.shape) == (24, T)
        ctx.sync()
        assert torch.equal(a[:, 4:4 + T], b)
        assert torch.equal(b[0], src[0, 0]) and torch.equal(b[1], src[1, 0])  # interleaved by default


def test_object_layer_two_block_classes(ctx, torch):
    """an object of 3 blocks (K = 101, 100, 100, all coded with block 0's K'), two transmissions, against nanorq_encode"""
    L = api()
    T, Kt, Z = 64, 301, 3
    data = np.random.default_rng(5).integers(0, 256, Kt * T, dtype=np.uint8)
    rq = L.nanorq_encoder_new_ex(data.nbytes, T, 0, Z, 8)
    assert rq and L.nanorq_blocks(rq) == Z
    ks = [L.nanorq_block_symbols(rq, b) for b in range(Z)]
    assert ks == [101, 100, 100]
    Kp = nanorq_amd.params(ks[0])["Kp"]
    io = mem_io(data)
    rng = np.random.default_rng(6)
    d_data = _dev(torch, data)
    buf = (C.c_uint8 * T)()
    classes = [(0, 1, ks[0], 0), (1, 2, ks[1], ks[0] * T)]  # (sbn0, nblk, K, byte offset)
    txs = [nanorq_amd.Sender(ctx, K, T, nb, d_data[off:], sbn0=s0, Kp=Kp) for s0, nb, K, off in classes]
    try:
        for tx in txs:
            tx.encode()
        for sbn in range(Z):
            assert L.nanorq_generate_symbols(rq, sbn, io)
        for (s0, nb, K, off), tx in zip(classes, txs):
            esis = np.concatenate([rng.choice(K, 20, replace=False), np.arange(K, K + 30), [(1 << 24) - 1, (1 << 24) - 7]])
            tags = np.array([(s << 24) | int(e) for s in range(s0, s0 + nb) for e in esis], np.uint32)
            rng.shuffle(tags)
            for inline in (False, True):
                out = tx.emit(_dev(torch, tags.view(np.int32)), inline=inline)
                ctx.sync()
                out = out.cpu().numpy()
                o = 4 if inline else 0
                for k, t in enumerate(tags):
                    sbn, esi = int(t) >> 24, int(t) & 0xFFFFFF
                    assert L.nanorq_encode(rq, buf, esi, sbn, io) == T
                    assert bytes(out[k, o:o + T]) == bytes(buf), (sbn, esi)
                    if inline:
                        assert bytes(out[k, :4]) == int(t).to_bytes(4, "big")
    finally:
        for tx in txs:
            tx.close()
        L.nanorq_free(rq)
        io.contents.destroy(io)


def _keep_per_block(torch, g, nblk, per, keep):
    """indices (interleaved emission: packet k of block k % nblk) of `keep` packets of every block, chosen at random, shuffled"""
    n = nblk * per
    blk = torch.arange(n) % nblk
    order = torch.argsort(blk.double() + torch.rand(n, generator=g, dtype=torch.float64) * 0.5)
    rank = torch.arange(n) - (blk[order] * per)
    kept = order[rank < keep]
    return kept[torch.randperm(len(kept), generator=g)]


@pytest.mark.parametrize("K,T,nblk", [(100, 64, 4), (1000, 48, 8), (8192, 1280, 256)])
def test_device_only_round_trip(ctx, torch, orc, K, T, nblk):
    """Sender.emit_range (inline, interleaved) -> about 10 % of every block's packets lost, the rest shuffled, in torch ->
    Receiver.add(inline=True) -> decode: the source comes back"""
    g = torch.Generator().manual_seed(K)
    src = torch.randint(0, 256, (nblk, K, T), dtype=torch.uint8, generator=g).cuda()
    R = (K + 8) // 9 + 1  # ~10 % of the K + R packets of a block may be lost; two more than K arrive
    with nanorq_amd.Sender(ctx, K, T, nblk, src) as tx:
        torch.cuda.synchronize()
        tx.encode()
        pk = tx.emit_range(0, K + R, interleave=True, inline=True)
        ctx.sync()
        kept = _keep_per_block(torch, g, nblk, K + R, K + 2).cuda()
        recv = pk[kept]
        torch.cuda.synchronize()
        with nanorq_amd.Receiver(ctx, K, T, nblk, R + 8) as rx:
            rx.add(recv, inline=True)
            st, _ = rx.decode()
            ctx.sync()
            assert st.all(), np.flatnonzero(st == 0)
            assert torch.equal(rx.source, src)
        if K == 8192:  # two sampled blocks' repair packets against the oracle
            pk_h = pk.cpu().numpy()
            for b in (3, 200):
                esis = np.arange(K, K + R, dtype=np.uint32)
                rep, _, _ = orc.encode_block(src[b].cpu().numpy().reshape(-1), K, T, esis)
                rows = (esis.astype(np.int64)) * nblk + b
                assert np.array_equal(pk_h[rows, 4:4 + T], rep), b
                assert all(bytes(pk_h[r, :4]) == ((b << 24) | int(e)).to_bytes(4, "big") for r, e in zip(rows, esis))


def test_fountain_top_up(ctx, torch):
    """a first emission too short for some blocks; then block b gets n_b more fresh repair packets from ESI e_b, a tag list built
    in torch from the receiver's counts, and every block decodes"""
    K, T, nblk, R1 = 1000, 48, 8, 40
    g = torch.Generator().manual_seed(11)
    src = torch.randint(0, 256, (nblk, K, T), dtype=torch.uint8, generator=g).cuda()
    with nanorq_amd.Sender(ctx, K, T, nblk, src) as tx, nanorq_amd.Receiver(ctx, K, T, nblk, 400) as rx:
        torch.cuda.synchronize()
        tx.encode()
        pk = tx.emit_range(0, K + R1, interleave=True, inline=True)
        ctx.sync()
        lose = torch.rand(nblk * (K + R1), generator=g) < torch.linspace(0.01, 0.08, nblk).repeat(K + R1)  # per-block loss rates
        first_pk = pk[torch.nonzero(~lose).flatten().cuda()]
        torch.cuda.synchronize()
        rx.add(first_pk, inline=True)
        st, _ = rx.decode()
        assert 0 < st.sum() < nblk, st
        gaps, nrep = (torch.from_numpy(x.astype(np.int64)) for x in rx.counts())
        need = torch.where(torch.from_numpy(st.astype(bool)), torch.zeros_like(gaps), (gaps - nrep).clamp(min=0) + 3)
        e0 = torch.full((nblk,), K + R1, dtype=torch.int64)  # the next fresh ESI of every block
        b = torch.repeat_interleave(torch.arange(nblk), need)
        first = torch.cumsum(need, 0) - need
        esi = e0[b] + torch.arange(int(need.sum())) - first[b]
        tags = ((b << 24) | esi).to(torch.int32).cuda()
        res = torch.full((len(tags),), 77, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        more = tx.emit(tags, inline=True, results=res)
        rx.add(more, inline=True)
        st2, _ = rx.decode()
        ctx.sync()
        assert (res == 0).all()
        assert st2.all(), st2
        assert torch.equal(rx.source, src)


def test_refusals(ctx, torch):
    K, T, nblk = 10, 16, 2
    src = torch.zeros((nblk, K, T), dtype=torch.uint8, device="cuda")
    tags = torch.zeros((4,), dtype=torch.int32, device="cuda")
    out = torch.zeros((4, 64), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(nanorq_amd.NrqError):
        nanorq_amd.Sender(ctx, K, T, 2, src, sbn0=255)  # sbn0 + nblk > 256
    with pytest.raises(nanorq_amd.NrqError):
        nanorq_amd.Sender(ctx, K, T, nblk, src, src_stride=K * T - 1)
    with nanorq_amd.Sender(ctx, K, T, nblk, src) as tx:
        with pytest.raises(nanorq_amd.NrqError, match="not encoded"):
            tx.emit(tags, out=out)
        with pytest.raises(nanorq_amd.NrqError, match="not encoded"):
            tx.emit_range(0, 2, out=out)
        tx.encode()
        L = ctx._L
        p = C.c_void_p(out.data_ptr())
        assert L.nrq_tx_emit(tx._h, C.c_void_p(tags.data_ptr()), 4, p, T - 1, 0, None) == -1  # short stride
        assert L.nrq_tx_emit(tx._h, C.c_void_p(tags.data_ptr()), 4, p, T + 3, 1, None) == -1  # short for an inline header
        assert L.nrq_tx_emit(tx._h, C.c_void_p(tags.data_ptr()), 4, p, 64, 2, None) == -1     # unknown flags
        assert L.nrq_tx_emit_range(tx._h, 0, 2, 0, p, 64, 4, None) == -1                    # unknown flags
        assert L.nrq_tx_emit_range(tx._h, 0, 2, 2, p, 64, 0, None) == -1                    # unknown order
        assert L.nrq_tx_emit_range(tx._h, (1 << 24) - 1, 2, 0, p, 64, 0, None) == -1        # ESIs past 2^24
        tx.emit(tags, out=out)  # still usable after the refusals
        ctx.sync()
