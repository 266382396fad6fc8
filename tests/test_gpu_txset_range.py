"""GPU tier of the range mode of a sender set (nrq_txset_count_all / _emit_all / _emit_all_syms, SenderSet.count_all / emit_all /
emit_all_syms): the lists the device's map pass writes against the numpy statement of the map (txset_range_support.range_ref) and
against the emulated pass; the packet buffer against what SenderSet.emit / emit_syms writes for those lists on the same set, byte
for byte with FILL slack and guard rows; a set of one member against that member's own range call; the loop SenderSet.emit_all ->
ReceiverSet.add -> decode -> write with no host-built list; relays; every refusal; failing runtime calls.

Payload instances and the cases that launch them (T, header bytes), each asserted by tx_support.emit_mode (one symbol) or
syms_set_support.emit_path (several) on the addresses and strides handed over:
  nrq_emit_set_kernel<TX_V16 / TX_V16_SHIFT / TXS_V16_KEY / TX_DWORD / TX_BYTE, false> and nrq_emit_set_syms_kernel<the same>:
  (16, 0) (16, 4) (16, 8) (36, 4) (13, 8)   test_range_is_the_list_emit"""
import ctypes as C

import numpy as np
import pytest

import nanorq_amd
from nanorq_amd import NrqError
import syms_set_support as SS
from rxset_support import MIX4, MIX360
from test_gpu_txset import OBJ_T, OBJECTS, _Senders, _dev, _i32, _object_senders, _tx
from tx_support import FILL, emit_mode, tag
from txset_range_support import SEG64, emu_range, range_ref

pytestmark = pytest.mark.gpu

_V16 = {0: "TX_V16", 4: "TX_V16_SHIFT", 8: "TXS_V16_KEY"}


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available()
    return t


@pytest.fixture(scope="module")
def ctx(torch):
    import gpu_support as G
    return G.ctx()


def _stride(T, G, hdr):
    """the smallest stride that keeps the packets as aligned as T allows, plus one unit of that alignment as slack"""
    al = 16 if T % 16 == 0 else 4 if T % 4 == 0 else 1
    return (G * T + hdr + al - 1) // al * al + al


def _guarded(torch, n, stride):
    buf = torch.full((n + 2, stride), FILL, dtype=torch.uint8, device="cuda")
    return buf, buf[1:n + 1]


def _range(torch, ctx, st, nrep, G, order, hdr, stride, source=True, rep0=0, syms=None, outs=True, mode=None, rows=()):
    """one SenderSet.emit_all (emit_all_syms with syms, by default when G > 1) into a FILLed buffer with a guard row on either side
    -> (whole buffer with guards, keys, tags, counts) as numpy; the lists None without outs, the counts None in the one-symbol call"""
    syms = G > 1 if syms is None else syms
    n = st.count_all(nrep, G, source)
    buf, out = _guarded(torch, n, stride)
    if mode is not None:
        rule = SS.emit_path if syms else emit_mode
        assert rule(out.data_ptr(), stride, st.T, hdr, rows) == mode
    ko = to = no = None
    if outs:
        ko = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        to = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        no = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda") if syms else None
    torch.cuda.synchronize()
    kw = dict(interleave=bool(order), inline=hdr >= 4, key_inline=hdr == 8, out=out, rep0=rep0, source=source, keys_out=ko, tags_out=to)
    got = st.emit_all_syms(nrep, G, nsym_out=no, **kw) if syms else st.emit_all(nrep, **kw)
    ctx.sync()
    assert got is out

    def host(t, dt):
        return None if t is None else t.cpu().numpy().view(dt)
    return buf.cpu().numpy(), host(ko, np.uint32), host(to, np.uint32), host(no, np.uint8)


def _list(torch, ctx, st, keys, tags, cnts, G, hdr, stride, syms):
    """the same buffer through the list emit on the same set -> whole buffer with guards"""
    n = len(tags)
    buf, out = _guarded(torch, n, stride)
    if n:
        k_d, t_d = _i32(torch, keys), _i32(torch, tags)
        res = torch.full((n,), 77, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        if syms:
            st.emit_syms(k_d, t_d, G, nsym=_dev(torch, cnts), out=out, inline=hdr >= 4, key_inline=hdr == 8, results=res)
        else:
            st.emit(k_d, t_d, out=out, inline=hdr >= 4, key_inline=hdr == 8, results=res)
        ctx.sync()
        assert (res.cpu().numpy() == 0).all()
    return buf.cpu().numpy()


def _check(torch, ctx, m, mix, nrep, G, order, hdr, source=True, rep0=0, syms=None, mode=None, scratch=True):
    """one range call on the set of `mix`: its lists are the numpy statement's and the emulated pass's, its buffer the list emit's,
    and the same buffer comes out with every out array NULL (the lists in the set's scratch)"""
    st = m.set
    syms = G > 1 if syms is None else syms
    stride = _stride(st.T, G, hdr)
    keys, tags, cnts, lens = range_ref(mix, order, int(source), rep0, nrep, G)
    total, per = st.count_all(nrep, G, source, per_block=True)
    assert total == len(tags) and np.array_equal(per, lens)
    buf, gk, gt, gn = _range(torch, ctx, st, nrep, G, order, hdr, stride, source, rep0, syms, mode=mode, rows=m.rows())
    assert np.array_equal(gk, keys), np.flatnonzero(gk != keys)[:10]
    assert np.array_equal(gt, tags), np.flatnonzero(gt != tags)[:10]
    if syms:
        assert np.array_equal(gn, cnts), np.flatnonzero(gn != cnts)[:10]
    ek, et, ec, _, _ = emu_range(mix, order, int(source), rep0, nrep, G, total)
    assert np.array_equal(gk, ek) and np.array_equal(gt, et) and (not syms or np.array_equal(gn, ec))
    want = _list(torch, ctx, st, keys, tags, cnts, G, hdr, stride, syms)
    assert np.array_equal(buf, want), np.flatnonzero((buf != want).any(axis=1))[:10]
    if total:
        assert (buf[1:-1, :hdr + int(cnts[0]) * st.T] != FILL).any()
    if scratch:
        buf2, k2, _, _ = _range(torch, ctx, st, nrep, G, order, hdr, stride, source, rep0, syms, outs=False)
        assert k2 is None and np.array_equal(buf2, want)
    return total


@pytest.fixture(scope="module")
def mix4(ctx, torch):
    made = {}

    def get(T):
        if T not in made:
            made[T] = _Senders(ctx, torch, MIX4, T, seed=T)
        return made[T]
    yield get
    for m in made.values():
        m.close()


@pytest.mark.parametrize("T,hdr", [(16, 0), (16, 4), (16, 8), (36, 4), (13, 8)])
def test_range_is_the_list_emit(ctx, torch, mix4, T, hdr):
    """MIX4 (K = 26 x2, K = 10 x3, K = 100 x9 in block order; 1052 packets with all source and 5 repair symbols): one case per
    payload instance, both orders, G = 1 (one-symbol kernels) and 4 (several-symbol kernels), with and without the source symbols,
    rep0 = 0 and 7"""
    m = mix4(T)
    mode = _V16[hdr] if T % 16 == 0 else "TX_DWORD" if T % 4 == 0 else "TX_BYTE"
    seen = set()
    for order in (0, 1):
        for G in (1, 4):
            for source in (True, False):
                for rep0 in (0, 7):
                    seen.add(_check(torch, ctx, m, MIX4, 5, G, order, hdr, source, rep0, mode=mode, scratch=rep0 == 7))
    assert 1052 in seen and 14 * 5 in seen


def test_one_symbol_form_of_the_several_symbol_call(ctx, torch, mix4):
    """emit_all_syms with G = 1 writes emit_all's buffer and lists, with every count 1"""
    m = mix4(16)
    for order in (0, 1):
        _check(torch, ctx, m, MIX4, 5, 1, order, 8, syms=True, mode="TXS_V16_KEY")


@pytest.mark.parametrize("order", [0, 1])
def test_360_blocks(ctx, torch, order):
    """360 blocks of K = 10, 4320 packets: past 4096 packets and past 256 blocks, every length tied"""
    m = _Senders(ctx, torch, MIX360, 16, seed=360)
    try:
        assert _check(torch, ctx, m, MIX360, 2, 1, order, 8) == 4320
    finally:
        m.close()


def test_64_segments_interleaved(ctx, torch):
    """a full table: 64 segments of one block each, K cycling over 10, 11, 26, 100"""
    m = _Senders(ctx, torch, SEG64, 16, seed=64)
    try:
        assert len(m.set.blocks()[0]) == 64
        _check(torch, ctx, m, SEG64, 5, 1, 1, 4)
        _check(torch, ctx, m, SEG64, 5, 4, 1, 8, rep0=7)
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------ one member ----
def _filled(torch, n, stride):
    return torch.full((n, stride), FILL, dtype=torch.uint8, device="cuda")


@pytest.mark.parametrize("interleave", [False, True])
def test_one_object_is_its_own_emit_all(ctx, torch, interleave):
    """a set holding one ObjectSender of two block classes and a staged last block: emit_all / emit_all_syms with source and
    rep0 = 0 give the packets and tags of ObjectSender.emit_all / emit_all_syms"""
    (key, _, _, _), nrep, G = OBJECTS[0], 6, 4
    txs, _ = _object_senders(ctx, torch, OBJECTS[:1])
    st = nanorq_amd.SenderSet(ctx, OBJ_T)
    try:
        otx = txs[0]
        st.attach(key, otx)
        n, stride = otx.count_all(nrep), otx.stride(True) + 16
        assert st.count_all(nrep) == n
        mine, own = _filled(torch, n, stride), _filled(torch, n, stride)
        t_mine, t_own = (torch.full((n,), -1, dtype=torch.int32, device="cuda") for _ in range(2))
        torch.cuda.synchronize()
        st.emit_all(nrep, interleave=interleave, inline=True, out=mine, tags_out=t_mine)
        otx.emit_all(nrep, interleave=interleave, inline=True, out=own, tags_out=t_own)
        ctx.sync()
        assert np.array_equal(t_mine.cpu().numpy(), t_own.cpu().numpy()) and np.array_equal(mine.cpu().numpy(), own.cpu().numpy())
        n, stride = otx.count_all_syms(nrep, G), otx.stride_syms(G, True) + 16
        assert st.count_all(nrep, G) == n
        mine, own = _filled(torch, n, stride), _filled(torch, n, stride)
        t_mine = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        c_mine = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        st.emit_all_syms(nrep, G, interleave=interleave, inline=True, out=mine, tags_out=t_mine, nsym_out=c_mine)
        _, t_own, c_own = otx.emit_all_syms(nrep, G, interleave=interleave, inline=True, out=own)
        ctx.sync()
        assert np.array_equal(t_mine.cpu().numpy(), t_own.cpu().numpy()) and np.array_equal(c_mine.cpu().numpy(), c_own.cpu().numpy())
        assert np.array_equal(mine.cpu().numpy(), own.cpu().numpy())
        assert len(set(c_own.cpu().tolist())) > 2  # full packets, a short last source packet, a short last repair packet
    finally:
        st.close()
        for t in txs:
            t.close()


@pytest.mark.parametrize("interleave", [False, True])
def test_one_sender_is_its_own_emit_range(ctx, torch, interleave):
    K, T, nblk, nrep, G = 26, 16, 3, 5, 4
    m = _Senders(ctx, torch, [(77, K, nblk, 4)], T, seed=9)
    try:
        tx, st = m.tx[0], m.set
        n, stride = (K + nrep) * nblk, tx.stride(True) + 16
        mine, own = _filled(torch, n, stride), _filled(torch, n, stride)
        t_mine, t_own = (torch.full((n,), -1, dtype=torch.int32, device="cuda") for _ in range(2))
        torch.cuda.synchronize()
        st.emit_all(nrep, interleave=interleave, inline=True, out=mine, tags_out=t_mine)
        tx.emit_range(0, K + nrep, interleave=interleave, inline=True, out=own, tags_out=t_own)
        ctx.sync()
        assert np.array_equal(t_mine.cpu().numpy(), t_own.cpu().numpy()) and np.array_equal(mine.cpu().numpy(), own.cpu().numpy())
        n, stride = nanorq_amd.pkt_count(K, 0, K + nrep, G) * nblk, tx.stride_syms(G, True) + 16
        assert st.count_all(nrep, G) == n
        mine, own = _filled(torch, n, stride), _filled(torch, n, stride)
        t_mine = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        c_mine = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        st.emit_all_syms(nrep, G, interleave=interleave, inline=True, out=mine, tags_out=t_mine, nsym_out=c_mine)
        _, t_own, c_own = tx.emit_range_syms(0, K + nrep, G, interleave=interleave, inline=True, out=own)
        ctx.sync()
        assert np.array_equal(t_mine.cpu().numpy(), t_own.cpu().numpy()) and np.array_equal(c_mine.cpu().numpy(), c_own.cpu().numpy())
        assert np.array_equal(mine.cpu().numpy(), own.cpu().numpy())
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------ the loop ----
def test_the_loop_with_no_list(ctx, torch):
    """two objects of different K under two keys: SenderSet.emit_all(key_inline) -> packets dropped by a fixed seed ->
    ReceiverSet.add(key_inline) leaves every block two symbols short; a second call with source=False, rep0=nrep tops the
    receptions up with tags disjoint from the first call's; decode() and write() give both objects back"""
    rng = np.random.default_rng(2024)
    two, nrep, more = OBJECTS[:2], 2, 4
    txs, datas = _object_senders(ctx, torch, two, seed=3)
    rxs = [nanorq_amd.ObjectReceiver(ctx, *tx.oti, rep_cap=16) for tx in txs]
    sset, rset = nanorq_amd.SenderSet(ctx, OBJ_T), nanorq_amd.ReceiverSet(ctx, OBJ_T)
    try:
        for (key, _, _, _), tx, rx in zip(two, txs, rxs):
            sset.attach(key, tx)
            rset.attach(key, rx)
        n = sset.count_all(nrep)
        k1, t1 = (torch.full((n,), -1, dtype=torch.int32, device="cuda") for _ in range(2))
        torch.cuda.synchronize()
        first = sset.emit_all(nrep, inline=True, key_inline=True, keys_out=k1, tags_out=t1)
        ctx.sync()
        k1, t1 = k1.cpu().numpy().view(np.uint32), t1.cpu().numpy().view(np.uint32)
        blk = k1.astype(np.uint64) << np.uint64(8) | (t1 >> 24).astype(np.uint64)
        drop = np.concatenate([rng.choice(np.flatnonzero(blk == b), nrep + 2, replace=False) for b in np.unique(blk)])
        keep = np.setdiff1d(np.arange(n), drop)
        kept = first[torch.from_numpy(keep).cuda()].contiguous()
        torch.cuda.synchronize()
        rset.add(kept, inline=True, key_inline=True)
        assert all(rx.want().numel() > 0 for rx in rxs)  # every reception is short
        m = sset.count_all(more, source=False)
        k2, t2 = (torch.full((m,), -1, dtype=torch.int32, device="cuda") for _ in range(2))
        torch.cuda.synchronize()
        second = sset.emit_all(more, inline=True, key_inline=True, source=False, rep0=nrep, keys_out=k2, tags_out=t2)
        rset.add(second, inline=True, key_inline=True)
        ctx.sync()
        k2, t2 = k2.cpu().numpy().view(np.uint32), t2.cpu().numpy().view(np.uint32)
        assert m == more * len(np.unique(blk)) and not set(zip(k1.tolist(), t1.tolist())) & set(zip(k2.tolist(), t2.tolist()))
        st, _ = rset.decode()
        assert st.all()
        for rx, data in zip(rxs, datas):
            out, left = rx.write()
            ctx.sync()
            assert left == 0 and np.array_equal(out.cpu().numpy(), data)
    finally:
        sset.close()
        rset.close()
        for h in rxs + txs:
            h.close()


# ------------------------------------------------------------------------------------------------ relays ----
def test_relays(ctx, torch):
    """relays of two receptions beside nothing else: refused while a block is not ready, naming the first member's key and SBN, the
    buffer still FILL; after ReceiverSet.decode() the same call succeeds and is the list emit; held=True is refused"""
    import oracle
    rng = np.random.default_rng(17)
    K, T, nblk, nrep = 20, 16, 2, 3
    members = [(3, 0), (4, 6)]  # (key, sbn0)
    mix = [(key, K, nblk, sbn0) for key, sbn0 in members]
    rset, sset = nanorq_amd.ReceiverSet(ctx, T), nanorq_amd.SenderSet(ctx, T)
    hs, ks, ts, pl = [], [], [], []
    try:
        for key, sbn0 in members:
            src = rng.integers(0, 256, (nblk, K, T), dtype=np.uint8)
            rx = nanorq_amd.Receiver(ctx, K, T, nblk, 8, sbn0=sbn0)
            rset.attach(key, rx)
            relay = rx.relay()
            sset.attach(key, relay)
            hs += [relay, rx]
            for b in range(nblk):
                rep = oracle.encode_block(src[b], K, T, np.arange(K, K + 5, dtype=np.uint32))[0]
                for e in list(range(3, K)) + list(range(K, K + 5)):
                    ks.append(key)
                    ts.append(tag(sbn0 + b, e))
                    pl.append(src[b, e] if e < K else rep[e - K])
        n = sset.count_all(nrep)
        stride = _stride(T, 1, 8)
        buf, out = _guarded(torch, n, stride)
        torch.cuda.synchronize()
        with pytest.raises(NrqError, match="relay under key 3 is not ready: SBN 0"):
            sset.emit_all(nrep, inline=True, key_inline=True, out=out)
        ctx.sync()
        assert bool((buf == FILL).all())
        p_d, k_d, t_d = _dev(torch, np.array(pl, np.uint8)), _i32(torch, np.array(ks, np.uint32)), _i32(torch, np.array(ts, np.uint32))
        torch.cuda.synchronize()
        rset.add(p_d, keys=k_d, tags=t_d)
        st, _ = rset.decode()
        assert st.all()
        for order in (0, 1):
            keys, tags, cnts, _ = range_ref(mix, order, 1, 0, nrep, 1)
            got, gk, gt, _ = _range(torch, ctx, sset, nrep, 1, order, 8, stride)
            assert np.array_equal(gk, keys) and np.array_equal(gt, tags)
            assert np.array_equal(got, _list(torch, ctx, sset, keys, tags, cnts, 1, 8, stride, False))
        with pytest.raises(NrqError, match="NRQ_TX_HELD"):
            sset.emit_all(nrep, inline=True, key_inline=True, out=out, held=True)
        with pytest.raises(NrqError, match="NRQ_TX_HELD"):
            sset.emit_all_syms(nrep, 2, inline=True, key_inline=True, held=True)
        hs[3].reset()  # the second member's reception starts over: its blocks are not ready any more
        with pytest.raises(NrqError, match="relay under key 4 is not ready: SBN 6"):
            sset.emit_all(nrep, inline=True, key_inline=True, out=out)
    finally:
        sset.close()
        rset.close()
        for h in hs:
            h.close()


# ------------------------------------------------------------------------------------------------ refusals and edges ----
def test_refusals_leave_the_buffer_untouched(ctx, torch):
    T, K = 16, 10
    L = ctx._L
    a, raw = _tx(ctx, torch, encode=True), _tx(ctx, torch, sbn0=5)
    rx = nanorq_amd.Receiver(ctx, K, T, 1, 2)
    relay = rx.relay()
    st, empty, bad = (nanorq_amd.SenderSet(ctx, T) for _ in range(3))
    try:
        st.attach(0, a)
        G = 4
        pk = torch.full((64, G * T + 8), FILL, dtype=torch.uint8, device="cuda")
        lists = torch.full((3, 64), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        P = C.c_void_p(pk.data_ptr())
        KO, TO, NO = (C.c_void_p(lists[i].data_ptr()) for i in range(3))
        npkt = C.c_uint32(99)
        TAG, HELD, KEY = nanorq_amd.TX_TAG_INLINE, nanorq_amd.TX_HELD, nanorq_amd.TX_KEY_INLINE

        def err():
            return L.nrq_ctx_error(ctx._h)

        def one(flags=0, source=1, rep0=0, nrep=2, order=1, stride=T + 8, s=st, pkts=P):
            return L.nrq_txset_emit_all(s._h, source, rep0, nrep, order, pkts, stride, flags, KO, TO, C.byref(npkt))

        def many(flags=0, source=1, rep0=0, nrep=2, g=G, order=1, stride=G * T + 8, s=st, pkts=P):
            return L.nrq_txset_emit_all_syms(s._h, source, rep0, nrep, g, order, pkts, stride, flags, KO, TO, NO, C.byref(npkt))

        for call in (one, many):
            assert call(flags=8) == -1 and b"unknown flags" in err()
            assert call(flags=KEY) == -1 and b"NRQ_TX_TAG_INLINE" in err()
            assert call(flags=TAG | HELD) == -1 and b"NRQ_TX_HELD" in err()
            assert call(pkts=None) == -1 and b"d_pkts is NULL" in err()
            assert call(order=2) == -1 and call(order=-1) == -1 and b"order" in err()
            assert call(source=2) == -1 and b"source" in err()
            assert call(nrep=(1 << 24) - K + 1) == -1 and b"2^24" in err()           # K + nrep - 1 = 0xFFFFFF + 1
            assert call(rep0=(1 << 24) - K - 1, nrep=2) == -1 and b"2^24" in err()  # the bound counts rep0
            assert call(flags=KEY, s=empty) == -1                                    # argument errors come first, also on an empty set
        assert one(stride=T - 1) == -1 and one(flags=TAG, stride=T + 3) == -1 and one(flags=TAG | KEY, stride=T + 7) == -1
        assert b"shorter than a packet" in err()
        assert many(stride=G * T - 1) == -1 and many(flags=TAG | KEY, stride=G * T + 7) == -1 and b"shorter than a packet" in err()
        assert many(g=0) == -1 and many(g=65, stride=65 * T) == -1 and b"outside 1..64" in err()
        # a member that is not encoded; a relay with a block that is not ready; a relay whose reception was destroyed
        bad.attach(1, raw)
        assert one(s=bad) == -1 and b"key 1 is not encoded" in err()
        bad.detach(1)
        bad.attach(2, relay)
        assert one(s=bad) == -1 and b"relay under key 2 is not ready: SBN 0" in err()
        rx.close()
        assert one(s=bad) == -1 and b"relay under key 2 was destroyed" in err()
        assert npkt.value == 99
        ctx.sync()
        assert bool((pk == FILL).all()) and bool((lists == 0x5A5A5A5A).all())       # nothing was enqueued, nothing written
        # an empty set, and neither source nor repair symbols: 0 packets, no launch
        assert one(s=empty) == 0 and npkt.value == 0
        npkt.value = 99
        assert many(source=0, nrep=0) == 0 and npkt.value == 0
        assert st.count_all(0, source=False) == 0 and empty.count_all(5) == 0
        ctx.sync()
        assert bool((pk == FILL).all()) and bool((lists == 0x5A5A5A5A).all())
        # every out array and h_npkt are nullable, each on its own
        assert L.nrq_txset_emit_all_syms(st._h, 1, 0, 2, G, 1, P, G * T + 8, TAG | KEY, None, TO, None, None) == 0
        assert L.nrq_txset_emit_all(st._h, 1, 0, 2, 0, P, T + 8, 0, KO, None, None) == 0
        ctx.sync()
        assert lists[1, :4].cpu().tolist() == [tag(0, 0), tag(0, 4), tag(0, 8), tag(0, 10)] and bool((lists[1, 4:] == 0x5A5A5A5A).all())
        assert lists[0, :12].cpu().tolist() == [0] * 12 and bool((lists[0, 12:] == 0x5A5A5A5A).all()) and bool((lists[2] == 0x5A5A5A5A).all())
        # count_all: the ESI bound at exactly 0xFFFFFF is accepted, one above is refused; G and source as the emits
        assert st.count_all(0xFFFFFF - K + 1) == 0xFFFFFF + 1 and st.count_all(0xFFFFFF - K + 1, source=False) == 0xFFFFFF - K + 1
        with pytest.raises(NrqError, match="2\\^24"):
            st.count_all(0xFFFFFF - K + 2)
        with pytest.raises(NrqError, match="outside 1..64"):
            st.count_all(2, G=65)
        assert L.nrq_txset_count_all(st._h, 2, 2, 1, None, None) == -1 and b"source" in err()
    finally:
        for h in (st, empty, bad, relay, rx, a, raw):
            h.close()


def test_total_cap_from_the_counts_alone(ctx, torch):
    """MIX360's table (360 blocks of K = 10; nothing encoded: the counts are host state).  The cap is 0x7FFFFFFF packets, and
    packets * G: nrep = 2**22 gives 360 * (10 + 2**22) = 1 509 953 040 packets, which is below it and is counted; nrep = 2**23
    (3 019 902 480 packets) is refused by count_all and by both emits before anything is allocated -- the emits are handed a
    buffer of one packet."""
    T = 16
    hs = [_tx(ctx, torch, nblk, sbn0, T=T) for _, _, nblk, sbn0 in MIX360]
    st = nanorq_amd.SenderSet(ctx, T)
    try:
        for (key, _, _, _), h in zip(MIX360, hs):
            st.attach(key, h)
        total, per = st.count_all(2, per_block=True)
        assert total == 4320 and per.tolist() == [12] * 360
        assert st.count_all(2 ** 22) == 360 * (10 + 2 ** 22) < 0x7FFFFFFF
        pk = torch.full((1, 64 * T), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for nrep, G in ((2 ** 23, 1), (2 ** 23, 2), (2 ** 23, 64)):  # too many packets; packets * G too large, at G = 2 and G = 64
            with pytest.raises(NrqError, match="more than one call takes"):
                st.count_all(nrep, G)
            L, P, npkt = ctx._L, C.c_void_p(pk.data_ptr()), C.c_uint32(99)
            assert L.nrq_txset_emit_all_syms(st._h, 1, 0, nrep, G, 1, P, 64 * T, 0, None, None, None, C.byref(npkt)) == -1
            assert b"more than one call takes" in L.nrq_ctx_error(ctx._h) and npkt.value == 99
            if G == 1:
                assert L.nrq_txset_emit_all(st._h, 1, 0, nrep, 1, P, T, 0, None, None, C.byref(npkt)) == -1
                assert b"more than one call takes" in L.nrq_ctx_error(ctx._h)
        ctx.sync()
        assert bool((pk == FILL).all())
    finally:
        for h in [st] + hs:
            h.close()


# ------------------------------------------------------------------------------------------------ failing runtime calls ----
def _books(c):
    b = (C.c_size_t * 3)()
    assert c._L.nrq_dev_pool_books(c._h, b) == 0
    return tuple(int(x) for x in b)


def test_failing_runtime_calls(torch):
    """fail_after on a context of its own: the n-th checked runtime call of an emit_all that has to grow the set's scratch fails.
    Every failure returns an error, the next call succeeds and is the list emit, and the pool's books end as in the run in which
    nothing failed."""
    import gpu_support as G
    G.ctx()  # (torch first, as every context of this process)
    T, mix, nrep = 16, [MIX4[0], MIX4[2]], 5
    keys, tags, cnts, _ = range_ref(mix, 1, 1, 0, nrep, 1)
    stride = _stride(T, 1, 8)
    texts, books = [], []
    for n_fail in range(1, 12):
        fctx = nanorq_amd.Context(0)  # (a pool of its own, empty: the scratch allocation reaches the runtime)
        m = _Senders(fctx, torch, mix, T, seed=n_fail)
        try:
            k_d, t_d = _i32(torch, keys[:4]), _i32(torch, tags[:4])
            small = _filled(torch, 4, stride)
            torch.cuda.synchronize()
            m.set.emit(k_d, t_d, out=small, inline=True, key_inline=True)  # (a first scratch: the range call has to replace it)
            fctx.sync()
            fctx._chk(fctx._L.nrq_dev_trim(fctx._h))                       # (nothing cached: the new one comes from the runtime)
            out = _filled(torch, len(tags), stride)
            torch.cuda.synchronize()
            err = None
            fctx.set_option("fail_after", n_fail)
            try:
                m.set.emit_all(nrep, inline=True, key_inline=True, out=out)  # (the emit alone: no wait of the test's behind it)
            except NrqError as e:
                err = str(e)
            fctx.set_option("fail_after", 0)
            fctx.sync()
            if err is not None:
                texts.append(err)
            again, _, _, _ = _range(torch, fctx, m.set, nrep, 1, 1, 8, stride, outs=False)  # (the same call: the same scratch)
            books.append(_books(fctx))
            got, gk, gt, _ = _range(torch, fctx, m.set, nrep, 1, 1, 8, stride)
            assert np.array_equal(gk, keys) and np.array_equal(gt, tags), err
            want = _list(torch, fctx, m.set, keys, tags, cnts, 1, 8, stride, False)
            assert np.array_equal(got, want) and np.array_equal(again, want), err
        finally:
            m.close()
            fctx.close()
        if err is None:
            break  # (the call makes fewer than n_fail checked runtime calls)
    assert err is None and len(texts) >= 4, texts
    assert any("hipMalloc" in t for t in texts) and any("hipStreamSynchronize" in t for t in texts) and any("hipGetLastError" in t for t in texts)
    assert all(b == books[-1] for b in books), books
