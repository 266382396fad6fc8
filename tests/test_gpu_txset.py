"""GPU tier of the sender sets (nrq_txset_*, nanorq_amd.SenderSet): the set's emit kernels against their CPU emulation
(nanorq_amd/csrc/txset_emu.cpp) byte for byte in every payload mode with and without held symbols, against each member's own
emit, relays whose ready state changes under the set, the want -> emit -> add -> decode loop through a SenderSet and a
ReceiverSet with no repacking in between, the API's refusals, lifetimes, and failing runtime calls.

nrq_emit_set_kernel<MODE, HELD> instances and the cases that launch them (T, header bytes):
  <TX_V16, false> (16, 0)   <TX_V16_SHIFT, false> (16, 4)   <TXS_V16_KEY, false> (16, 8)   <TX_DWORD, false> (36, *)   <TX_BYTE, false> (13, *)
      test_device_matches_emulation
  <TX_V16, false> (T, 0)    <TX_V16_SHIFT, false> (T, 4)    <TXS_V16_KEY, false> (T, 8)    T = 32, 1024, 1040, 2064: a lane takes its
      neighbour's dwords, a full wave, a second round of one lane fed by the carry, a carry out of a round that began with one
  <TX_DWORD, false> (T, *)  T = 252, 256 (a stride of 4 mod 16), 260: 63 lanes, one round, a second round of one lane
  <TX_BYTE, false> (T, *)   T = 63, 64 (an odd stride), 65
      test_device_matches_emulation_at_wave_edges
  <TX_V16, true> (16, 0)    <TX_V16_SHIFT, true> (16, 4)    <TXS_V16_KEY, true> (16, 8)    <TX_DWORD, true> (36, 4)   <TX_BYTE, true> (13, 8)
  <TX_V16, true> (1040, 0)  <TX_V16_SHIFT, true> (1040, 4)  <TXS_V16_KEY, true> (1040, 8)  <TX_DWORD, true> (260, 4)  <TX_BYTE, true> (65, 8)
      test_held_device_matches_emulation
Every case asserts, by tx_support.emit_mode on the addresses and strides it hands over, that it runs the instance it is listed for."""
import ctypes as C

import numpy as np
import pytest

import nanorq_amd
from nanorq_amd import EXT_SUBBLOCKS, NrqError
from rx_support import ADDED, EmuRx, payloads_for
from rxset_support import MIX4, MIX360
from tx_support import emit_mode
from txset_support import FILL, FOREIGN, NOT_READY, UNKNOWN_KEY, Seg, be32, emu_txset_emit, global_blocks, keyed_tags, tag
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
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _i32(torch, a):
    return _dev(torch, np.ascontiguousarray(a, np.uint32).view(np.int32))


def _L(Kp):
    return nanorq_amd.params(Kp)["L"]


class _Senders:
    """the Senders of a mix on the device, encoded, attached to one set; segs: the same table for the emulation, with the
    intermediate symbols the device made"""

    def __init__(self, ctx, torch, mix, T, seed=1):
        rng = np.random.default_rng(seed)
        self.set = nanorq_amd.SenderSet(ctx, T)
        self.tx, self.segs, self.src = [], [], []
        for key, K, nblk, sbn0 in mix:
            Kp = nanorq_amd.params(K)["Kp"]
            src = rng.integers(0, 256, (nblk, K, T), dtype=np.uint8)
            self.src.append(_dev(torch, src))
            torch.cuda.synchronize()
            tx = nanorq_amd.Sender(ctx, K, T, nblk, self.src[-1], sbn0=sbn0)
            tx.encode()
            ctx.sync()
            inter = ctx.download(tx.inter_ptr, nblk * _L(Kp) * T).reshape(nblk, _L(Kp), T)
            self.tx.append(tx)
            self.segs.append(Seg(key, K, Kp, T, sbn0, src, inter))
            self.set.attach(key, tx)

    def rows(self):
        """(address, stride) of every row table an emit reads: the source rows and the intermediate symbols of each member"""
        return [(src.data_ptr(), s.K * s.T) for src, s in zip(self.src, self.segs)] + \
               [(tx.inter_ptr, _L(s.Kp) * s.T) for tx, s in zip(self.tx, self.segs)]

    def close(self):
        self.set.close()
        for t in self.tx:
            t.close()


def _emit(torch, ctx, st, keys, tags, hdr, stride, held=False, mode=None, rows=()):
    """one SenderSet.emit into a FILLed buffer with a guard row of FILL on either side -> (packets, results) as numpy; mode: the
    instance the call must take by the launch rule, from the buffer's address, the stride, the set's T and the row tables `rows`"""
    n = len(tags)
    buf = torch.full((n + 2, stride), FILL, dtype=torch.uint8, device="cuda")
    out = buf[1:n + 1]
    if mode is not None:
        assert emit_mode(out.data_ptr(), stride, st.T, hdr, rows) == mode
    res = torch.full((n,), 77, dtype=torch.int32, device="cuda")
    k_d = None if keys is None else _i32(torch, keys)
    t_d = _i32(torch, tags)
    torch.cuda.synchronize()
    got = st.emit(k_d, t_d, out=out, inline=hdr >= 4, key_inline=hdr == 8, results=res, held=held)
    ctx.sync()
    assert got is out
    assert bool((buf[0] == FILL).all()) and bool((buf[n + 1] == FILL).all()), "guard rows"
    return out.cpu().numpy(), res.cpu().numpy()


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


def _stride(T, hdr, slack):
    """the smallest stride that keeps the packets as aligned as T allows, plus slack rows of that alignment"""
    al = 16 if T % 16 == 0 else 4 if T % 4 == 0 else 1
    return (T + hdr + al - 1) // al * al + slack * al


@pytest.mark.parametrize("n", [1, 65, 4097])
@pytest.mark.parametrize("hdr", [0, 4, 8])
@pytest.mark.parametrize("T", [16, 36, 13])
def test_device_matches_emulation(ctx, torch, mix4, T, hdr, n):
    """the four-member mix: T = 16 gives the 16-byte forms (plain, under the FEC Payload ID, under key + FEC Payload ID), T = 36 the
    4-byte form, T = 13 the byte form; one packet, two waves, two bucketing tiles"""
    m = mix4(T)
    rng = np.random.default_rng(T * 100 + hdr * 10 + n)
    keys, tags = keyed_tags(rng, m.segs, n)
    stride = _stride(T, hdr, int(n == 65))
    pk, res = _emit(torch, ctx, m.set, keys, tags, hdr, stride)
    epk, eres, _ = emu_txset_emit(m.segs, keys, tags, hdr, stride)
    assert np.array_equal(res, eres), np.flatnonzero(res != eres)[:10]
    assert np.array_equal(pk, epk), np.flatnonzero((pk != epk).any(axis=1))[:10]
    if n > 1:
        assert (res == 0).any() and (res == FOREIGN).any()


def _edge_stride(T, hdr, mode):
    """a stride for T bytes behind hdr that leaves the packets on `mode`: 16-byte aligned with a 16-byte slack; 4 (mod 16); odd"""
    need = T + hdr
    if mode in ("TX_V16", "TX_V16_SHIFT", "TXS_V16_KEY"):
        return (need + 15) // 16 * 16 + 16
    if mode == "TX_DWORD":
        return need + (4 - need) % 16
    return need | 1


_V16 = {0: "TX_V16", 4: "TX_V16_SHIFT", 8: "TXS_V16_KEY"}
# (T, mode): the sizes at which each form first fills a wave's round (64 lanes of 16, 4 or 1 bytes) and first wraps into the next
EDGES = [(T, None) for T in (32, 1024, 1040, 2064)] + [(T, "TX_DWORD") for T in (252, 256, 260)] + [(T, "TX_BYTE") for T in (63, 64, 65)]


@pytest.mark.parametrize("hdr", [0, 4, 8])
@pytest.mark.parametrize("T,mode", EDGES)
def test_device_matches_emulation_at_wave_edges(ctx, torch, mix4, T, mode, hdr):
    """the four-member mix at the symbol sizes where a payload form fills or wraps a wave: the shifted 16-byte forms take a
    neighbour lane's dwords (T = 32), the tail comes from lane 63 (1024), a second round has one live lane fed by the carry (1040),
    a third a carry out of a round that began with one (2064); the dword and byte forms at 63 lanes, one round and one lane more.
    About 300 packets: source, repair (multi-row gathers) and foreign ones; buffer, stride slack and guard rows compared whole."""
    m = mix4(T)
    mode = mode or _V16[hdr]
    rng = np.random.default_rng(T * 100 + hdr)
    keys, tags = keyed_tags(rng, m.segs, 300)
    stride = _edge_stride(T, hdr, mode)
    pk, res = _emit(torch, ctx, m.set, keys, tags, hdr, stride, mode=mode, rows=m.rows())
    epk, eres, _ = emu_txset_emit(m.segs, keys, tags, hdr, stride)
    assert np.array_equal(res, eres), np.flatnonzero(res != eres)[:10]
    assert np.array_equal(pk, epk), np.flatnonzero((pk != epk).any(axis=1))[:10]
    assert (res == 0).any() and (res == FOREIGN).any()
    esi = tags & 0xFFFFFF
    assert (res[esi < 10] == 0).any() and (res[esi >= 100] == 0).any()  # (source and repair packets of some member)


def test_device_matches_emulation_no_keys(ctx, torch, mix4):
    """d_keys NULL: every packet has key 0"""
    m = mix4(16)
    rng = np.random.default_rng(8)
    _, tags = keyed_tags(rng, [s for s in m.segs if s.key == 0], 300)
    pk, res = _emit(torch, ctx, m.set, None, tags, 4, 32)
    epk, eres, _ = emu_txset_emit(m.segs, None, tags, 4, 32)
    assert np.array_equal(res, eres) and np.array_equal(pk, epk) and (res == 0).any()


def test_device_matches_emulation_360_blocks(ctx, torch):
    m = _Senders(ctx, torch, MIX360, 16, seed=360)
    try:
        rng = np.random.default_rng(360)
        keys, tags = keyed_tags(rng, m.segs, 4097)
        pk, res = _emit(torch, ctx, m.set, keys, tags, 8, 32)
        epk, eres, _ = emu_txset_emit(m.segs, keys, tags, 8, 32)
        assert np.array_equal(res, eres) and np.array_equal(pk, epk)
        g, nb = global_blocks(m.segs, keys, tags)
        assert nb == 360 and len(np.unique(g)) > 257
        bk, bs = m.set.blocks()
        assert list(bk) == [1] * 240 + [2] * 120 and list(bs) == list(range(240)) + list(range(120))
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------------------------ held ----
class _Relays:
    """receptions on the device and in the emulation fed the same lossy stream, their relays attached to one set beside one plain
    sender; block 0 of every reception is complete and made ready by the relay's encode"""

    def __init__(self, ctx, torch, T, seed):
        rng = np.random.default_rng(seed)
        self.set = nanorq_amd.SenderSet(ctx, T)
        self.hs, self.segs, self.sent, self.tables = [], [], [], []
        for key, K, nblk, sbn0, cap in ((7, 31, 3, 2, 6), (7, 30, 2, 5, 40), (2, 10, 2, 2, 3)):
            Kp = nanorq_amd.params(K)["Kp"]
            rx = nanorq_amd.Receiver(ctx, K, T, nblk, cap, sbn0=sbn0)
            emu = EmuRx(K, T, nblk, cap, sbn0=sbn0, Kp=Kp)
            sent = np.array([tag(sbn0 + b, e) for b in range(nblk) for e in range(K + K // 4 + 4)], np.uint32)
            keep = (rng.random(len(sent)) >= 0.25) | ((sent >> 24) == sbn0)  # (block 0 loses nothing)
            deliv = sent[keep]
            rng.shuffle(deliv)
            for part in np.array_split(deliv, 2):
                pl = payloads_for(part, T, key)
                p_d, t_d = _dev(torch, pl), _i32(torch, part)
                torch.cuda.synchronize()
                rx.add(p_d, tags=t_d)
                ctx.sync()
                emu.add(pl, tags=part)
            relay = rx.relay()
            relay.encode()
            ctx.sync()
            ready = relay.ready()
            assert ready[0] and not ready[1:].any()
            inter = ctx.download(relay.inter_ptr, nblk * _L(Kp) * T).reshape(nblk, _L(Kp), T)
            self.segs.append(Seg(key, K, Kp, T, sbn0, emu.src, inter, rx=emu, ready=ready))
            self.tables += [(rx.src_ptr, K * T), (relay.inter_ptr, _L(Kp) * T), (rx.rep_ptr, cap * T)]
            self.sent.append((key, sent, emu))
            self.set.attach(key, relay)
            self.hs += [relay, rx]
        self.plain = _Senders(ctx, torch, [(9, 26, 2, 2)], T, seed=seed + 1)
        tx = self.plain.tx[0]
        self.plain.set.detach(9)
        self.set.attach(9, tx)
        self.segs += self.plain.segs

    def rows(self):
        """(address, stride) of every row table a held emit reads: the receptions' source and repair rows, the relays' intermediate
        symbols, the plain sender's tables"""
        return self.tables + self.plain.rows()

    def tags(self, rng):
        ks, ts = [], []
        for key, sent, emu in self.sent:
            extra = np.array([tag(sbn, e) for sbn in range(max(0, emu.sbn0 - 1), emu.sbn0 + emu.nblk + 1)
                              for e in (emu.max_esi, emu.max_esi + 1, emu.bm_words * 32 + 31, (1 << 24) - 1, emu.K + 60)], np.uint32)
            ts.append(np.concatenate([sent, extra]))
            ks.append(np.full(len(ts[-1]), key, np.uint32))
        k2, t2 = keyed_tags(rng, self.plain.segs, 80)
        keys, tags = np.concatenate(ks + [k2]), np.concatenate(ts + [t2])
        perm = rng.permutation(len(tags))
        return keys[perm], tags[perm]

    def close(self):
        self.set.close()
        for h in self.hs:
            h.close()
        self.plain.close()


@pytest.mark.parametrize("T,hdr", [(16, 0), (16, 4), (16, 8), (36, 4), (13, 8), (1040, 0), (1040, 4), (1040, 8), (260, 4), (65, 8)])
def test_held_device_matches_emulation(ctx, torch, T, hdr):
    """NRQ_TX_HELD over relay members beside a plain sender, in every payload mode: blocks that are ready, held source and repair
    symbols of blocks that are not, symbols not held, ESIs behind the bitmap, foreign SBNs; each mode also at a size that takes
    the wave into a second round (T = 1040, 260, 65)"""
    m = _Relays(ctx, torch, T, seed=T + hdr)
    try:
        keys, tags = m.tags(np.random.default_rng(T))
        stride = _stride(T, hdr, 1)
        mode = _V16[hdr] if T % 16 == 0 else "TX_DWORD" if T % 4 == 0 else "TX_BYTE"
        pk, res = _emit(torch, ctx, m.set, keys, tags, hdr, stride, held=True, mode=mode, rows=m.rows())
        epk, eres, _ = emu_txset_emit(m.segs, keys, tags, hdr, stride, held=True)
        assert np.array_equal(res, eres), np.flatnonzero(res != eres)[:10]
        assert np.array_equal(pk, epk), np.flatnonzero((pk != epk).any(axis=1))[:10]
        g, nb = global_blocks(m.segs, keys, tags)
        bits = np.concatenate([s.ready for s in sorted(m.segs, key=lambda s: (s.key, s.sbn0))] + [[True]])
        cold = ~bits[g]
        esi = tags & 0xFFFFFF
        assert (res[cold & (esi < 10)] == 0).any() and (res[cold & (esi >= 31)] == 0).any() and (res[cold] == NOT_READY).any()
        # without the flag: nothing from a block that is not ready, the rest as before
        pk0, res0 = _emit(torch, ctx, m.set, keys, tags, hdr, stride)
        epk0, eres0, _ = emu_txset_emit(m.segs, keys, tags, hdr, stride)
        assert np.array_equal(res0, eres0) and np.array_equal(pk0, epk0)
        assert (res0[cold] == NOT_READY).all() and (pk0[cold] == FILL).all()
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------------------------ objects ----
OBJ_T = 64
OBJECTS = [  # (key, F, ObjectSender arguments, flags)
    (0x1001, 213 * OBJ_T - 5, dict(Z=5), 0),                                      # two block classes: 3 blocks of 43, 2 of 42
    (7, 300 * OBJ_T, dict(Z=2), 0),                                               # one class, K = 150
    (0xFFFFFFFF, 90 * OBJ_T - 17, dict(Z=3, N=2, Al=8, flags=EXT_SUBBLOCKS), EXT_SUBBLOCKS),  # N > 1: sub-blocks
]


def _object_senders(ctx, torch, objects, seed=0):
    txs, datas = [], []
    for key, F, kw, _ in objects:
        datas.append(payload(F, seed=F + seed))
        d = _dev(torch, datas[-1])
        torch.cuda.synchronize()
        txs.append(nanorq_amd.ObjectSender(ctx, d, OBJ_T, **kw))
        txs[-1].encode()
    return txs, datas


def _object_tags(rng, key, tx, per_block):
    """source and repair ESIs of every block of an object, and SBNs at and behind Z"""
    out = []
    for sbn, (K, _) in enumerate(tx.blocks):
        out += [tag(sbn, e) for e in rng.integers(0, K + 30, per_block)] + [tag(sbn, 0), tag(sbn, K - 1), tag(sbn, K), tag(sbn, (1 << 24) - 1)]
    Z = len(tx.blocks)
    out += [tag(Z, 0), tag(min(255, Z + 1), 5), tag(255, 1)]
    return np.full(len(out), key, np.uint32), np.array(out, np.uint32)


@pytest.mark.parametrize("inline,key_inline", [(False, False), (True, False), (True, True)])
def test_against_the_members_alone(ctx, torch, inline, key_inline):
    """three objects -- two block classes with a staged last block, one class, N = 2 sub-blocks -- in one set: every packet of a
    mixed list equals, behind the key, what the object's own emit writes for that tag, and so does its result"""
    rng = np.random.default_rng(11)
    txs, _ = _object_senders(ctx, torch, OBJECTS)
    st = nanorq_amd.SenderSet(ctx, OBJ_T)
    try:
        for (key, _, _, _), tx in zip(OBJECTS, txs):
            st.attach(key, tx)
        parts = [_object_tags(rng, key, tx, 40) for (key, _, _, _), tx in zip(OBJECTS, txs)]
        parts.append((np.full(20, UNKNOWN_KEY, np.uint32), parts[0][1][:20]))
        keys, tags = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        perm = rng.permutation(len(tags))
        keys, tags = keys[perm], tags[perm]
        hdr = 8 if key_inline else 4 if inline else 0
        stride = st.stride(inline, key_inline) + 16
        pk, res = _emit(torch, ctx, st, keys, tags, hdr, stride)
        koff = 4 if key_inline else 0
        owned = np.zeros(len(tags), bool)
        for (key, _, _, _), tx in zip(OBJECTS, txs):
            sel = np.flatnonzero(keys == key)
            owned[sel] = True
            mstride = OBJ_T + (16 if inline else 0)
            out = torch.full((len(sel), mstride), FILL, dtype=torch.uint8, device="cuda")
            mres = torch.full((len(sel),), 77, dtype=torch.int32, device="cuda")
            t_d = _i32(torch, tags[sel])
            torch.cuda.synchronize()
            tx.emit(t_d, out=out, inline=inline, results=mres)
            ctx.sync()
            mpk, mres = out.cpu().numpy(), mres.cpu().numpy()
            plen = OBJ_T + (4 if inline else 0)
            assert np.array_equal(res[sel], mres), key
            assert np.array_equal(pk[sel, koff:koff + plen], mpk[:, :plen]), key
            assert (pk[sel, koff + plen:] == FILL).all()
            beyond = (tags[sel] >> 24) >= len(tx.blocks)
            assert beyond.any() and (mres[beyond] == FOREIGN).all() and (mres[~beyond] == 0).all()
            assert (pk[sel[beyond]] == FILL).all()
            if key_inline:
                assert np.array_equal(pk[sel[~beyond], :4], be32(keys[sel[~beyond]]))
        assert (res[~owned] == FOREIGN).all() and (pk[~owned] == FILL).all() and (~owned).sum() == 20
    finally:
        st.close()
        for t in txs:
            t.close()


# ------------------------------------------------------------------------------------------------------------------ relays ----
def test_relays_and_their_ready_state(ctx, torch):
    """two receptions in a ReceiverSet, their relays in a SenderSet: held symbols and NOT_READY after a partial ingest; after
    ReceiverSet.decode(), with no call on the SenderSet, fresh repair symbols equal the oracle's; a reset enqueued directly behind
    an emit leaves that emit's packets whole and takes the member out of the next one"""
    import oracle
    rng = np.random.default_rng(99)
    K, T, nblk = 20, 16, 2
    members = [(3, 0), (4, 6)]  # (key, sbn0)
    fresh = np.arange(K + 8, K + 12, dtype=np.uint32)
    rset, sset = nanorq_amd.ReceiverSet(ctx, T), nanorq_amd.SenderSet(ctx, T)
    hs, srcs, reps = [], [], []
    try:
        for key, sbn0 in members:
            src = rng.integers(0, 256, (nblk, K, T), dtype=np.uint8)
            srcs.append(src)
            reps.append([oracle.encode_block(src[b], K, T, np.arange(K, K + 12, dtype=np.uint32))[0] for b in range(nblk)])
            rx = nanorq_amd.Receiver(ctx, K, T, nblk, 8, sbn0=sbn0)
            rset.attach(key, rx)
            relay = rx.relay()
            sset.attach(key, relay)
            hs += [relay, rx]
        rxs = hs[1::2]

        def feed(esis):
            """every block's symbols of these ESIs, all members, in one ReceiverSet.add"""
            ks, ts, pl = [], [], []
            for (key, sbn0), src, rep in zip(members, srcs, reps):
                for b in range(nblk):
                    for e in esis:
                        ks.append(key)
                        ts.append(tag(sbn0 + b, e))
                        pl.append(src[b, e] if e < K else rep[b][e - K])
            p_d, k_d, t_d = _dev(torch, np.array(pl, np.uint8)), _i32(torch, np.array(ks, np.uint32)), _i32(torch, np.array(ts, np.uint32))
            torch.cuda.synchronize()
            rset.add(p_d, keys=k_d, tags=t_d)
            ctx.sync()

        def ask(esis, held=False, sync=True):
            ks = np.array([key for key, _ in members for b in range(nblk) for e in esis], np.uint32)
            ts = np.array([tag(sbn0 + b, e) for _, sbn0 in members for b in range(nblk) for e in esis], np.uint32)
            out = torch.full((len(ts), T + 16), FILL, dtype=torch.uint8, device="cuda")
            res = torch.full((len(ts),), 77, dtype=torch.int32, device="cuda")
            k_d, t_d = _i32(torch, ks), _i32(torch, ts)
            torch.cuda.synchronize()
            sset.emit(k_d, t_d, out=out, inline=True, key_inline=True, results=res, held=held)
            if sync:
                ctx.sync()
            return ks, ts, out, res

        def check_oracle(ks, ts, out, res, only=None):
            out, res = out.cpu().numpy(), res.cpu().numpy()
            for k, (key, t) in enumerate(zip(ks, ts)):
                if only is not None and key != only:
                    continue
                i = [m[0] for m in members].index(key)
                b, e = (int(t) >> 24) - members[i][1], int(t) & 0xFFFFFF
                assert res[k] == 0, (key, b, e)
                assert bytes(out[k, :8]) == int(key).to_bytes(4, "big") + int(t).to_bytes(4, "big")
                assert np.array_equal(out[k, 8:8 + T], srcs[i][b, e] if e < K else reps[i][b][e - K]), (key, b, e)
                assert (out[k, 8 + T:] == FILL).all()

        feed(list(range(3, K)) + [K, K + 1])  # three source symbols short, two repair symbols: not decodable
        for (key, sbn0), rx in zip(members, rxs):
            held = rx.held()
            n = int(held.numel())
            assert n == nblk * (K - 3 + 2)
            out = torch.full((n, T + 8), FILL, dtype=torch.uint8, device="cuda")
            res = torch.full((n,), 77, dtype=torch.int32, device="cuda")
            k_d = torch.full((n,), key, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            sset.emit(k_d, held, out=out, inline=True, key_inline=True, results=res, held=True)
            ctx.sync()
            check_oracle(np.full(n, key, np.uint32), held.cpu().numpy().view(np.uint32), out, res)
        ks, ts, out, res = ask(fresh, held=True)
        assert (res.cpu().numpy() == NOT_READY).all() and (out.cpu().numpy() == FILL).all()
        feed([K + 2, K + 3])
        st, _ = rset.decode()
        assert st.all()
        check_oracle(*ask(fresh))  # no call on the SenderSet in between: the emit sees the masks as they are now
        check_oracle(*ask([0, 1, 2, K + 5], held=True))
        # a reset directly behind an emit that nobody waited for
        first = ask(fresh, sync=False)
        rxs[0].reset()
        ks, ts, out2, res2 = ask(fresh)
        check_oracle(*first)
        res2, out2 = res2.cpu().numpy(), out2.cpu().numpy()
        mine = ks == members[0][0]
        assert (res2[mine] == NOT_READY).all() and (out2[mine] == FILL).all()
        check_oracle(ks, ts, torch.from_numpy(out2), torch.from_numpy(res2), only=members[1][0])
    finally:
        sset.close()
        rset.close()
        for h in hs:
            h.close()


def test_the_loop_closes_through_two_sets(ctx, torch):
    """two objects lose a fifth of their source packets; want(extra=2) of each receiver, keys from torch.full, ONE SenderSet.emit
    with key and tag inline, ONE ReceiverSet.add of the buffer as emitted: everything ADDED, every block decodes"""
    rng = np.random.default_rng(77)
    two = OBJECTS[:2]
    txs, datas = _object_senders(ctx, torch, two, seed=1)
    rxs = [nanorq_amd.ObjectReceiver(ctx, *tx.oti, rep_cap=64) for tx in txs]
    sset, rset = nanorq_amd.SenderSet(ctx, OBJ_T), nanorq_amd.ReceiverSet(ctx, OBJ_T)
    try:
        for (key, _, _, _), tx, rx in zip(two, txs, rxs):
            sset.attach(key, tx)
            rset.attach(key, rx)
        ks = np.concatenate([np.full(sum(K for K, _ in tx.blocks), key, np.uint32) for (key, _, _, _), tx in zip(two, txs)])
        ts = np.concatenate([[tag(sbn, e) for sbn, (K, _) in enumerate(tx.blocks) for e in range(K)] for tx in txs]).astype(np.uint32)
        keep = rng.permutation(np.flatnonzero(rng.random(len(ts)) >= 0.2))
        k_d, t_d = _i32(torch, ks[keep]), _i32(torch, ts[keep])
        torch.cuda.synchronize()
        first = sset.emit(k_d, t_d, inline=True, key_inline=True)
        rset.add(first, inline=True, key_inline=True)
        assert all((rx.counts()[0] > 0).any() for rx in rxs)
        wants = [rx.want(extra=2) for rx in rxs]
        assert all(w.numel() > 0 for w in wants)
        tags = torch.cat(wants)
        keys = torch.cat([torch.full((int(w.numel()),), key, dtype=torch.int32, device="cuda") for (key, _, _, _), w in zip(two, wants)])
        res_tx = torch.full((int(tags.numel()),), 77, dtype=torch.int32, device="cuda")
        res_rx = torch.full((int(tags.numel()),), 77, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        answer = sset.emit(keys, tags, inline=True, key_inline=True, results=res_tx)
        rset.add(answer, inline=True, key_inline=True, results=res_rx)
        ctx.sync()
        assert (res_tx.cpu().numpy() == 0).all() and (res_rx.cpu().numpy() == ADDED).all()
        st, _ = rset.decode()
        assert st.all()
        for rx, data in zip(rxs, datas):
            assert rx.want(extra=2).numel() == 0
            out, left = rx.write()
            ctx.sync()
            assert left == 0 and np.array_equal(out.cpu().numpy(), data)
    finally:
        sset.close()
        rset.close()
        for h in rxs + txs:
            h.close()


# ------------------------------------------------------------------------------------------------------------------ the API ----
def _tx(ctx, torch, nblk=1, sbn0=0, T=16, K=10, encode=False):
    src = torch.zeros((nblk, K, T), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    tx = nanorq_amd.Sender(ctx, K, T, nblk, src, sbn0=sbn0)
    if encode:
        tx.encode()
    return tx


def test_attach_rules(ctx, torch):
    other = nanorq_amd.Context(0)
    hs = []

    def mk(*a, **k):
        hs.append(_tx(*a, **k))
        return hs[-1]
    st, st2 = nanorq_amd.SenderSet(ctx, 16), nanorq_amd.SenderSet(ctx, 16)
    obj = _dev(torch, payload(213 * 16 - 5, seed=1))
    torch.cuda.synchronize()
    otx, otx2 = nanorq_amd.ObjectSender(ctx, obj, 16, Z=5), nanorq_amd.ObjectSender(ctx, obj, 16, Z=5)
    try:
        a = mk(ctx, torch, 4, 10)
        st.attach(1, a)
        with pytest.raises(NrqError, match="another context"):
            st.attach(2, mk(other, torch))
        with pytest.raises(NrqError, match="is not the set's"):
            st.attach(2, mk(ctx, torch, T=32))
        with pytest.raises(NrqError, match="in a set already"):
            st.attach(2, a)
        with pytest.raises(NrqError, match="in a set already"):
            st2.attach(2, a)
        for nblk, sbn0 in ((1, 10), (1, 13), (3, 8), (8, 12), (1, 12)):
            with pytest.raises(NrqError, match="overlap"):
                st.attach(1, mk(ctx, torch, nblk, sbn0))
        st.attach(2, mk(ctx, torch, 4, 10))   # the same span under another key
        st.attach(1, mk(ctx, torch, 2, 14))   # another span under the same key, touching it on either side
        st.attach(1, mk(ctx, torch, 10, 0))
        with pytest.raises(NrqError, match="owns its key"):
            st.attach(1, otx)                 # an object under a key that has members
        st.attach(3, otx)
        with pytest.raises(NrqError, match="owns its key"):
            st.attach(3, mk(ctx, torch, 1, 100))  # a member under an object's key, even beside its blocks
        with pytest.raises(NrqError, match="owns its key"):
            st.attach(3, otx2)
        with pytest.raises(NrqError, match="in a set already"):
            st2.attach(3, otx)
        bk, bs = st.blocks()
        assert list(bk) == [1] * 16 + [2] * 4 + [3] * 5 and list(bs) == list(range(16)) + [10, 11, 12, 13] + list(range(5))
        with pytest.raises(NrqError, match="no member under key"):
            st.detach(99)
        st.detach(3)
        st2.attach(3, otx)                    # detached: free to join another set
        st.detach(1)
        st.attach(7, a)
        assert list(st.blocks()[0]) == [2] * 4 + [7] * 4
    finally:
        for h in [st, st2, otx, otx2] + hs:
            h.close()
        other.close()


def test_caps(ctx, torch):
    hs = [_tx(ctx, torch, encode=True) for _ in range(nanorq_amd.TXSET_MAX_SEGS + 1)]
    big = [_tx(ctx, torch, 256, encode=i == 3) for i in range(4)] + [_tx(ctx, torch, 1)]
    st, st2 = nanorq_amd.SenderSet(ctx, 16), nanorq_amd.SenderSet(ctx, 16)
    try:
        for i, h in enumerate(hs[:-1]):
            st.attach(i, h)
        with pytest.raises(NrqError, match="at most 64 table segments"):
            st.attach(1000, hs[-1])
        for i, h in enumerate(big[:-1]):
            st2.attach(i, h)
        with pytest.raises(NrqError, match="at most 1024 blocks"):
            st2.attach(1000, big[-1])
        # the full set still emits: one packet of its last member (rows of zeros: a packet of zeros)
        pk, res = _emit(torch, ctx, st, np.array([63], np.uint32), np.array([tag(0, 12)], np.uint32), 8, 32)
        assert res[0] == 0 and bytes(pk[0, :8]) == (63).to_bytes(4, "big") + tag(0, 12).to_bytes(4, "big") and (pk[0, 8:24] == 0).all()
        with pytest.raises(NrqError, match="key 0 is not encoded"):  # (members 0 .. 2 of the block-full set are not encoded)
            _emit(torch, ctx, st2, np.array([3], np.uint32), np.array([tag(255, 3)], np.uint32), 0, 16)
    finally:
        for h in [st, st2] + hs + big:
            h.close()


def test_emit_argument_errors(ctx, torch):
    T = 16
    L = ctx._L
    a, raw = _tx(ctx, torch, encode=True), _tx(ctx, torch, sbn0=5)
    st, empty = nanorq_amd.SenderSet(ctx, T), nanorq_amd.SenderSet(ctx, T)
    try:
        st.attach(0, a)
        pk = torch.full((4, T + 8), FILL, dtype=torch.uint8, device="cuda")
        kt = torch.zeros(4, dtype=torch.int32, device="cuda")
        res = torch.full((4,), 77, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        P, KT = C.c_void_p(pk.data_ptr()), C.c_void_p(kt.data_ptr())

        def emit(stride, keys, tags, n, flags, s=st, pkts=P):
            return L.nrq_txset_emit(s._h, keys, tags, n, pkts, stride, flags, C.c_void_p(res.data_ptr()))
        TAG, HELD, KEY = nanorq_amd.TX_TAG_INLINE, nanorq_amd.TX_HELD, nanorq_amd.TX_KEY_INLINE
        assert emit(T + 8, KT, KT, 4, KEY) == -1 and b"NRQ_TX_TAG_INLINE" in L.nrq_ctx_error(ctx._h)   # key inline without tag inline
        assert emit(T + 8, KT, KT, 4, 8) == -1 and b"unknown flags" in L.nrq_ctx_error(ctx._h)
        assert emit(T - 1, KT, KT, 4, 0) == -1 and emit(T + 3, KT, KT, 4, TAG) == -1 and emit(T + 7, KT, KT, 4, TAG | KEY) == -1
        assert b"shorter than a packet" in L.nrq_ctx_error(ctx._h)
        assert emit(T, KT, KT, 4, 0, pkts=None) == -1 and emit(T, KT, None, 4, 0) == -1
        assert emit(T + 8, KT, KT, 4, KEY, s=empty) == -1                                               # flag errors come first
        assert emit(T, KT, KT, 0, 0) == 0 and emit(T, KT, KT, 4, 0, s=empty) == 0                       # n == 0, an empty set
        ctx.sync()
        assert (res.cpu().numpy() == 77).all() and (pk.cpu().numpy() == FILL).all()                    # nothing was enqueued
        assert emit(T, KT, KT, 4, 0) == 0 and emit(T + 4, None, KT, 4, TAG) == 0 and emit(T + 8, KT, KT, 4, TAG | KEY | HELD) == 0
        ctx.sync()
        assert (res.cpu().numpy() == 0).all()                                                           # HELD on a set of plain senders
        st.emit(kt, kt, out=pk, results=None)                                                           # d_results may be NULL
        st.attach(1, raw)
        assert emit(T, KT, KT, 4, 0) == -1 and b"key 1 is not encoded" in L.nrq_ctx_error(ctx._h)
        raw.encode()
        assert emit(T, KT, KT, 4, 0) == 0
        ctx.sync()
    finally:
        for h in (st, empty, a, raw):
            h.close()


def test_lifetimes(ctx, torch):
    """after detach that key's packets are no member's; a member closed before the set leaves it; a relay whose reception was
    closed makes the emit fail, naming its key, until it is detached; the set closed first leaves its members ordinary senders"""
    T = 16
    a, b, c = (_tx(ctx, torch, 2, 0, encode=True) for _ in range(3))
    rx = nanorq_amd.Receiver(ctx, 10, T, 2, 2)
    relay = rx.relay()
    st = nanorq_amd.SenderSet(ctx, T)
    keys = np.array([1, 2, 3, 1, 2, 3], np.uint32)
    tags = np.array([tag(0, 1)] * 3 + [tag(1, 11)] * 3, np.uint32)
    try:
        for k, h in ((1, a), (2, b), (3, c)):
            st.attach(k, h)

        def emit():
            return _emit(torch, ctx, st, keys, tags, 8, 32)[1].tolist()
        assert emit() == [0] * 6
        st.detach(2)
        assert emit() == [0, -1, 0, 0, -1, 0]
        c.close()
        assert emit() == [0, -1, -1, 0, -1, -1] and list(st.blocks()[0]) == [1, 1]
        st.attach(3, b)  # (the key of the closed member is free again)
        assert emit() == [0, -1, 0, 0, -1, 0]
        st.attach(2, relay)
        assert emit() == [0, NOT_READY, 0, 0, NOT_READY, 0]
        rx.close()
        with pytest.raises(NrqError, match="relay under key 2 was destroyed"):
            emit()
        st.detach(2)
        assert emit() == [0, -1, 0, 0, -1, 0]
        st.close()
        for h in (a, b):   # the former members are ordinary senders: their own emit, and another set
            t_d = _i32(torch, tags)
            res = torch.full((6,), 77, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            h.emit(t_d, inline=True, results=res)
            ctx.sync()
            assert res.cpu().tolist() == [0] * 6
        with nanorq_amd.SenderSet(ctx, T) as st3:
            st3.attach(1, a)
            a.close()      # the member first, then the set
        with nanorq_amd.SenderSet(ctx, T) as st4:
            st4.attach(1, b)
    finally:
        for h in (st, relay, rx, a, b, c):
            h.close()


def test_failing_runtime_calls(torch):
    """fail_after on a context of its own: the n-th checked runtime call of nrq_txset_attach, and of an nrq_txset_emit that has to
    grow its scratch, fails.  The call returns an error and nothing is half attached; the next call succeeds and matches the
    emulation."""
    import gpu_support as G
    G.ctx()  # (torch first, as every context of this process)
    T, mix = 16, [MIX4[0], MIX4[2]]  # (two keys)
    rng = np.random.default_rng(5)
    failed = {"attach": 0, "emit": 0}
    texts = []
    for what in ("attach", "emit"):
        for n_fail in range(1, 10):
            fctx = nanorq_amd.Context(0)  # (a pool of its own, empty: the scratch allocation reaches the runtime)
            m = _Senders(fctx, torch, mix, T, seed=n_fail)
            try:
                keys, tags = keyed_tags(rng, m.segs, 600)
                err = None
                if what == "attach":
                    m.set.detach(mix[1][0])
                    fctx.set_option("fail_after", n_fail)
                    try:
                        m.set.attach(mix[1][0], m.tx[1])
                    except NrqError as e:
                        err = str(e)
                    fctx.set_option("fail_after", 0)
                    if err is not None:
                        assert list(m.set.blocks()[0]) == [mix[0][0]] * mix[0][2], err  # nothing half attached
                        pk, res = _emit(torch, fctx, m.set, keys, tags, 8, 32)
                        epk, eres, _ = emu_txset_emit(m.segs[:1], keys, tags, 8, 32)
                        assert np.array_equal(res, eres) and np.array_equal(pk, epk), err
                        m.set.attach(mix[1][0], m.tx[1])
                else:
                    _emit(torch, fctx, m.set, keys[:4], tags[:4], 8, 32)  # (a first scratch: the larger call has to replace it)
                    fctx._chk(fctx._L.nrq_dev_trim(fctx._h))              # (nothing cached: the new one comes from the runtime)
                    out = torch.full((len(tags), 32), FILL, dtype=torch.uint8, device="cuda")
                    k_d, t_d = _i32(torch, keys), _i32(torch, tags)
                    torch.cuda.synchronize()
                    fctx.set_option("fail_after", n_fail)
                    try:
                        m.set.emit(k_d, t_d, out=out, inline=True, key_inline=True)  # (the emit alone: no wait of the test's behind it)
                    except NrqError as e:
                        err = str(e)
                    fctx.set_option("fail_after", 0)
                    fctx.sync()
                if err is not None:
                    failed[what] += 1
                    texts.append(err)
                pk, res = _emit(torch, fctx, m.set, keys, tags, 8, 32)
                epk, eres, _ = emu_txset_emit(m.segs, keys, tags, 8, 32)
                assert np.array_equal(res, eres) and np.array_equal(pk, epk), err
            finally:
                m.close()
                fctx.close()
            if err is None:
                break  # (the call makes fewer than n_fail checked runtime calls)
    assert failed["attach"] == 3 and failed["emit"] == 6, (failed, texts)
    assert any("hipMalloc" in t for t in texts) and any("hipStreamSynchronize" in t for t in texts) and any("hipMemcpy" in t for t in texts)
