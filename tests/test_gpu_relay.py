"""GPU tier of the relays (nrq_rx_relay / nrq_orx_relay, nanorq_amd.Receiver.relay() / ObjectReceiver.relay()): a transmission
made from a reception, over the reception's own rows, that emits any (SBN, ESI) of every block the reception has completed.

Expected payloads come from the oracle's encode of the ORIGINAL source data (orc.encode_block), never from this library's own
sender; the object tests compare with an ObjectSender over the original object, byte for byte, and close the loop through a
second receiver (SHA-256).  Receptions carry two symbols of overhead per block and the oracle's own decode verdict is asserted
first, so no case depends on a lucky rank."""
import hashlib

import numpy as np
import pytest

import nanorq_amd
from nanorq_amd import EXT_PER_BLOCK_KP, EXT_SUBBLOCKS, TX_NOT_READY, NrqError
from tx_support import FILL, range_tags, tag
from util import loss_pattern, payload

pytestmark = pytest.mark.gpu

KINDS = ["forced", "default"]


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available()
    return t


@pytest.fixture(scope="module")
def ctx(torch):
    import gpu_support as G
    return G.ctx()


def _ctx(kind):
    import gpu_support as G
    return G.ctx(kind)


def _dev(torch, a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()  # (torch's stream and the library's are not ordered)
    return t


def _host(ctx, torch, t):
    ctx.sync()
    return t.cpu().numpy()


class Block:
    """one block of a test reception: the original source, what was lost, and the repair symbols that arrived"""

    def __init__(self, orc, K, T, Kp, src, lost, rep_esis):
        self.orc, self.K, self.T, self.Kp = orc, K, T, Kp
        self.src = src
        self.lost = np.asarray(lost, np.uint32)
        self.keep = np.setdiff1d(np.arange(K, dtype=np.uint32), self.lost)
        self.rep_esis = np.asarray(rep_esis, np.uint32)
        self.rep = self.symbols(self.rep_esis)

    def symbols(self, esis):
        """the oracle's payload of every ESI of the list (source rows below K)"""
        esis = np.asarray(esis, np.uint32)
        out = np.zeros((len(esis), self.T), np.uint8)
        lo = esis < self.K
        out[lo] = self.src[esis[lo]]
        if (~lo).any():
            out[~lo] = self.orc.encode_block(self.src, self.K, self.T, esis[~lo], Kp=self.Kp)[0]
        return out

    def oracle_decodes(self, esis=None, syms=None):
        if esis is None:
            esis, syms = np.concatenate([self.keep, self.rep_esis]), np.concatenate([self.src[self.keep], self.rep])
        ok, out, _ = self.orc.decode_block(esis, syms, self.K, self.T, Kp=self.Kp, max_esi=(1 << 24) - 1)
        return ok and np.array_equal(out, self.src)


def _lossy_blocks(orc, K, T, nblk, Kp, seed, loss=0.1, max_esi=None):
    """blocks that lost `loss` of their source symbols and received as many repair symbols plus two, their ESIs scattered over
    (K, max_esi]"""
    row = nanorq_amd.params(Kp or K)["Kp"]
    max_esi = max_esi or 2 * row
    rng = np.random.default_rng(seed)
    out = []
    for b in range(nblk):
        src = payload(K * T, seed=seed, block=b).reshape(K, T)
        lost = loss_pattern(K, loss, seed, block=b)
        if len(lost) == 0:
            lost = np.array([K // 2], np.uint32)
        esis = rng.choice(np.arange(K, max_esi + 1), len(lost) + 2, replace=False).astype(np.uint32)
        out.append(Block(orc, K, T, Kp, src, lost, esis))
    return out


def _feed(torch, rx, blocks, sbn0, which=None):
    """the blocks' received packets (kept source rows, then the repair symbols in list order) into the reception, in one call"""
    tags, rows = [], []
    for b, blk in enumerate(blocks):
        if which is not None and b not in which:
            continue
        es = np.concatenate([blk.keep, blk.rep_esis])
        tags.append(((sbn0 + b) << 24) | es.astype(np.uint32))
        rows.append(np.concatenate([blk.src[blk.keep], blk.rep]))
    tags, rows = np.concatenate(tags).astype(np.uint32), np.concatenate(rows)
    rx.add(_dev(torch, rows), tags=_dev(torch, tags.view(np.int32)))


def _emit_and_check(ctx, torch, relay, tags, expect, T, inline, slack, sbn0=0, nblk=None):
    """relay.emit(tags) into a buffer with guard rows on both sides: packet k holds expect[k] (None: the packet must stay
    untouched, with -1 for a foreign SBN and -2 for a block of the span that is not ready)"""
    n = len(tags)
    stride = T + (4 if inline else 0) + slack
    buf = torch.full((n + 2, stride), FILL, dtype=torch.uint8, device="cuda")
    res = torch.full((n,), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    relay.emit(_dev(torch, np.asarray(tags, np.uint32).view(np.int32)), out=buf[1:n + 1], inline=inline, results=res)
    pk, res = _host(ctx, torch, buf), _host(ctx, torch, res)
    assert (pk[0] == FILL).all() and (pk[n + 1] == FILL).all(), "guard rows"
    pk = pk[1:n + 1]
    off = 4 if inline else 0
    for k, t in enumerate(tags):
        if expect[k] is None:
            b = (int(t) >> 24) - sbn0
            want = -1 if not 0 <= b < nblk else TX_NOT_READY
            assert res[k] == want, (k, hex(int(t)), res[k])
            assert (pk[k] == FILL).all(), k
            continue
        assert res[k] == 0, (k, hex(int(t)), res[k])
        if inline:
            assert bytes(pk[k, :4]) == int(t).to_bytes(4, "big"), k
        assert np.array_equal(pk[k, off:off + T], expect[k]), (k, hex(int(t)))
        assert (pk[k, off + T:] == FILL).all(), k


def _tag_list(rng, blocks, sbn0, per_block=24):
    """per block: source ESIs (lost and received ones), repair ESIs the reception received, repair ESIs it never saw (some beyond
    2 K', some next to 2^24); plus two foreign SBNs.  -> (tags, expected payloads)"""
    tags, expect = [], []
    for b, blk in enumerate(blocks):
        K = blk.K
        es = list(blk.lost[:4]) + list(blk.keep[:3]) + [0, K - 1] + list(blk.rep_esis[:4])
        es += [int(x) for x in rng.integers(K, 2 * K, 4)] + [int(x) for x in rng.integers(4 * K, 1 << 23, 3)]
        es += [(1 << 24) - 1, (1 << 24) - 1 - b, K]
        es = np.array(es[:per_block], np.uint32)
        sy = blk.symbols(es)
        tags += [tag(sbn0 + b, e) for e in es]
        expect += list(sy)
    for sbn in (sbn0 - 1, sbn0 + len(blocks)):
        if 0 <= sbn < 256:
            tags.append(tag(sbn, 1))
            expect.append(None)
    order = rng.permutation(len(tags))
    return np.array(tags, np.uint32)[order], [expect[i] for i in order]


# ------------------------------------------------------------------------------------------------ 1. relay equals origin ----
# (K, T, nblk, sbn0, K' (0: K's own row)): the device planner's sizes; 16-byte, dword and byte rows (T = 100 and 1288 leave the
# relay's intermediate rows unaligned too); K = 15000 at T = 16 / 24: the narrow strips with the split back-substitution
ORIGIN_CASES = [
    (100, 16, 3, 5, 0),
    (100, 100, 3, 253, 0),
    (100, 1280, 2, 1, 127),      # K' above K's own row (101)
    (1000, 1280, 3, 2, 0),
    (1000, 1288, 2, 9, 0),
    (1000, 100, 2, 1, 0),
    (8192, 1280, 2, 1, 0),
    (8192, 16, 2, 200, 0),
    (15000, 16, 2, 1, 0),
    (15000, 24, 1, 3, 0),
]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("K,T,nblk,sbn0,Kp", ORIGIN_CASES)
def test_relay_equals_origin(torch, orc, K, T, nblk, sbn0, Kp, kind):
    ctx = _ctx(kind)
    blocks = _lossy_blocks(orc, K, T, nblk, Kp, seed=K + T)
    for b, blk in enumerate(blocks):
        assert blk.oracle_decodes(), "the oracle does not decode block %d of this reception" % b
    rng = np.random.default_rng(K * 7 + T)
    with nanorq_amd.Receiver(ctx, K, T, nblk, rep_cap=len(max((b.lost for b in blocks), key=len)) + 8, sbn0=sbn0, Kp=Kp) as rx:
        with rx.relay() as relay:
            assert not relay.ready().any()
            _feed(torch, rx, blocks, sbn0)
            st, used = rx.decode()
            assert st.all(), st
            assert relay.ready().all()
            for b, blk in enumerate(blocks):  # the reception itself is still right
                assert np.array_equal(_host(ctx, torch, rx.source[b]), blk.src), b
            tags, expect = _tag_list(rng, blocks, sbn0)
            for inline, slack in ((False, 0), (True, 0), (False, 16), (True, 12 if T % 16 == 0 else 3)):
                _emit_and_check(ctx, torch, relay, tags, expect, T, inline, slack, sbn0=sbn0, nblk=nblk)
            # the range form over all blocks: source symbols and the first repair ESIs
            n = K + 3 if K <= 1000 else 40
            esi0 = 0 if K <= 1000 else K - 20
            pk = _host(ctx, torch, relay.emit_range(esi0, n, interleave=True, inline=False))
            rt = range_tags(nblk, sbn0, esi0, n, True)
            want = {b: blk.symbols(np.arange(esi0, esi0 + n)) for b, blk in enumerate(blocks)}
            for k, t in enumerate(rt):
                assert np.array_equal(pk[k], want[(int(t) >> 24) - sbn0][(int(t) & 0xFFFFFF) - esi0]), (k, hex(int(t)))


# ------------------------------------------------------------------------------------------------------ 2. mixed states ----
def _singular_case(K, seed0=1):
    """a loss pattern and as many repair ESIs whose system is rank deficient (host planner), and one more repair ESI that
    completes it: the seeded search of tests/test_gpu_rx.py, which returns None instead of skipping"""
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
    return None


def test_mixed_states(ctx, torch, orc):
    """blocks 0 and 4 lose nothing, 1 and 5 are decoded, 2 is rank deficient until one more packet, 3 has too few symbols"""
    K, T, nblk, sbn0 = 100, 32, 6, 2
    found = _singular_case(K)
    assert found is not None, "no rank deficient pattern found"
    s_lost, s_reps, s_extra = found
    src = [payload(K * T, seed=21, block=b).reshape(K, T) for b in range(nblk)]
    none = np.zeros(0, np.uint32)
    lossy = _lossy_blocks(orc, K, T, nblk, 0, seed=21)
    blocks = [Block(orc, K, T, 0, src[0], none, none), lossy[1], Block(orc, K, T, 0, src[2], s_lost, s_reps),
              Block(orc, K, T, 0, src[3], [3, 40, 41, 77, 99], [K + 5, K + 9, K + 1]), Block(orc, K, T, 0, src[4], none, none), lossy[5]]
    assert blocks[1].oracle_decodes() and blocks[5].oracle_decodes()
    later = {2: np.array([s_extra], np.uint32), 3: np.array([K + 50, K + 2, K + 70, K + 71], np.uint32)}
    for b, es in later.items():
        blk, all_rep = blocks[b], np.concatenate([blocks[b].rep_esis, es])
        assert blk.oracle_decodes(np.concatenate([blk.keep, all_rep]), np.concatenate([blk.src[blk.keep], blk.symbols(all_rep)])), b
    rng = np.random.default_rng(5)
    ctx.ktime_enable(True)
    try:
        with nanorq_amd.Receiver(ctx, K, T, nblk, rep_cap=40, sbn0=sbn0) as rx, rx.relay() as relay:
            _feed(torch, rx, blocks, sbn0)
            st, _ = rx.decode()
            assert list(st) == [1, 1, 0, 0, 1, 1]
            assert list(relay.ready()) == [False, True, False, False, False, True]
            ctx.ktime_read()
            relay.encode()
            assert len(ctx.ktime_read()) >= 1, "the loss-free blocks need a solve"
            assert list(relay.ready()) == [True, True, False, False, True, True]
            relay.encode()
            assert ctx.ktime_read() == [], "an encode with nothing left to make ready launched a solve"
            tags, expect = _tag_list(rng, blocks, sbn0)
            for k, t in enumerate(tags):
                if (int(t) >> 24) - sbn0 in (2, 3):
                    expect[k] = None
            assert sum(e is None for e in expect) > 20
            _emit_and_check(ctx, torch, relay, tags, expect, T, True, 8, sbn0=sbn0, nblk=nblk)
            with pytest.raises(NrqError, match=r"not ready: SBN 4, 5 \(2 of 6\)"):
                relay.emit_range(0, K + 4)
            # the packets the two blocks lack
            for b, es in later.items():
                rx.add(_dev(torch, blocks[b].symbols(es)), tags=_dev(torch, (((sbn0 + b) << 24) | es).astype(np.uint32).view(np.int32)))
            st, used = rx.decode()
            assert st.all() and used[2] == len(s_lost) + 1
            ctx.ktime_read()
            relay.encode()
            assert ctx.ktime_read() == [], "every block was made ready by a decode: nothing to encode"
            assert relay.ready().all()
            n = K + 6
            pk = _host(ctx, torch, relay.emit_range(0, n, interleave=False, inline=True))
            rt = range_tags(nblk, sbn0, 0, n, False)
            for b, blk in enumerate(blocks):
                want = blk.symbols(np.arange(n))
                for i in range(n):
                    k = b * n + i
                    assert bytes(pk[k, :4]) == int(rt[k]).to_bytes(4, "big")
                    assert np.array_equal(pk[k, 4:4 + T], want[i]), (b, i)
    finally:
        ctx.ktime_enable(False)


# -------------------------------------------------------------------------------------------------------- 3. attach late ----
@pytest.mark.parametrize("kind", KINDS)
def test_attach_late(torch, orc, kind):
    ctx = _ctx(kind)
    K, T, nblk, sbn0 = 1000, 48, 3, 4
    blocks = _lossy_blocks(orc, K, T, nblk, 0, seed=33)
    assert all(b.oracle_decodes() for b in blocks)
    rng = np.random.default_rng(8)
    with nanorq_amd.Receiver(ctx, K, T, nblk, rep_cap=200, sbn0=sbn0) as rx:
        _feed(torch, rx, blocks, sbn0)
        st, _ = rx.decode()
        assert st.all()
        with rx.relay() as relay:
            assert not relay.ready().any()
            tags, expect = _tag_list(rng, blocks, sbn0)
            held = [e if (int(t) >> 24) - sbn0 not in range(nblk) else None for t, e in zip(tags, expect)]
            _emit_and_check(ctx, torch, relay, tags, held, T, False, 0, sbn0=sbn0, nblk=nblk)
            st, _ = rx.decode()  # nothing to decode: nothing becomes ready
            assert st.all() and not relay.ready().any()
            relay.encode()
            assert relay.ready().all()
            _emit_and_check(ctx, torch, relay, tags, expect, T, False, 0, sbn0=sbn0, nblk=nblk)
            _emit_and_check(ctx, torch, relay, tags, expect, T, True, 4, sbn0=sbn0, nblk=nblk)


# ------------------------------------------------------------------------------------------------------------ 4. objects ----
# (Kt, T, Z, N, Al, flags): the headline object's shape scaled down -- two block classes (3 blocks of K = 43, 2 of 42), F not a
# multiple of T; K' = 46 for both classes, or 46 / 42 with NANORQ_EXT_PER_BLOCK_KP
OBJ_CASES = [
    (213, 64, 5, 1, 8, 0),
    (213, 96, 5, 3, 8, EXT_SUBBLOCKS),
    (213, 64, 5, 1, 8, EXT_PER_BLOCK_KP),
    (213, 100, 5, 1, 4, EXT_PER_BLOCK_KP),   # dword rows
]


def _object(torch, Kt, T, seed):
    F = Kt * T - 37
    data = payload(F, seed=seed)
    return data, _dev(torch, data)


def _select(tags, blocks, rng, lose, rep_lo, rep_n, whole=()):
    """packet indices of a reception out of an emit_all: per block every source packet but `lose` random ones (blocks in `whole`
    lose nothing) and the repair packets number rep_lo .. rep_lo + lost + rep_n - 1; shuffled"""
    sbn, esi = tags >> 24, tags & 0xFFFFFF
    keep = np.zeros(len(tags), bool)
    lost = {}
    for b, (K, _) in enumerate(blocks):
        gone = np.zeros(0, np.int64) if b in whole else rng.choice(K, lose, replace=False)
        lost[b] = np.sort(gone)
        mine = sbn == b
        keep |= mine & (esi < K) & ~np.isin(esi, gone)
        if len(gone):
            keep |= mine & (esi >= K + rep_lo) & (esi < K + rep_lo + len(gone) + rep_n)
    idx = np.flatnonzero(keep)
    rng.shuffle(idx)
    return idx, lost


def _oracle_decodes_object(orc, pkts, tags, idx, blocks, T, max_esi):
    """the oracle's verdict per block on the inline packets pkts[idx] (arrival order): every block must decode"""
    sbn, esi = tags[idx] >> 24, tags[idx] & 0xFFFFFF
    for b, (K, Kp) in enumerate(blocks):
        mine = sbn == b
        if (esi[mine] < K).sum() == K:
            continue
        ok, _, _ = orc.decode_block(esi[mine], pkts[idx[mine], 4:4 + T], K, T, Kp=Kp, max_esi=max_esi)
        assert ok, "the oracle does not decode block %d of this reception" % b


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", OBJ_CASES)
def test_object_relay(torch, orc, case, kind):
    ctx = _ctx(kind)
    Kt, T, Z, N, Al, flags = case
    data, obj = _object(torch, Kt, T, seed=Kt + T + N)
    want_sha = hashlib.sha256(data.tobytes()).hexdigest()
    rng = np.random.default_rng(T + N)
    nrep = 40
    with nanorq_amd.ObjectSender(ctx, obj, T, Z=Z, N=N, Al=Al, flags=flags) as tx:
        p = tx.params
        assert p.ZL and p.ZS and p.F % T and (p.KpL != p.KpS) == bool(flags & EXT_PER_BLOCK_KP)
        tx.encode()
        n = tx.count_all(nrep)
        t_il = torch.zeros(n, dtype=torch.int32, device="cuda")
        t_bm = torch.zeros(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ref_il = _host(ctx, torch, tx.emit_all(nrep, interleave=True, inline=True, tags_out=t_il))
        ref_bm = _host(ctx, torch, tx.emit_all(nrep, interleave=False, inline=False, tags_out=t_bm))
        t_il, t_bm = t_il.cpu().numpy().view(np.uint32), t_bm.cpu().numpy().view(np.uint32)
        oti = tx.oti
        blocks = tx.blocks
    idx, lost = _select(t_il, blocks, rng, lose=6, rep_lo=0, rep_n=2, whole=(1,))
    _oracle_decodes_object(orc, ref_il, t_il, idx, blocks, T, p.max_esi)
    with nanorq_amd.ObjectReceiver(ctx, *oti, flags=flags, rep_cap=48) as rx, rx.relay() as relay:
        assert relay.oti == oti and relay.blocks == blocks
        rx.add(_dev(torch, ref_il[idx]), inline=True)
        st, _ = rx.decode()
        assert st.all(), st
        assert list(relay.ready()) == [b != 1 for b in range(Z)]
        with pytest.raises(NrqError, match=r"not ready: SBN 1 \(1 of 5\)"):
            relay.emit_all(nrep)
        relay.encode()
        assert relay.ready().all()
        g_il = torch.zeros(n, dtype=torch.int32, device="cuda")
        g_bm = torch.zeros(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        got_il = _host(ctx, torch, relay.emit_all(nrep, interleave=True, inline=True, tags_out=g_il))
        got_bm = _host(ctx, torch, relay.emit_all(nrep, interleave=False, inline=False, tags_out=g_bm))
        assert np.array_equal(g_il.cpu().numpy().view(np.uint32), t_il) and np.array_equal(g_bm.cpu().numpy().view(np.uint32), t_bm)
        got_il, ref_il = got_il[:, :T + 4], ref_il[:, :T + 4]  # (the bytes between a packet's end and the stride are nobody's)
        assert np.array_equal(got_il, ref_il), np.flatnonzero((got_il != ref_il).any(1))[:8]
        assert np.array_equal(got_bm, ref_bm), np.flatnonzero((got_bm != ref_bm).any(1))[:8]
        # a tag list over the object, one packet at a time against the origin's
        pick = rng.choice(n, 200, replace=False)
        tl = np.concatenate([t_bm[pick], [tag(Z, 0)]]).astype(np.uint32)
        res = torch.full((len(tl),), 77, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        pk = _host(ctx, torch, relay.emit(_dev(torch, tl.view(np.int32)), results=res))
        assert np.array_equal(pk[:-1], ref_bm[pick]) and list(res.cpu().numpy()) == [0] * 200 + [-1]
        # a second receiver fed with relay-made REPAIR packets and five source packets per block
        sbn, esi = t_il >> 24, t_il & 0xFFFFFF
        Ks = np.array([K for K, _ in blocks])[sbn]
        take = np.flatnonzero((esi < 5) | ((esi >= Ks) & (esi < 2 * Ks - 5 + 2)))
        rng.shuffle(take)
        _oracle_decodes_object(orc, ref_il, t_il, take, blocks, T, p.max_esi)  # (the origin's packets: the relay's were shown equal)
        with nanorq_amd.ObjectReceiver(ctx, *oti, flags=flags, rep_cap=48) as rx2:
            rx2.add(_dev(torch, got_il[take]), inline=True)
            st, _ = rx2.decode()
            assert st.all(), st
            out, left = rx2.write()
            assert left == 0 and hashlib.sha256(_host(ctx, torch, out).tobytes()).hexdigest() == want_sha


# ------------------------------------------------------------------------------------------------------------- 5. chains ----
@pytest.mark.parametrize("kind", KINDS)
def test_chain_of_relays(torch, orc, kind):
    """origin -> relay A -> relay B: A receives every source packet but six per block and repair packets 0 .. 7; B receives,
    from A, only what A did NOT receive -- the six source symbols A recovered and repair packets from number 8 on"""
    ctx = _ctx(kind)
    Kt, T, Z, N, Al, flags = OBJ_CASES[1]
    data, obj = _object(torch, Kt, T, seed=99)
    want_sha = hashlib.sha256(data.tobytes()).hexdigest()
    rng = np.random.default_rng(12)
    nrep = 48
    with nanorq_amd.ObjectSender(ctx, obj, T, Z=Z, N=N, Al=Al, flags=flags) as tx:
        tx.encode()
        n = tx.count_all(nrep)
        t_o = torch.zeros(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ref = _host(ctx, torch, tx.emit_all(nrep, inline=True, tags_out=t_o))
        t_o = t_o.cpu().numpy().view(np.uint32)
        oti, blocks, max_esi = tx.oti, tx.blocks, tx.params.max_esi
    idx_a, lost_a = _select(t_o, blocks, rng, lose=6, rep_lo=0, rep_n=2)
    sbn, esi = t_o >> 24, t_o & 0xFFFFFF
    Ks = np.array([K for K, _ in blocks])[sbn]
    a_lost = np.zeros(n, bool)
    for b in range(Z):
        a_lost |= (sbn == b) & np.isin(esi, lost_a[b])
    idx_b = np.flatnonzero(a_lost | ((esi >= Ks + 8) & (esi < Ks + 8 + (Ks - 6) + 2)))
    assert not np.intersect1d(idx_a, idx_b).size
    rng.shuffle(idx_b)
    _oracle_decodes_object(orc, ref, t_o, idx_a, blocks, T, max_esi)
    _oracle_decodes_object(orc, ref, t_o, idx_b, blocks, T, max_esi)
    with nanorq_amd.ObjectReceiver(ctx, *oti, flags=flags, rep_cap=56) as rx_a, rx_a.relay() as relay_a:
        rx_a.add(_dev(torch, ref[idx_a]), inline=True)
        assert rx_a.decode()[0].all() and relay_a.ready().all()
        from_a = relay_a.emit_all(nrep, inline=True)
        ctx.sync()
        with nanorq_amd.ObjectReceiver(ctx, *oti, flags=flags, rep_cap=56) as rx_b, rx_b.relay() as relay_b:
            rx_b.add(from_a[_dev(torch, idx_b)].contiguous(), inline=True)
            assert rx_b.decode()[0].all() and relay_b.ready().all()
            out, left = rx_b.write()
            assert left == 0 and hashlib.sha256(_host(ctx, torch, out).tobytes()).hexdigest() == want_sha
            assert np.array_equal(_host(ctx, torch, relay_b.emit_all(nrep, inline=True))[:, :T + 4], ref[:, :T + 4])


# ------------------------------------------------------------------------------------- 6. no effect without a relay ----
STAT_FIELDS = ("strip_bytes", "planner", "plan_wg_threads", "backsub_strip", "wg_threads", "host_planned")


@pytest.mark.parametrize("K,T,nblk", [(1000, 64, 5), (15000, 16, 3)])
def test_no_effect_without_a_relay(ctx, torch, orc, K, T, nblk):
    """A reception without a relay decodes as the same reception does through decode_blocks_lazy WITHOUT intermediate symbols:
    statuses, `used`, recovered bytes and the launch choices nrq_call_stats reports.  There is no stats field for the
    back-substitution's view (all pivots / the needed ones): that nrq_rx_decode passes an `inter` only while a relay is attached
    -- and so keeps the needed-pivot view otherwise -- is for the review of nrq_rx_decode; what a run can show is shown here, and
    the last part shows that the same reception WITH a relay does change the call (its intermediate symbols get written)."""
    blocks = _lossy_blocks(orc, K, T, nblk, 0, seed=K + 1)
    blocks[1] = Block(orc, K, T, 0, blocks[1].src, np.zeros(0, np.uint32), np.zeros(0, np.uint32))             # nothing lost
    blocks[2] = Block(orc, K, T, 0, blocks[2].src, blocks[2].lost, blocks[2].rep_esis[:len(blocks[2].lost) - 1])  # too few
    rep_cap = max(len(b.rep_esis) for b in blocks) + 4
    L = nanorq_amd.params(K)["L"]

    def receive(with_relay):
        with nanorq_amd.Receiver(ctx, K, T, nblk, rep_cap=rep_cap) as rx:
            relay = rx.relay() if with_relay else None
            _feed(torch, rx, blocks, 0)
            lost, reps = rx.lists()
            before = _host(ctx, torch, rx.source).copy()
            rows = ctx.download(rx.rep_ptr, nblk * rep_cap * T).reshape(nblk, rep_cap, T).copy()
            st, used = rx.decode()
            stats = ctx.stats()
            after = _host(ctx, torch, rx.source).copy()
            inter = None
            if relay is not None:
                inter = ctx.download(relay.inter_ptr, nblk * L * T).reshape(nblk, L, T).copy()
                relay.close()
            return lost, reps, before, rows, st, used, stats, after, inter

    lost, reps, before, rows, st, used, stats, after, _ = receive(False)
    assert list(st) == [1, 1, 0] + [1] * (nblk - 3)
    sel = [b for b in range(nblk) if len(lost[b]) and len(reps[b]) >= len(lost[b])]
    ns = len(sel)
    lc, rc = max(len(lost[b]) for b in sel), max(len(reps[b]) for b in sel)
    h_lost, h_resi = np.zeros((ns, lc), np.uint32), np.zeros((ns, rc), np.uint32)
    for i, b in enumerate(sel):
        h_lost[i, :len(lost[b])] = lost[b]
        h_resi[i, :len(reps[b])] = reps[b]
    nl = np.array([len(lost[b]) for b in sel], np.uint32)
    av = np.array([len(reps[b]) for b in sel], np.uint32)
    nu = np.minimum(av, nl + 2)
    d_src, d_rep = _dev(torch, before[sel]), _dev(torch, rows[sel][:, :rc].copy())
    st2, used2 = ctx.decode_blocks_lazy(K, T, ns, d_src.data_ptr(), K * T, h_lost, nl, h_resi, nu, av, d_rep.data_ptr(), rc * T)
    stats2 = ctx.stats()
    out2 = _host(ctx, torch, d_src)
    assert list(st2) == [st[b] for b in sel] and list(used2) == [used[b] for b in sel]
    for i, b in enumerate(sel):
        assert np.array_equal(out2[i], after[b]) and np.array_equal(after[b], blocks[b].src), b
    for f in STAT_FIELDS:
        assert stats[f] == stats2[f], (f, stats[f], stats2[f])
    # with a relay: the same verdicts and bytes, and the intermediate symbols of the decoded blocks are the oracle's
    r = receive(True)
    assert list(r[4]) == list(st) and list(r[5]) == list(used)
    for b, blk in enumerate(blocks):  # (an incomplete block's missing rows hold whatever the buffer held)
        rows_b = slice(None) if st[b] else blk.keep
        assert np.array_equal(r[7][b][rows_b], after[b][rows_b]), b
    for b in sel:
        want = orc.encode_block(blocks[b].src, K, T, (), want_inter=True)[1]
        assert np.array_equal(r[8][b], want), b


def test_reset_and_receive_again(ctx, torch, orc):
    K, T, nblk, sbn0 = 100, 36, 3, 7
    first = _lossy_blocks(orc, K, T, nblk, 0, seed=61)
    second = _lossy_blocks(orc, K, T, nblk, 0, seed=62)
    second[2] = Block(orc, K, T, 0, second[2].src, np.zeros(0, np.uint32), np.zeros(0, np.uint32))
    assert all(b.oracle_decodes() for b in first + second[:2])
    rng = np.random.default_rng(2)
    with nanorq_amd.Receiver(ctx, K, T, nblk, rep_cap=40, sbn0=sbn0) as rx, rx.relay() as relay:
        for blocks in (first, second):
            _feed(torch, rx, blocks, sbn0)
            assert rx.decode()[0].all()
            relay.encode()
            assert relay.ready().all()
            tags, expect = _tag_list(rng, blocks, sbn0)
            _emit_and_check(ctx, torch, relay, tags, expect, T, True, 0, sbn0=sbn0, nblk=nblk)
            rx.reset()
            assert not relay.ready().any()
            relay.encode()  # nothing is complete: nothing to make ready
            assert not relay.ready().any()
            held = [e if (int(t) >> 24) - sbn0 not in range(nblk) else None for t, e in zip(tags, expect)]
            _emit_and_check(ctx, torch, relay, tags, held, T, True, 0, sbn0=sbn0, nblk=nblk)


# ----------------------------------------------------------------------------------------- 7. refusals and lifetime ----
def test_refusals_and_lifetime(ctx, torch, orc):
    K, T, nblk, sbn0 = 100, 16, 3, 3
    blocks = _lossy_blocks(orc, K, T, nblk, 0, seed=71)
    tags = np.array([tag(sbn0 + b, e) for b in range(nblk) for e in (0, K - 1, K, K + 7)] + [tag(sbn0 + nblk, 0)], np.uint32)
    rx = nanorq_amd.Receiver(ctx, K, T, nblk, rep_cap=40, sbn0=sbn0)
    relay = rx.relay()
    with pytest.raises(NrqError, match="has a relay already"):
        rx.relay()
    # nothing is ready: a tag-list emit is not refused, every packet of the span gets -2
    _emit_and_check(ctx, torch, relay, tags, [None] * len(tags), T, False, 0, sbn0=sbn0, nblk=nblk)
    with pytest.raises(NrqError, match=r"not ready: SBN 3, 4, 5 \(3 of 3\)"):
        relay.emit_range(0, 4)
    _feed(torch, rx, blocks, sbn0, which=(0, 2))
    st, _ = rx.decode()
    assert list(st) == [1, 0, 1] and list(relay.ready()) == [True, False, True]
    with pytest.raises(NrqError, match=r"not ready: SBN 4 \(1 of 3\)"):
        relay.emit_range(0, 4)
    # the reception goes first: the relay is detached, its calls fail with a text, nothing dangles
    rx.close()
    for call in (relay.encode, relay.ready, lambda: relay.emit(_dev(torch, tags.view(np.int32))), lambda: relay.emit_range(0, 4)):
        with pytest.raises(NrqError, match="reception was destroyed"):
            call()
    relay.close()
    # a relay closed before its reception leaves the reception as it was, and free for another relay
    with nanorq_amd.Receiver(ctx, K, T, nblk, rep_cap=40, sbn0=sbn0) as rx:
        rx.relay().close()
        _feed(torch, rx, blocks, sbn0)
        assert rx.decode()[0].all()
        with rx.relay() as again:
            again.encode()
            assert again.ready().all()


def test_object_refusals_and_lifetime(ctx, torch):
    Kt, T, Z, N, Al, flags = OBJ_CASES[0]
    p = nanorq_amd.obj_params_enc(Kt * T - 37, T, 0, Z, N, Al, flags)
    rx = nanorq_amd.ObjectReceiver(ctx, p.oti_common, p.oti_specific, flags=flags, rep_cap=16)
    relay = rx.relay()
    with pytest.raises(NrqError, match="has a relay already"):
        rx.relay()
    tags = np.array([tag(b, 1) for b in range(Z + 1)], np.uint32)
    _emit_and_check(ctx, torch, relay, tags, [None] * len(tags), T, True, 0, sbn0=0, nblk=Z)
    with pytest.raises(NrqError, match=r"not ready: SBN 0, 1, 2, 3, 4 \(5 of 5\)"):
        relay.emit_all(2)
    rx.close()
    for call in (relay.encode, relay.ready, lambda: relay.emit_all(2), lambda: relay.emit(_dev(torch, tags.view(np.int32)))):
        with pytest.raises(NrqError, match="reception was destroyed"):
            call()
    assert relay.oti == (p.oti_common, p.oti_specific)
    relay.close()
