"""GPU tier of a reception set's want and held listings as runs (nrq_rxset_want_syms / nrq_rxset_held_syms, ReceiverSet.want_syms /
held_syms) and of NRQ_TX_HELD in nrq_txset_emit_syms (SenderSet.emit_syms(held=True)): the device against the CPU emulation over
twin books and against the members' own want_syms() / held_syms() concatenated in blocks() order (also after decode, reset, detach
and a member's close), the loop want_syms -> emit_syms -> add_syms -> decode with no per-member call, the held dump into a second
set, the held emit against the emulation at the wave edges in the five payload paths, the count-only, cap and refusal rules, and a
failing runtime call.  Every comparison is exact.  T = 16 unless a payload path needs another."""
import ctypes as C

import numpy as np
import pytest

import nanorq_amd
import runs_support as U
import rxset_runs_support as RR
import syms_set_support as SS
from nanorq_amd import NrqError
from rx_support import ADDED, EmuRx, ModelRx
from rxset_support import MIX4, UNTOUCHED, keyed_payloads, tag
from rxset_want_support import QUERIES
from test_gpu_rxset_want import BUILDERS, OBJ2, _add, _dev, _i32, _lossy_first_pass, _mix_table, _objects, _queries, _u32
from tx_support import FILL
from want_support import BIG, GUARD, WANT_SOURCE

pytestmark = pytest.mark.gpu
T = 16
HI = RR.HI


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available()
    return t


@pytest.fixture(scope="module")
def ctx(torch):
    import gpu_support as G
    return G.ctx()


@pytest.fixture(scope="module")
def tables(ctx, torch):
    """the twin tables of test_gpu_rxset_want.py, built on first use and shared (the listings only read the books)"""
    built = {}

    def get(name):
        if name not in built:
            built[name] = BUILDERS[name](ctx, torch)
        return built[name]
    yield get
    for t in built.values():
        t.close()


def _u8(t):
    return t.cpu().numpy()


def _args(q):
    return () if q is None else (WANT_SOURCE if q[0] else 0, q[1], q[2])


def _list(st, q, G, per_block=False):
    """ReceiverSet.want_syms(q) or, q None, held_syms -> numpy (keys, tags, nsym[, cnt])"""
    r = st.held_syms(G, per_block=per_block) if q is None else st.want_syms(G, extra=q[1], source=q[0], esi_from=q[2], per_block=per_block)
    return (_u32(r[0]), _u32(r[1]), _u8(r[2])) + tuple(r[3:])


# ------------------------------------------------------------------------------- the device against the emulation ----
GS_OF = {"cases": U.GS, "mix4": U.GS, "mix360": (5,), "caps": (16,)}


@pytest.mark.parametrize("name", list(BUILDERS))
def test_device_against_emulation(ctx, tables, name):
    """keys, first tags, counts, per-block packet counts and both totals, for want in both modes and for held; and the reference
    of the CPU tier once per table: the packetisation of the device's own one-symbol listing with each member's K"""
    tb = tables(name)
    bk, _ = tb.st.blocks()
    listed = 0
    queries = _queries(name) if name != "cases" else _queries(name)[::3]
    for G in GS_OF[name]:
        for q in list(queries) + [None]:
            keys, tags, ns, cnt = _list(tb.st, q, G, per_block=True)
            e = RR.emu_list_syms(tb.emu, "held" if q is None else "want", G, *_args(q))
            what = (name, G, q)
            assert e.rc == 0 and len(tags) == len(keys) == len(ns) == e.npkt == int(cnt.sum()), what
            assert np.array_equal(cnt, e.cnt) and len(cnt) == len(bk), what
            assert np.array_equal(tags, e.tags) and np.array_equal(ns, e.ns), what
            assert np.array_equal(keys, e.keys) and np.array_equal(keys, np.repeat(bk, cnt)), what
            assert int(ns.astype(np.int64).sum()) == e.nsym, what
            listed += e.npkt > 0
    assert listed >= 3
    G = GS_OF[name][-1]
    for q in (QUERIES[2], None):
        one = tb.st.held(per_block=True) if q is None else tb.st.want(extra=q[1], source=q[0], esi_from=q[2], per_block=True)
        ref = RR.reference(tb.emu, _u32(one[0]), _u32(one[1]), one[2], G)
        keys, tags, ns, cnt = _list(tb.st, q, G, per_block=True)
        RR.check_listing((keys, tags, ns, cnt, len(tags), int(ns.astype(np.int64).sum())), ref, _u32(one[1]), G)


# ---------------------------------------------------------------------------------------- against the members alone ----
def _members_alone(members, q, G):
    """(keys, tags, nsym) of the members' own want_syms / held_syms, members = [(key, rx)] in block order"""
    ks, ts, ns = [np.zeros(0, np.uint32)], [np.zeros(0, np.uint32)], [np.zeros(0, np.uint8)]
    for key, rx in members:
        t, n = rx.held_syms(G) if q is None else rx.want_syms(G, extra=q[1], source=q[0], esi_from=q[2])
        ts.append(_u32(t))
        ns.append(_u8(n))
        ks.append(np.full(int(t.numel()), key, np.uint32))
    return np.concatenate(ks), np.concatenate(ts), np.concatenate(ns)


def _check_identity(st, members, G, queries=QUERIES):
    """the set's lists are the members' own, one behind the other -> the number of packets seen"""
    members = sorted(members, key=lambda m: (m[0], getattr(m[1], "sbn0", 0)))
    total = 0
    for q in list(queries) + [None]:
        keys, tags, ns = _list(st, q, G)
        mk, mt, mn = _members_alone(members, q, G)
        assert np.array_equal(tags, mt) and np.array_equal(ns, mn) and np.array_equal(keys, mk), (G, q)
        total += len(mt)
    return total


@pytest.mark.parametrize("name", ["cases", "mix4"])
def test_against_the_members_alone(ctx, tables, name):
    tb = tables(name)
    for G in (5, 64):
        assert _check_identity(tb.st, tb.rxs, G, _queries(name)[:6]) > 0


def test_after_decode_reset_detach_and_close(ctx, torch):
    """two objects (one of two block classes) and two plain receptions under one key: the identity with the members' own lists
    after the first pass, after a top-up in packets and decode, after a member's reset, a detach and a member's close"""
    rng = np.random.default_rng(17)
    G = 5
    txs, _ = _objects(ctx, torch, OBJ2)
    rxs = [nanorq_amd.ObjectReceiver(ctx, *tx.oti, rep_cap=64) for tx in txs]
    extra_rx = [nanorq_amd.Receiver(ctx, 10, T, 3, 8, sbn0=s) for s in (0, 4)]
    sset, rset = nanorq_amd.SenderSet(ctx, T), nanorq_amd.ReceiverSet(ctx, T)
    try:
        for (key, _, _), tx, rx in zip(OBJ2, txs, rxs):
            sset.attach(key, tx)
            rset.attach(key, rx)
        rset.attach(99, extra_rx[1])
        rset.attach(99, extra_rx[0])
        members = [(k, rx) for (k, _, _), rx in zip(OBJ2, rxs)] + [(99, r) for r in extra_rx]
        _lossy_first_pass(torch, rng, OBJ2, txs, sset, rset, 0.1)
        pt = np.array([tag(s, e) for s in (0, 1, 2, 4, 5, 6) for e in (0, 1, 2, 4, 6, 8, 9, 12, 11)], np.uint32)
        pk = np.full(len(pt), 99, np.uint32)
        assert (_add(torch, ctx, rset, keyed_payloads(pk, pt, T), pt, pk) == ADDED).all()
        assert _check_identity(rset, members, G) > 0
        keys, tags, nsym = rset.want_syms(G, extra=2)                   # top up in packets, decode: recovered blocks drop out ...
        n = int(tags.numel())
        answer = torch.zeros((n, sset.stride_syms(G, True, True)), dtype=torch.uint8, device="cuda")  # (no sender under key 99)
        torch.cuda.synchronize()
        rset.add_syms(sset.emit_syms(keys, tags, G, nsym=nsym, out=answer, inline=True, key_inline=True), G, nsym=nsym, inline=True, key_inline=True)
        st, _ = rset.decode()
        nobj = sum(len(tx.blocks) for tx in txs)
        assert st[:2].all() and st[8:].all() and not st[2:8].any() and len(st) == nobj + 6
        _, _, _, cnt = rset.want_syms(G, extra=2, per_block=True)
        assert not cnt[:2].any() and not cnt[8:].any() and cnt[2:8].all()
        _, _, hn, hcnt = rset.held_syms(G, per_block=True)              # ... and list all K in held, in ceil(K / G) packets
        assert (hcnt[:2] >= 30).all() and (hcnt[8:] >= 9).all() and int(_u8(hn).astype(np.int64).sum()) == int(rset.held()[1].numel())
        _check_identity(rset, members, G)
        extra_rx[0].reset()
        assert list(rset.held_syms(G, per_block=True)[3][2:5]) == [0] * 3 and list(rset.want_syms(G, source=True, per_block=True)[3][2:5]) == [2] * 3
        _check_identity(rset, members, G)
        rset.detach(7)
        _check_identity(rset, [m for m in members if m[0] != 7], G)
        extra_rx[1].close()                                             # a member closed while attached drops out of the order
        left = [m for m in members if m[0] != 7 and m[1] is not extra_rx[1]]
        assert len(rset.blocks()[0]) == 3 + 5
        assert _check_identity(rset, left, G) > 0
    finally:
        for h in [sset, rset] + rxs + extra_rx + txs:
            h.close()


# --------------------------------------------------------------------------------- the loop with no per-member call ----
LOOP, LOOP_SEED, loop_losses = RR.LOOP, RR.LOOP_SEED, RR.loop_losses  # (the seed is pinned on the CPU tier: test_rxset_runs_emu.py)


@pytest.mark.parametrize("G", [5, 16])
def test_the_loop_closes_in_packets_with_no_per_member_call(ctx, torch, G):
    """senders of K = 10, 32, 100, 257 lose 10 - 25 % of their source symbols; ReceiverSet.want_syms -> ONE SenderSet.emit_syms with
    key and tag inline -> ONE ReceiverSet.add_syms of the buffer as emitted -> ReceiverSet.decode, until every block has status 1:
    within 3 rounds (the first asks for exactly the gaps; a block left undecoded although r >= g is asked again with
    extra = r - g + 1, as the header prescribes)"""
    g = torch.Generator().manual_seed(40 + G)
    txs, rxs, srcs = [], [], []
    sset, rset = nanorq_amd.SenderSet(ctx, T), nanorq_amd.ReceiverSet(ctx, T)
    try:
        for key, K, nblk, sbn0 in LOOP:
            srcs.append(torch.randint(0, 256, (nblk, K, T), dtype=torch.uint8, generator=g).cuda())
            torch.cuda.synchronize()
            txs.append(nanorq_amd.Sender(ctx, K, T, nblk, srcs[-1], sbn0=sbn0))
            txs[-1].encode()
            rxs.append(nanorq_amd.Receiver(ctx, K, T, nblk, rep_cap=K // 2 + 8, sbn0=sbn0))
            sset.attach(key, txs[-1])
            rset.attach(key, rxs[-1])
        lost = loop_losses(LOOP_SEED)
        ks = np.array([key for m, (key, K, nblk, s0) in enumerate(LOOP) for b in range(nblk) for e in range(K) if e not in lost[(m, b)]], np.uint32)
        ts = np.array([tag(s0 + b, e) for m, (key, K, nblk, s0) in enumerate(LOOP) for b in range(nblk) for e in range(K) if e not in lost[(m, b)]],
                      np.uint32)
        perm = np.random.default_rng(G).permutation(len(ts))
        k_d, t_d = _i32(torch, ks[perm]), _i32(torch, ts[perm])
        torch.cuda.synchronize()
        rset.add(sset.emit(k_d, t_d, inline=True, key_inline=True), inline=True, key_inline=True)
        gaps, _ = rset.counts()
        order = sorted(range(len(LOOP)), key=lambda m: (LOOP[m][0], LOOP[m][3]))
        assert list(gaps) == [len(lost[(m, b)]) for m in order for b in range(LOOP[m][2])] and (gaps > 0).sum() >= 10
        rounds, st = 0, np.zeros(len(gaps), np.int32)
        while not st.all():
            assert rounds < 3, (rounds, st)
            keys, tags, nsym, cnt = rset.want_syms(G, extra=rounds, per_block=True)
            n = int(tags.numel())
            assert n > 0 and not cnt[st != 0].any()
            if rounds == 0:  # exactly the gaps, in packets
                assert int(_u8(nsym).astype(np.int64).sum()) == int(gaps.sum()) and n < int(gaps.sum())
            res_tx = torch.full((n,), 77, dtype=torch.int32, device="cuda")
            res_rx = torch.full((n * G,), UNTOUCHED, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            answer = sset.emit_syms(keys, tags, G, nsym=nsym, inline=True, key_inline=True, results=res_tx)
            rset.add_syms(answer, G, nsym=nsym, inline=True, key_inline=True, results=res_rx)
            ctx.sync()
            assert (res_tx.cpu().numpy() == 0).all()
            live = (np.arange(G)[None, :] < _u8(nsym)[:, None]).reshape(-1)
            codes = res_rx.cpu().numpy()
            assert (codes[live] == ADDED).all()
            st, _ = rset.decode()
            rounds += 1
        print("rounds", rounds)
        assert rounds <= 3
        assert rset.want_syms(G, extra=2)[1].numel() == 0 and rset.want_syms(G, source=True)[1].numel() == 0
        for rx, src in zip(rxs, srcs):
            ctx.sync()
            assert bool((rx.source == src).all())
    finally:
        for h in [sset, rset] + rxs + txs:
            h.close()


# ------------------------------------------------------------------------------------------------------ the held dump ----
def _partial_stream(rng, spec):
    """(keys, tags) that leave every block of spec [(key, K, nblk, sbn0)] partial: about 60 % of its source ESIs and eight
    repair ESIs with runs in arrival order, shuffled per block"""
    ks, ts = [], []
    for key, K, nblk, sbn0 in spec:
        for b in range(nblk):
            src = np.flatnonzero(rng.random(K) < 0.6)
            src = src[src != K - 1]  # (at least one gap)
            rep = np.concatenate([np.arange(K + 2, K + 7), [K + 9, K + 8], [K]])  # (all within the smallest member's max_esi = 20)
            es = np.concatenate([rng.permutation(src), rep])
            ts.append(np.array([tag(sbn0 + b, int(e)) for e in es], np.uint32))
            ks.append(np.full(len(es), key, np.uint32))
    return np.concatenate(ks), np.concatenate(ts)


@pytest.mark.parametrize("G", [5, 16])
def test_the_held_dump_fills_a_second_set(ctx, torch, G):
    """partially filled receptions and a partially filled object with relays in a SenderSet: ReceiverSet.held_syms -> ONE
    SenderSet.emit_syms(held=True, key_inline=True) answers the list in full -> a second, empty ReceiverSet that add_syms the
    output ends with the first one's books and rows"""
    rng = np.random.default_rng(41 + G)
    spec = [(5, 10, 3, 0), (5, 26, 2, 3), (9, 100, 2, 0)]
    obj_spec = OBJ2[:1]
    otx, _ = _objects(ctx, torch, obj_spec)
    first = [(key, nanorq_amd.Receiver(ctx, K, T, nblk, 24, sbn0=sbn0)) for key, K, nblk, sbn0 in spec]
    second = [(key, nanorq_amd.Receiver(ctx, K, T, nblk, 24, sbn0=sbn0)) for key, K, nblk, sbn0 in spec]
    first.append((obj_spec[0][0], nanorq_amd.ObjectReceiver(ctx, *otx[0].oti, rep_cap=24)))
    second.append((obj_spec[0][0], nanorq_amd.ObjectReceiver(ctx, *otx[0].oti, rep_cap=24)))
    relays, relays2 = [], []
    rset, rset2 = nanorq_amd.ReceiverSet(ctx, T), nanorq_amd.ReceiverSet(ctx, T)
    sset, sset2, oset = nanorq_amd.SenderSet(ctx, T), nanorq_amd.SenderSet(ctx, T), nanorq_amd.SenderSet(ctx, T)
    try:
        for (key, rx), (_, rx2) in zip(first, second):
            rset.attach(key, rx)
            rset2.attach(key, rx2)
        oset.attach(obj_spec[0][0], otx[0])
        keys, tags = _partial_stream(rng, spec)
        assert (_add(torch, ctx, rset, keyed_payloads(keys, tags, T), tags, keys) == ADDED).all()
        _lossy_first_pass(torch, rng, obj_spec, otx, oset, rset, 0.3)
        for (key, rx), (_, rx2) in zip(first, second):
            relays.append(rx.relay())
            sset.attach(key, relays[-1])
            relays2.append(rx2.relay())
            sset2.attach(key, relays2[-1])
        gaps, nrep = rset.counts()
        assert (gaps > 0).all() and (nrep > 0).sum() >= 7
        keys, tags, nsym, cnt = rset.held_syms(G, per_block=True)
        n = int(tags.numel())
        total = int(_u8(nsym).astype(np.int64).sum())
        assert n > 30 and (cnt > 0).all() and total == int(rset.held()[1].numel()) and n < total
        res_tx = torch.full((n,), 77, dtype=torch.int32, device="cuda")
        res_rx = torch.full((n * G,), UNTOUCHED, dtype=torch.int32, device="cuda")
        stride = sset.stride_syms(G, True, True)
        dump = torch.full((n, stride), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        sset.emit_syms(keys, tags, G, nsym=nsym, out=dump, inline=True, key_inline=True, results=res_tx, held=True)
        rset2.add_syms(dump, G, nsym=nsym, inline=True, key_inline=True, results=res_rx)
        ctx.sync()
        assert (res_tx.cpu().numpy() == 0).all()                          # the list is answered in full
        live = (np.arange(G)[None, :] < _u8(nsym)[:, None]).reshape(-1)
        assert (res_rx.cpu().numpy()[live] == ADDED).all()
        for a, b in zip(rset.counts(), rset2.counts()):
            assert np.array_equal(a, b)
        for a, b in zip(rset.lists(), rset2.lists()):
            assert np.array_equal(a, b)
        for a, b in zip(rset.held(per_block=True), rset2.held(per_block=True)):
            assert np.array_equal(_u8(a) if hasattr(a, "cpu") else a, _u8(b) if hasattr(b, "cpu") else b)
        # the rows: the second set's relays give the same dump, byte for byte
        dump2 = torch.full((n, stride), FILL, dtype=torch.uint8, device="cuda")
        res2 = torch.full((n,), 77, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        sset2.emit_syms(keys, tags, G, nsym=nsym, out=dump2, inline=True, key_inline=True, results=res2, held=True)
        ctx.sync()
        assert (res2.cpu().numpy() == 0).all() and bool((dump == dump2).all())
        d = dump.cpu().numpy()
        c = _u8(nsym).astype(np.int64)
        assert all((d[k, 8 + c[k] * T:] == FILL).all() for k in range(0, n, 7))   # (the bytes behind hdr + c * T keep the fill)
    finally:
        for h in [sset, sset2, oset, rset, rset2] + relays + relays2 + [r for _, r in first + second] + otx:
            h.close()


# ------------------------------------------------------------------------- the held emit against the emulation ----
def _far_relay(ctx, torch, T_, G):
    """the relay in three states as test_gpu_runs._mixed_relay makes it (block 0 ready, block 1 complete but not ready, block 2
    partial), over RR.far_stream: block 2's runs lie beyond row 64 of its repair list at every G -> (sender, receiver, relay, its
    twin in the emulation, its model, the intermediate symbols as the device has them)"""
    K, nblk, sbn0 = U.K3, U.NB3, U.S3
    g = torch.Generator().manual_seed(T_ * 100 + G)
    src = torch.randint(0, 256, (nblk, K, T_), dtype=torch.uint8, generator=g).cuda()
    torch.cuda.synchronize()
    Kp = nanorq_amd.params(K)["Kp"]
    tx = nanorq_amd.Sender(ctx, K, T_, nblk, src, sbn0=sbn0)
    tx.encode()
    rx = nanorq_amd.Receiver(ctx, K, T_, nblk, rep_cap=RR.REP_CAP3, sbn0=sbn0, max_esi=U.MAXE3)
    emu = EmuRx(K, T_, nblk, RR.REP_CAP3, sbn0=sbn0, max_esi=U.MAXE3, Kp=Kp)
    mod = ModelRx(K, T_, nblk, RR.REP_CAP3, sbn0=sbn0, max_esi=U.MAXE3, Kp=Kp)
    stream = RR.far_stream(G)

    def add(b):
        tags = np.array([tag(sbn0 + b, e) for e in stream[b]], np.uint32)
        pk = tx.emit(_i32(torch, tags))
        res = torch.full((len(tags),), 77, dtype=torch.int32, device="cuda")
        ctx.sync()
        rx.add(pk, tags=_i32(torch, tags), results=res)
        ctx.sync()
        pk_h = pk.cpu().numpy()
        assert not res.cpu().numpy().any() and not emu.add(pk_h, tags=tags).any() and not mod.add(pk_h, tags).any()
    add(1)
    assert list(rx.decode()[0]) == [0, 1, 0]
    relay = rx.relay()
    add(0)
    assert list(rx.decode()[0]) == [1, 1, 0] and list(relay.ready()) == [True, False, False]
    add(2)
    ctx.sync()
    src_h = src.cpu().numpy()
    for b in (0, 1):  # what the decode did to the rows and the books
        emu.src[b, U.LOST3[b]] = src_h[b, U.LOST3[b]]
        emu.mark_complete(b)
        mod.mark_complete(b)
    b2 = emu.rep_esi[2 * emu.rep_cap:3 * emu.rep_cap].tolist()
    assert b2.index(U.K3 + 5) >= 64 and emu.nrep[2] <= emu.rep_cap
    Lr = nanorq_amd.params(Kp)["L"]
    inter = ctx.download(relay.inter_ptr, nblk * Lr * T_).reshape(nblk, Lr, T_)
    return tx, rx, relay, emu, mod, inter


@pytest.fixture(scope="module")
def mixed(ctx, torch):
    """the mixed member table of the CPU tier (rxset_runs_support.Mixed) on the device, per (T, G): the relay in three states, a
    plain sender of another K over the relay's first SBNs and an object's relay of two block classes, under three keys, and the
    table's twin in the emulation -- built on first use and shared (the emits only read)"""
    built = {}

    def get(T_, G):
        if (T_, G) not in built:
            p = nanorq_amd.params
            tx, rx, relay, emu, mod, inter = _far_relay(ctx, torch, T_, G)
            g = torch.Generator().manual_seed(T_ * 100 + G + 1)
            src_s = torch.randint(0, 256, (RR.NBS, RR.KS, T_), dtype=torch.uint8, generator=g).cuda()
            torch.cuda.synchronize()
            tx_s = nanorq_amd.Sender(ctx, RR.KS, T_, RR.NBS, src_s, sbn0=RR.SBNS)
            tx_s.encode()
            ctx.sync()
            Ls = p(p(RR.KS)["Kp"])["L"]
            inter_s = ctx.download(tx_s.inter_ptr, RR.NBS * Ls * T_).reshape(RR.NBS, Ls, T_)
            m = RR.Mixed(T_, G, relay=(emu, mod, inter), sender=(src_s.cpu().numpy(), inter_s))
            # the object: its OTI alone (nothing of it is ever decoded), the rows its twins in the emulation were given
            op = nanorq_amd.obj_params_enc((RR.ZL * RR.KOL + RR.ZS * RR.KOS) * T_, T_, Z=RR.ZL + RR.ZS, Al=8 if T_ % 8 == 0 else 1)
            orx = nanorq_amd.ObjectReceiver(ctx, op.oti_common, op.oti_specific, rep_cap=m.obj[0][0].rep_cap)
            assert [k for k, _ in orx.blocks] == [RR.KOL] * RR.ZL + [RR.KOS] * RR.ZS and orx.params.max_esi == m.obj[0][0].max_esi
            for tg, pay in m.obj_streams:
                assert (_add(torch, ctx, orx, pay, tg) == ADDED).all()
            orelay = orx.relay()
            sset = nanorq_amd.SenderSet(ctx, T_)
            for key, h in ((RR.KEY_O, orelay), (RR.KEY_S, tx_s), (RR.KEY_R, relay)):
                sset.attach(key, h)
            Lr, Lo = p(p(U.K3)["Kp"])["L"], p(p(RR.KOL)["Kp"])["L"]
            rows = [(rx.src_ptr, U.K3 * T_), (relay.inter_ptr, Lr * T_), (rx.rep_ptr, RR.REP_CAP3 * T_), (src_s.data_ptr(), RR.KS * T_),
                    (tx_s.inter_ptr, Ls * T_),   # (the object's rows are the library's own allocations: their steps alone)
                    (0, RR.KOL * T_), (0, RR.KOS * T_), (0, Lo * T_), (0, m.obj[0][0].rep_cap * T_)]
            built[(T_, G)] = (m, sset, rows, (sset, orelay, orx, tx_s, relay, rx, tx))
        return built[(T_, G)][:3]
    yield get
    for _, _, _, hs in built.values():
        for h in hs:
            h.close()


@pytest.mark.parametrize("G", [1, 5, 64])
@pytest.mark.parametrize("T_,hdr,kind,path", RR.PATH_ROWS, ids=[r[3] for r in RR.PATH_ROWS])
def test_held_emit_against_emulation_at_the_wave_edges(ctx, torch, mixed, T_, hdr, kind, path, G):
    """the mixed member table of the CPU tier, its packets interleaved so that one wave holds packets of segments of different K:
    n below one wave's packets, exactly one wave, and the whole list (later waves), in each payload path.  Results and bytes
    equal the emulation's over the twin table, the result table of the header member by member, and the one-symbol held set
    emit's packets laid out as runs; the plain sender's packets are what they are without the flag"""
    m, sset, rows = mixed(T_, G)
    keys, tags, counts = m.packets()
    per = 64 // G
    stride = RR.stride_of(T_, G, hdr, kind)
    assert len(tags) > per
    for n in sorted({max(1, per - 1), per, len(tags)}):
        k, t, c = keys[:n], tags[:n], counts[:n]
        buf = torch.full((n + 2, stride), FILL, dtype=torch.uint8, device="cuda")
        out = buf[1:-1]
        res = torch.full((n,), 77, dtype=torch.int32, device="cuda")
        assert SS.emit_path(out.data_ptr(), stride, T_, hdr, rows) == path
        k_d, t_d, c_d = _i32(torch, k), _i32(torch, t), _dev(torch, c)
        torch.cuda.synchronize()
        sset.emit_syms(k_d, t_d, G, nsym=c_d, out=out, inline=hdr > 0, key_inline=hdr == 8, results=res, held=True)
        ctx.sync()
        pk_d, res_d = out.cpu().numpy(), res.cpu().numpy()
        assert bool((buf[0] == FILL).all()) and bool((buf[-1] == FILL).all()), "guard rows"
        pk_e, res_e, _ = RR.emu_txset_emit_held_syms(m.segs, k, t, c, G, hdr, stride)
        assert np.array_equal(res_d, res_e), (n, np.flatnonzero(res_d != res_e)[:8])
        bad = np.flatnonzero((pk_d != pk_e).any(1))
        assert len(bad) == 0, (n, bad[:8], k[bad[:8]], t[bad[:8]])
        want_res = m.results(k, t, c)
        assert np.array_equal(res_d, want_res), (n, np.flatnonzero(res_d != want_res)[:8])
        want = m.expected(k, t, c, res_d, hdr, stride)
        bad = np.flatnonzero((pk_d != want).any(1))
        assert len(bad) == 0, (n, bad[:8], k[bad[:8]], t[bad[:8]])
        if n == len(tags):
            for key in (RR.KEY_R, RR.KEY_O):
                assert set(res_d[k == key].tolist()) == {0, RR.FOREIGN, RR.NOT_READY, RR.BAD_RANGE}, key
            obj_ok = (k == RR.KEY_O) & (res_d == 0)                              # both of the object's segments answer,
            assert (obj_ok & ((t >> 24) < RR.ZL)).any() and (obj_ok & ((t >> 24) >= RR.ZL)).any()
            assert (obj_ok & ((t & HI) >= RR.KOL)).any()                         # from repair rows too
            assert (res_d[k == RR.KEY_NONE] == RR.FOREIGN).all()
            # without the flag: the sender's packets and those of the relay's ready block are the same bytes
            out0 = torch.full((n, stride), FILL, dtype=torch.uint8, device="cuda")
            res0 = torch.full((n,), 77, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            sset.emit_syms(k_d, t_d, G, nsym=c_d, out=out0, inline=hdr > 0, key_inline=hdr == 8, results=res0)
            ctx.sync()
            same = (k == RR.KEY_S) | (k == RR.KEY_NONE) | ((k == RR.KEY_R) & ((t >> 24) == U.S3) & (res_d != RR.BAD_RANGE))
            assert np.array_equal(res0.cpu().numpy()[same], res_d[same]) and np.array_equal(out0.cpu().numpy()[same], pk_d[same])
            assert (res_d[k == RR.KEY_S] == 0).sum() >= 3 and RR.NOT_READY not in res_d[k == RR.KEY_S]


# ---------------------------------------------------------------------------------------------------------------- rules ----
def test_count_only_and_a_cap_one_short(ctx, torch, tables):
    tb = tables("mix4")
    L, st, G = ctx._L, tb.st, 5
    u32p = C.POINTER(C.c_uint32)
    for fn, args in ((L.nrq_rxset_want_syms, (0, 2, 0, G)), (L.nrq_rxset_held_syms, (G,))):
        npkt, nsym, nb = C.c_uint32(0), C.c_uint32(0), len(st.blocks()[0])
        cnt = np.full(nb + 2, GUARD, np.uint32)
        assert fn(st._h, *args, None, None, None, 0, cnt.ctypes.data_as(u32p), C.byref(npkt), C.byref(nsym)) == 0
        one = st.want(extra=2)[1].numel() if len(args) > 1 else st.held()[1].numel()
        assert npkt.value > 8 and int(cnt[:nb].sum()) == npkt.value and (cnt[nb:] == GUARD).all() and nsym.value == one > npkt.value
        n2 = C.c_uint32(0)
        assert fn(st._h, *args, None, None, None, 0, None, C.byref(n2), None) == 0 and n2.value == npkt.value   # (h_cnt, h_nsym NULL)
        n = npkt.value
        keys = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        tags = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        ns = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        K_, T_, N_ = C.c_void_p(keys.data_ptr()), C.c_void_p(tags.data_ptr()), C.c_void_p(ns.data_ptr())
        cnt2, n3, s3 = np.zeros(nb, np.uint32), C.c_uint32(0), C.c_uint32(0)
        with pytest.raises(NrqError, match="d_tags and d_nsym have room for %d" % (n - 1)):
            ctx._chk(fn(st._h, *args, K_, T_, N_, n - 1, cnt2.ctypes.data_as(u32p), C.byref(n3), C.byref(s3)))
        ctx.sync()
        assert (n3.value, s3.value) == (n, nsym.value) and np.array_equal(cnt2, cnt[:nb])   # totals and counts filled, nothing written
        assert (keys.cpu().numpy() == 0x5A5A5A5A).all() and (tags.cpu().numpy() == 0x5A5A5A5A).all() and (ns.cpu().numpy() == 0x5A).all()
        assert fn(st._h, *args, None, T_, N_, n, None, C.byref(n3), None) == 0                  # d_keys NULL, cap exact
        ctx.sync()
        ref = st.want_syms(G, extra=2) if len(args) > 1 else st.held_syms(G)
        assert np.array_equal(tags.cpu().numpy(), ref[1].cpu().numpy()) and np.array_equal(ns.cpu().numpy(), ref[2].cpu().numpy())
        assert (keys.cpu().numpy() == 0x5A5A5A5A).all()


def test_refusals_enqueue_nothing(ctx, torch):
    L = ctx._L
    err = lambda: L.nrq_ctx_error(ctx._h) or b""
    rxs = [nanorq_amd.Receiver(ctx, 10, T, 2, 4, sbn0=s) for s in (0, 2)]
    st, empty = nanorq_amd.ReceiverSet(ctx, T), nanorq_amd.ReceiverSet(ctx, T)
    try:
        st.attach(1, rxs[0])
        st.attach(2, rxs[1])
        npkt, nsym = C.c_uint32(7), C.c_uint32(7)
        buf = torch.full((64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        p = C.c_void_p(buf.data_ptr())
        N, S = C.byref(npkt), C.byref(nsym)
        want = lambda *a: L.nrq_rxset_want_syms(st._h, *a)
        heldf = lambda *a: L.nrq_rxset_held_syms(st._h, *a)
        for flags in (2, 3, 0x80000000):
            npkt.value = nsym.value = 7
            assert want(flags, 0, 0, 5, None, None, None, 0, None, N, S) == -1 and (npkt.value, nsym.value) == (0, 0)
            assert b"nrq_rxset_want_syms: unknown flags" in err()
        with pytest.raises(NrqError, match="nrq_rxset_want_syms: NRQ_WANT_SOURCE takes neither"):
            st.want_syms(5, source=True, extra=1)
        with pytest.raises(NrqError, match="nrq_rxset_want_syms: extra .* is above 2\\^24"):
            st.want_syms(5, extra=BIG + 1)
        for G in (0, 65):
            assert want(0, 0, 0, G, None, None, None, 0, None, N, S) == -1 and b"nrq_rxset_want_syms: G=%d outside 1..64" % G in err()
            assert heldf(G, None, None, None, 0, None, N, S) == -1 and b"nrq_rxset_held_syms: G=%d outside 1..64" % G in err()
        for tg, ns in ((p, None), (None, p)):                                        # exactly one of d_tags / d_nsym
            assert want(1, 0, 0, 5, None, tg, ns, 64, None, N, S) == -1 and b"nrq_rxset_want_syms: d_tags and d_nsym go together" in err()
            assert heldf(5, p, tg, ns, 64, None, N, S) == -1 and b"nrq_rxset_held_syms: d_tags and d_nsym go together" in err()
        assert want(1, 0, 0, 5, p, None, None, 64, None, N, S) == -1 and b"nrq_rxset_want_syms: d_keys without d_tags" in err()
        assert heldf(5, p, None, None, 64, None, N, S) == -1 and b"nrq_rxset_held_syms: d_keys without d_tags" in err()
        assert want(1, 0, 0, 5, None, None, None, 0, None, None, S) == -1 and b"h_npkt is NULL" in err()
        assert heldf(5, None, None, None, 0, None, None, S) == -1 and b"h_npkt is NULL" in err()
        assert L.nrq_rxset_want_syms(None, 0, 0, 0, 5, None, None, None, 0, None, N, S) == -1
        assert L.nrq_rxset_held_syms(None, 5, None, None, None, 0, None, N, S) == -1
        npkt.value = nsym.value = 7
        assert L.nrq_rxset_want_syms(empty._h, 0, 2, 0, 5, p, p, p, 0, None, N, S) == 0 and (npkt.value, nsym.value) == (0, 0)  # an empty set
        for r in (empty.want_syms(5, per_block=True), empty.held_syms(5, per_block=True)):
            assert r[0].numel() == r[1].numel() == r[2].numel() == 0 and len(r[3]) == 0
        ctx.sync()
        assert (buf.cpu().numpy() == 0x5A5A5A5A).all()                              # nothing was enqueued
        keys, tags, ns = st.want_syms(4, source=True)
        assert _u32(keys).tolist() == [1] * 6 + [2] * 6
        assert _u32(tags).tolist() == [tag(s, e) for s in range(4) for e in (0, 4, 8)] and _u8(ns).tolist() == [4, 4, 2] * 4
        assert st.held_syms(4)[1].numel() == 0 and st.want_syms(1, source=True)[1].numel() == 40
    finally:
        for h in [st, empty] + rxs:
            h.close()


def test_the_held_flag_needs_a_relay_member(ctx, torch):
    """a set of plain senders still refuses NRQ_TX_HELD (results and packets untouched); with one relay attached it is accepted and
    the senders answer as without it"""
    K, nblk, G = 10, 2, 4
    g = torch.Generator().manual_seed(7)
    src = torch.randint(0, 256, (nblk, K, T), dtype=torch.uint8, generator=g).cuda()
    torch.cuda.synchronize()
    tx = nanorq_amd.Sender(ctx, K, T, nblk, src)
    tx.encode()
    rx = nanorq_amd.Receiver(ctx, K, T, nblk, 4, sbn0=0)
    sset = nanorq_amd.SenderSet(ctx, T)
    relay = None
    try:
        sset.attach(3, tx)
        tags = np.array([tag(0, 0), tag(1, 4), tag(0, K + 1), tag(1, 8)], np.uint32)
        nsym = np.array([4, 4, 4, 2], np.uint8)
        k3, k8 = _i32(torch, np.full(4, 3, np.uint32)), _i32(torch, np.array([8, 8, 3, 3], np.uint32))
        t_d, n_d = _i32(torch, tags), _dev(torch, nsym)
        out = torch.full((4, G * T + 8), FILL, dtype=torch.uint8, device="cuda")
        plain = torch.full((4, G * T + 8), FILL, dtype=torch.uint8, device="cuda")
        res = torch.full((4,), 77, dtype=torch.int32, device="cuda")
        pt = np.array([tag(0, e) for e in (0, 1, 2, 3, 7, K + 4, K + 5)], np.uint32)  # the reception: block 0 partial, block 1 untouched
        p_d = _i32(torch, pt)
        torch.cuda.synchronize()
        with pytest.raises(NrqError, match="nrq_txset_emit_syms: NRQ_TX_HELD"):
            sset.emit_syms(k3, t_d, G, nsym=n_d, out=out, inline=True, key_inline=True, results=res, held=True)
        ctx.sync()
        assert bool((out == FILL).all()) and (res.cpu().numpy() == 77).all()
        sset.emit_syms(k3, t_d, G, nsym=n_d, out=plain, inline=True, key_inline=True)
        rx.add(tx.emit(p_d), tags=p_d)
        relay = rx.relay()
        sset.attach(8, relay)
        sset.emit_syms(k3, t_d, G, nsym=n_d, out=out, inline=True, key_inline=True, results=res, held=True)
        ctx.sync()
        assert (res.cpu().numpy() == 0).all() and bool((out == plain).all())         # the sender's packets, as without the flag
        out.fill_(FILL)
        torch.cuda.synchronize()
        sset.emit_syms(k8, t_d, G, nsym=n_d, out=out, inline=True, key_inline=True, results=res, held=True)
        ctx.sync()
        assert res.cpu().numpy().tolist() == [0, RR.NOT_READY, 0, 0]                 # held 0..3; block 1 holds nothing
        o, p0 = out.cpu().numpy(), plain.cpu().numpy()
        assert np.array_equal(o[0, 4:], p0[0, 4:]) and o[0, :4].tolist() == [0, 0, 0, 8] and (o[1] == FILL).all()
        assert np.array_equal(o[2:, 4:], p0[2:, 4:])
        res.fill_(77)
        torch.cuda.synchronize()
        sset.emit_syms(k8, t_d, G, nsym=n_d, out=out, inline=True, key_inline=True, results=res)   # without the flag: not ready
        ctx.sync()
        assert res.cpu().numpy().tolist() == [RR.NOT_READY, RR.NOT_READY, 0, 0]
    finally:
        for h in [sset, relay, rx, tx]:
            if h is not None:
                h.close()


# ---------------------------------------------------------------------------------------------- a failing runtime call ----
def test_a_failing_runtime_call(torch):
    """fail_after on a context of its own: the n-th checked runtime call of ReceiverSet.want_syms -- the count call of
    nrq_rxset_want_syms, then its fill call -- fails, for n = 1, 2, ... up to the first n at which both succeed.  The call returns
    the error, the members' books are unchanged, and the same call afterwards gives the full list."""
    import gpu_support as G_
    G_.ctx()  # (torch first, as every context of this process)
    fctx = nanorq_amd.Context(0)
    tb = None
    G = 5
    try:
        tb = _mix_table(fctx, torch, MIX4, 1500, 35)
        ref = tb.st.want_syms(G, extra=2, per_block=True)
        ref = (_u32(ref[0]), _u32(ref[1]), _u8(ref[2]), ref[3])
        books = tb.st.lists()
        assert len(ref[1]) > 8
        failed = 0
        for n_fail in range(1, 33):
            fctx.set_option("fail_after", n_fail)
            try:
                got = tb.st.want_syms(G, extra=2, per_block=True)
                err = None
            except NrqError as e:
                err = str(e)
            fctx.set_option("fail_after", 0)
            fctx.sync()
            if err is None:
                break  # (the two calls make fewer than n_fail checked runtime calls)
            failed += 1
            assert "failed" in err, err
            now = tb.st.lists()
            assert all(np.array_equal(a, b) for a, b in zip(now, books)), (n_fail, err)
            k, t, s, c = tb.st.want_syms(G, extra=2, per_block=True)
            assert np.array_equal(_u32(k), ref[0]) and np.array_equal(_u32(t), ref[1]) and np.array_equal(_u8(s), ref[2]), (n_fail, err)
            assert np.array_equal(c, ref[3])
        print("failed calls", failed)
        assert failed >= 10 and err is None   # (hipSetDevice, the memset, two error checks, the download and the wait of each call at least)
        assert np.array_equal(_u32(got[1]), ref[1])
    finally:
        if tb:
            tb.close()
        fctx.close()


def test_a_failing_runtime_call_in_the_held_emit(torch):
    """the same on SenderSet.emit_syms(held=True): the n-th checked runtime call of nrq_txset_emit_syms under NRQ_TX_HELD -- those
    of the call's set-up, then the held kernel's launch -- fails, up to the first n at which all succeed.  The call returns the
    error, and the same call afterwards answers the whole held list with the bytes of the call before the failures."""
    import gpu_support as G_
    G_.ctx()  # (torch first, as every context of this process)
    fctx = nanorq_amd.Context(0)
    K, nblk, G = 26, 2, 5
    tx = rx = relay = rset = sset = None
    try:
        g = torch.Generator().manual_seed(3)
        src = torch.randint(0, 256, (nblk, K, T), dtype=torch.uint8, generator=g).cuda()
        torch.cuda.synchronize()
        tx = nanorq_amd.Sender(fctx, K, T, nblk, src)
        tx.encode()
        rx = nanorq_amd.Receiver(fctx, K, T, nblk, 16)
        pt = np.array([tag(b, e) for b in range(nblk) for e in list(range(0, K - 4)) + [K + 2, K + 3, K + 4, K + 9]], np.uint32)
        p_d = _i32(torch, pt)
        torch.cuda.synchronize()
        rx.add(tx.emit(p_d), tags=p_d)
        relay = rx.relay()
        rset, sset = nanorq_amd.ReceiverSet(fctx, T), nanorq_amd.SenderSet(fctx, T)
        rset.attach(6, rx)
        sset.attach(6, relay)
        keys, tags, nsym = rset.held_syms(G)
        n = int(tags.numel())
        assert n >= 2 * (K // G) and int(_u8(nsym).astype(np.int64).sum()) == len(pt)
        stride = sset.stride_syms(G, True, True)

        def emit():
            out = torch.full((n, stride), FILL, dtype=torch.uint8, device="cuda")
            res = torch.full((n,), 77, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            sset.emit_syms(keys, tags, G, nsym=nsym, out=out, inline=True, key_inline=True, results=res, held=True)
            fctx.sync()
            return out.cpu().numpy(), res.cpu().numpy()
        ref, ref_res = emit()
        assert (ref_res == 0).all()
        failed, err = 0, "none yet"
        for n_fail in range(1, 33):
            fctx.set_option("fail_after", n_fail)
            try:
                emit()
                err = None
            except NrqError as e:
                err = str(e)
            fctx.set_option("fail_after", 0)
            fctx.sync()
            if err is None:
                break  # (the call makes fewer than n_fail checked runtime calls)
            failed += 1
            assert "failed" in err, err
            got, got_res = emit()
            assert np.array_equal(got_res, ref_res) and np.array_equal(got, ref), (n_fail, err)
        print("failed calls", failed)
        assert failed >= 2 and err is None
    finally:
        for h in (sset, rset, relay, rx, tx):
            if h is not None:
                h.close()
        fctx.close()
