"""GPU tier of a reception set's want and held listings with keys (nrq_rxset_want / nrq_rxset_held, ReceiverSet.want / held): the
device against the CPU emulation over twin books, against the members' own want() / held() concatenated in blocks() order (also
after decode, reset, detach and a member's close), the count-only and cap rules, the loop want -> emit -> add -> decode with no
per-member call, the held dump into a second set, the argument and lifetime rules, and a failing runtime call.  T = 16
throughout; the books are built by ReceiverSet.add."""
import ctypes as C

import numpy as np
import pytest

import nanorq_amd
from nanorq_amd import NrqError
from rx_support import ADDED, EmuRx
from rxset_support import MIX4, MIX360, UNTOUCHED, EmuSet, keyed_payloads, keyed_stream, rep_cap_of, tag
from rxset_want_support import QUERIES, emu_list
from util import payload
from want_support import BIG, CASE_NAMES, GUARD, NBLK, SBN0, WANT_SOURCE, case as case_of

pytestmark = pytest.mark.gpu
T = 16
CAPS = [(m // 4, 10, 16, 16 * (m % 4)) for m in range(64)]  # both caps: 64 members, 1024 blocks


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


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _add(torch, ctx, h, pl, tags, keys=None):
    """one add of host-built packets (payload rows, tags, and keys for a set) -> the result codes"""
    res = torch.full((len(tags),), UNTOUCHED, dtype=torch.int32, device="cuda")
    p_d, t_d = _dev(torch, pl), _i32(torch, tags)
    kw = {} if keys is None else dict(keys=_i32(torch, keys))
    torch.cuda.synchronize()
    h.add(p_d, tags=t_d, results=res, **kw)
    ctx.sync()
    return res.cpu().numpy()


class _Table:
    """A ReceiverSet over Receivers and, beside it, EmuRx twins with the same books: both ingest the same keyed packets."""

    def __init__(self, ctx, torch, spec, streams):
        """spec: [(key, K, nblk, sbn0, rep_cap, max_esi, Kp)], attached in reverse; streams: [(keys, tags)], one add each"""
        self.st, self.rxs, self.emu = nanorq_amd.ReceiverSet(ctx, T), [], []
        eset = EmuSet()
        for key, K, nblk, sbn0, rep_cap, max_esi, Kp in reversed(spec):
            self.rxs.append((key, nanorq_amd.Receiver(ctx, K, T, nblk, rep_cap, sbn0=sbn0, max_esi=max_esi)))
            self.st.attach(*self.rxs[-1])
            self.emu.append((key, EmuRx(K, T, nblk, rep_cap, sbn0, max_esi=max_esi, Kp=Kp), 0))
            eset.attach(key, self.emu[-1][1])
        for keys, tags in streams:
            pl = keyed_payloads(keys, tags, T)
            got = _add(torch, ctx, self.st, pl, tags, keys)
            assert np.array_equal(got, eset.add(pl, keys, tags))   # (the twins' books are the device's)

    def in_order(self):
        return [rx for _, rx in sorted(self.rxs, key=lambda m: (m[0], m[1].sbn0))]

    def close(self):
        self.st.close()
        for _, r in self.rxs:
            r.close()


def _mix_table(ctx, torch, mix, n, seed, small_cap=False):
    kps = [nanorq_amd.params(m[1])["Kp"] for m in mix]
    spec = [(key, K, nblk, sbn0, rep_cap_of(K, small_cap), 0, Kp) for (key, K, nblk, sbn0), Kp in zip(mix, kps)]
    return _Table(ctx, torch, spec, [keyed_stream(np.random.default_rng(seed), mix, kps, n)])


def _case_table(ctx, torch):
    """the receptions of want_support.CASE_NAMES as members of one set under distinct keys: K, max_esi and rep_cap all differ"""
    cases = [case_of(name) for name in CASE_NAMES]
    spec = [(1000 - 7 * i, c.K, NBLK, SBN0, c.rep_cap, c.max_esi, c.Kp) for i, c in enumerate(cases)]
    halves = [[np.array_split(c.stream, 2)[h] for c in cases] for h in (0, 1)]
    streams = [(np.concatenate([np.full(len(p), s[0], np.uint32) for s, p in zip(spec, half)]), np.concatenate(half)) for half in halves]
    return _Table(ctx, torch, spec, streams)


BUILDERS = {"cases": _case_table, "mix4": lambda c, t: _mix_table(c, t, MIX4, 1500, 32), "mix360": lambda c, t: _mix_table(c, t, MIX360, 5000, 33),
            "caps": lambda c, t: _mix_table(c, t, CAPS, 24000, 34)}


@pytest.fixture(scope="module")
def tables(ctx, torch):
    """the tables both comparisons list, built on first use and shared (the listings only read the books)"""
    built = {}

    def get(name):
        if name not in built:
            built[name] = BUILDERS[name](ctx, torch)
        return built[name]
    yield get
    for t in built.values():
        t.close()


def _queries(name):
    return sorted({q for n in CASE_NAMES for q in case_of(n).queries}) if name == "cases" else QUERIES


# ------------------------------------------------------------------------------- the device against the emulation ----
@pytest.mark.parametrize("name", list(BUILDERS))
def test_device_against_emulation(ctx, tables, name):
    """tags, keys, per-block counts and total, for want in both modes and for held.  `cases`: one-word bitmaps, K = 31 / 32 / 33,
    max_esi = K', 257 seen words, thousands of repair ESIs; `mix360`: a scan over 361 entries; `caps`: 1024 blocks, 1025 entries"""
    tb = tables(name)
    bk, _ = tb.st.blocks()
    listed = 0
    for source, extra, esi_from in _queries(name):
        keys, tags, cnt = tb.st.want(extra=extra, source=source, esi_from=esi_from, per_block=True)
        rc, n, e_cnt, e_keys, e_tags = emu_list(tb.emu, "want", WANT_SOURCE if source else 0, extra, esi_from)
        what = (name, source, extra, esi_from)
        assert rc == 0 and int(tags.numel()) == int(keys.numel()) == n == int(cnt.sum()), what
        assert np.array_equal(cnt, e_cnt) and len(cnt) == len(bk), what
        assert np.array_equal(_u32(tags), e_tags), what
        assert np.array_equal(_u32(keys), e_keys) and np.array_equal(e_keys, np.repeat(bk, cnt)), what
        listed += n > 0
    assert listed >= 3
    keys, tags, cnt = tb.st.held(per_block=True)
    rc, n, e_cnt, e_keys, e_tags = emu_list(tb.emu, "held")
    assert rc == 0 and n == int(tags.numel()) > 0 and np.array_equal(cnt, e_cnt)
    assert np.array_equal(_u32(tags), e_tags) and np.array_equal(_u32(keys), e_keys)


# ---------------------------------------------------------------------------------------- against the members alone ----
def _members_alone(members, want_args=None):
    """(keys, tags, counts per member) of the members' own want(**want_args) / held(), members = [(key, rx)] in block order"""
    ks, ts = [np.zeros(0, np.uint32)], [np.zeros(0, np.uint32)]
    for key, rx in members:
        t = _u32(rx.held() if want_args is None else rx.want(**want_args))
        ts.append(t)
        ks.append(np.full(len(t), key, np.uint32))
    return np.concatenate(ks), np.concatenate(ts)


def _check_identity(st, members, queries=QUERIES):
    """the set's lists are the members' own, one behind the other -> the number of tags seen"""
    members = sorted(members, key=lambda m: (m[0], getattr(m[1], "sbn0", 0)))
    total = 0
    for source, extra, esi_from in queries:
        keys, tags = st.want(extra=extra, source=source, esi_from=esi_from)
        mk, mt = _members_alone(members, dict(extra=extra, source=source, esi_from=esi_from))
        assert np.array_equal(_u32(tags), mt) and np.array_equal(_u32(keys), mk), (source, extra, esi_from)
        total += len(mt)
    keys, tags = st.held()
    mk, mt = _members_alone(members)
    assert np.array_equal(_u32(tags), mt) and np.array_equal(_u32(keys), mk)
    return total + len(mt)


@pytest.mark.parametrize("name", list(BUILDERS))
def test_against_the_members_alone(ctx, tables, name):
    tb = tables(name)
    q = _queries(name)
    assert _check_identity(tb.st, tb.rxs, q if name != "caps" else q[:2]) > 0


def _objects(ctx, torch, specs, seed=0):
    """ObjectSenders (encoded) of (key, F, Z) and their data"""
    txs, datas = [], []
    for key, F, Z in specs:
        datas.append(payload(F, seed=F + seed))
        d = _dev(torch, datas[-1])
        torch.cuda.synchronize()
        txs.append(nanorq_amd.ObjectSender(ctx, d, T, Z=Z))
        txs[-1].encode()
    return txs, datas


def _lossy_first_pass(torch, rng, specs, txs, sset, rset, loss):
    """every source packet of every object but a share `loss`, shuffled, in ONE emit and ONE add"""
    ks = np.concatenate([np.full(sum(K for K, _ in tx.blocks), key, np.uint32) for (key, _, _), tx in zip(specs, txs)])
    ts = np.concatenate([[tag(sbn, e) for sbn, (K, _) in enumerate(tx.blocks) for e in range(K)] for tx in txs]).astype(np.uint32)
    keep = rng.permutation(np.flatnonzero(rng.random(len(ts)) >= loss))
    k_d, t_d = _i32(torch, ks[keep]), _i32(torch, ts[keep])
    torch.cuda.synchronize()
    rset.add(sset.emit(k_d, t_d, inline=True, key_inline=True), inline=True, key_inline=True)


OBJ2 = [(0x1001, 213 * T - 5, 5), (7, 300 * T, 2)]  # two block classes (3 blocks of K = 43, 2 of 42); one class, K = 150


def test_an_object_of_two_classes_against_its_own_lists(ctx, torch):
    rng = np.random.default_rng(5)
    specs = OBJ2[:1]
    txs, _ = _objects(ctx, torch, specs)
    orx = nanorq_amd.ObjectReceiver(ctx, *txs[0].oti, rep_cap=64)
    plain = nanorq_amd.Receiver(ctx, 10, T, 2, 8, sbn0=1)
    sset, rset = nanorq_amd.SenderSet(ctx, T), nanorq_amd.ReceiverSet(ctx, T)
    try:
        assert len({K for K, _ in txs[0].blocks}) == 2
        sset.attach(specs[0][0], txs[0])
        rset.attach(specs[0][0], orx)
        rset.attach(3, plain)
        _lossy_first_pass(torch, rng, specs, txs, sset, rset, 0.2)
        _, _, cnt = rset.want(source=True, per_block=True)
        assert len(cnt) == 7 and list(cnt[:2]) == [10, 10] and cnt[2:5].any() and cnt[5:].any()   # ZL >= 1 and ZS >= 1 blocks ask
        assert _check_identity(rset, [(3, plain), (specs[0][0], orx)]) > 0
    finally:
        for h in (sset, rset, orx, plain, txs[0]):
            h.close()


# ------------------------------------------------------------------------------------------------ after state changes ----
def test_after_decode_reset_detach_and_close(ctx, torch):
    rng = np.random.default_rng(17)
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
        # the plain receptions: seven source symbols and two repair symbols per block (no sender has them: they stay undecodable)
        pt = np.array([tag(s, e) for s in (0, 1, 2, 4, 5, 6) for e in (0, 1, 2, 4, 6, 8, 9, 12, 11)], np.uint32)
        pk = np.full(len(pt), 99, np.uint32)
        assert (_add(torch, ctx, rset, keyed_payloads(pk, pt, T), pt, pk) == ADDED).all()
        _check_identity(rset, members)
        keys, tags = rset.want(extra=2)                                 # top up, decode: recovered blocks drop out of want ...
        n = int(tags.numel())
        answer = torch.zeros((n, sset.stride(True, True)), dtype=torch.uint8, device="cuda")  # (no sender under key 99: its rows stay 0)
        torch.cuda.synchronize()
        rset.add(sset.emit(keys, tags, out=answer, inline=True, key_inline=True), inline=True, key_inline=True)
        st, _ = rset.decode()
        nobj = sum(len(tx.blocks) for tx in txs)
        # (block order: key 7, key 99, key 0x1001 -- the objects' blocks decode, the plain receptions cannot)
        assert st[:2].all() and st[8:].all() and not st[2:8].any() and len(st) == nobj + 6
        _, _, cnt = rset.want(extra=2, per_block=True)
        assert not cnt[:2].any() and not cnt[8:].any() and list(cnt[2:8]) == [3] * 6
        _, _, hcnt = rset.held(per_block=True)                          # ... and list all K in held
        gaps, nrep = rset.counts()                                      # (K - nlost + nrep per block, the header's sum)
        assert not gaps[:2].any() and not gaps[8:].any() and nrep[:2].all()
        assert np.array_equal(hcnt, np.array([150] * 2 + [10] * 6 + [43] * 3 + [42] * 2) - gaps + nrep) and list(hcnt[2:8]) == [9] * 6
        _check_identity(rset, members)
        extra_rx[0].reset()
        _, _, hcnt = rset.held(per_block=True)
        assert list(hcnt[2:8]) == [0] * 3 + [9] * 3 and list(rset.want(source=True, per_block=True)[2][2:5]) == [10] * 3
        _check_identity(rset, members)
        rset.detach(7)
        _check_identity(rset, [m for m in members if m[0] != 7])
        extra_rx[1].close()                                             # a member closed while attached drops out of the order
        left = [m for m in members if m[0] != 7 and m[1] is not extra_rx[1]]
        assert len(rset.blocks()[0]) == 3 + 5
        assert _check_identity(rset, left) > 0
    finally:
        for h in [sset, rset] + rxs + extra_rx + txs:
            h.close()


# ------------------------------------------------------------------------------------------------- count only, the cap ----
def test_count_only_and_a_cap_too_small(ctx, torch, tables):
    tb = tables("mix4")
    L, st = ctx._L, tb.st
    u32p = C.POINTER(C.c_uint32)
    for fn, args in ((L.nrq_rxset_want, (0, 2, 0)), (L.nrq_rxset_held, ())):
        n, nb = C.c_uint32(0), len(st.blocks()[0])
        cnt = np.full(nb + 2, GUARD, np.uint32)
        assert fn(st._h, *args, None, None, 0, cnt.ctypes.data_as(u32p), C.byref(n)) == 0
        assert n.value > 8 and int(cnt[:nb].sum()) == n.value and (cnt[nb:] == GUARD).all()
        n2 = C.c_uint32(0)
        assert fn(st._h, *args, None, None, 0, None, C.byref(n2)) == 0 and n2.value == n.value   # (h_cnt NULL: the total alone)
        keys = torch.full((n.value,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        tags = torch.full((n.value,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        cnt2, n3 = np.zeros(nb, np.uint32), C.c_uint32(0)
        with pytest.raises(NrqError, match="d_tags has room for %d" % (n.value - 1)):
            ctx._chk(fn(st._h, *args, C.c_void_p(keys.data_ptr()), C.c_void_p(tags.data_ptr()), n.value - 1, cnt2.ctypes.data_as(u32p), C.byref(n3)))
        ctx.sync()
        assert n3.value == n.value and np.array_equal(cnt2, cnt[:nb])       # total and counts still filled, nothing written
        assert (keys.cpu().numpy() == 0x5A5A5A5A).all() and (tags.cpu().numpy() == 0x5A5A5A5A).all()
        assert fn(st._h, *args, None, C.c_void_p(tags.data_ptr()), n.value, None, C.byref(n3)) == 0   # d_keys NULL: the tags alone
        ctx.sync()
        ref = st.want(extra=2)[1] if args else st.held()[1]
        assert np.array_equal(tags.cpu().numpy(), ref.cpu().numpy()) and (keys.cpu().numpy() == 0x5A5A5A5A).all()


# --------------------------------------------------------------------------------- the loop with no per-member call ----
def test_the_loop_closes_with_no_per_member_call(ctx, torch):
    """two objects lose a fifth of their source packets; ReceiverSet.want(extra=2) -> ONE SenderSet.emit with key and tag inline ->
    ONE ReceiverSet.add of the buffer as emitted -> ReceiverSet.decode(): everything ADDED, every block decodes, nothing wanted"""
    rng = np.random.default_rng(77)
    txs, datas = _objects(ctx, torch, OBJ2, seed=1)
    rxs = [nanorq_amd.ObjectReceiver(ctx, *tx.oti, rep_cap=64) for tx in txs]
    sset, rset = nanorq_amd.SenderSet(ctx, T), nanorq_amd.ReceiverSet(ctx, T)
    try:
        for (key, _, _), tx, rx in zip(OBJ2, txs, rxs):
            sset.attach(key, tx)
            rset.attach(key, rx)
        _lossy_first_pass(torch, rng, OBJ2, txs, sset, rset, 0.2)
        assert (rset.counts()[0] > 0).sum() >= 6
        keys, tags = rset.want(extra=2)
        n = int(tags.numel())
        assert n > 0 and len(set(_u32(keys).tolist())) == 2
        res_tx = torch.full((n,), 77, dtype=torch.int32, device="cuda")
        res_rx = torch.full((n,), 77, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        answer = sset.emit(keys, tags, inline=True, key_inline=True, results=res_tx)
        rset.add(answer, inline=True, key_inline=True, results=res_rx)
        ctx.sync()
        assert (res_tx.cpu().numpy() == 0).all() and (res_rx.cpu().numpy() == ADDED).all()
        st, _ = rset.decode()
        assert st.all()
        for flags in (dict(extra=2), dict(source=True)):
            keys, tags, cnt = rset.want(per_block=True, **flags)
            assert keys.numel() == tags.numel() == 0 and not cnt.any()
        for rx, data in zip(rxs, datas):
            out, left = rx.write()
            ctx.sync()
            assert left == 0 and np.array_equal(out.cpu().numpy(), data)
    finally:
        for h in [sset, rset] + rxs + txs:
            h.close()


# ------------------------------------------------------------------------------------------------------ the held dump ----
def test_the_held_dump_fills_a_second_set(ctx, torch):
    """partially filled receptions with relays: ReceiverSet.held() -> ONE SenderSet.emit(held=True) over the relays -> a second
    ReceiverSet of the same shapes.  Every packet is ADDED, in list order: the second set ends with the same held list."""
    mix = [(5, 10, 3, 0), (5, 26, 2, 3), (9, 10, 3, 0)]
    tb = _mix_table(ctx, torch, mix, 150, 41)
    relays, second = [], []
    sset, rset2 = nanorq_amd.SenderSet(ctx, T), nanorq_amd.ReceiverSet(ctx, T)
    try:
        for key, rx in tb.rxs:
            relays.append(rx.relay())
            sset.attach(key, relays[-1])
            second.append(nanorq_amd.Receiver(ctx, rx.K, T, rx.nblk, rx.rep_cap, sbn0=rx.sbn0))
            rset2.attach(key, second[-1])
        keys, tags, cnt = tb.st.held(per_block=True)
        n = int(tags.numel())
        gaps, nrep = tb.st.counts()
        assert n > 30 and (gaps > 0).any() and (nrep > 0).any() and (cnt > 0).sum() >= 6
        res_tx = torch.full((n,), 77, dtype=torch.int32, device="cuda")
        res_rx = torch.full((n,), 77, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        dump = sset.emit(keys, tags, inline=True, key_inline=True, results=res_tx, held=True)
        rset2.add(dump, inline=True, key_inline=True, results=res_rx)
        ctx.sync()
        assert (res_tx.cpu().numpy() == 0).all()
        done = np.repeat(gaps == 0, cnt)   # (a block that is complete in the first set: its repair symbols come back IGN)
        assert (res_rx.cpu().numpy()[~done] == ADDED).all()
        k2, t2, cnt2 = rset2.held(per_block=True)
        first_k, first_t = _u32(keys), _u32(tags)
        if done.any():  # what a complete block holds in the second set: its K source symbols
            keep = ~done | ((first_t & 0xFFFFFF) < np.repeat([rx.K for rx in tb.in_order() for _ in range(rx.nblk)], cnt))
            first_k, first_t = first_k[keep], first_t[keep]
        assert np.array_equal(_u32(t2), first_t) and np.array_equal(_u32(k2), first_k)
    finally:
        for h in [sset, rset2] + relays + second:
            h.close()
        tb.close()


# -------------------------------------------------------------------------------------- argument and lifetime rules ----
def test_argument_and_lifetime_rules(ctx, torch):
    L = ctx._L
    err = lambda: L.nrq_ctx_error(ctx._h) or b""
    rxs = [nanorq_amd.Receiver(ctx, 10, T, 2, 4, sbn0=s) for s in (0, 2)]
    st, empty = nanorq_amd.ReceiverSet(ctx, T), nanorq_amd.ReceiverSet(ctx, T)
    try:
        st.attach(1, rxs[0])
        st.attach(2, rxs[1])
        n = C.c_uint32(7)
        buf = torch.full((64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        p = C.c_void_p(buf.data_ptr())
        for flags in (2, 3, 0x80000000):
            assert L.nrq_rxset_want(st._h, flags, 0, 0, None, None, 0, None, C.byref(n)) == -1 and n.value == 0
            assert b"nrq_rxset_want: unknown flags" in err()
        with pytest.raises(NrqError, match="nrq_rxset_want: NRQ_WANT_SOURCE takes neither"):
            st.want(source=True, extra=1)
        with pytest.raises(NrqError, match="nrq_rxset_want: NRQ_WANT_SOURCE takes neither"):
            st.want(source=True, esi_from=3)
        with pytest.raises(NrqError, match="nrq_rxset_want: extra .* is above 2\\^24"):
            st.want(extra=BIG + 1)
        assert st.want(extra=BIG)[1].numel() == 2 * 2 * 4                           # (capped at the free repair rows)
        assert L.nrq_rxset_want(st._h, 0, 0, 0, p, None, 64, None, C.byref(n)) == -1 and b"nrq_rxset_want: d_keys without d_tags" in err()
        assert L.nrq_rxset_held(st._h, p, None, 64, None, C.byref(n)) == -1 and b"nrq_rxset_held: d_keys without d_tags" in err()
        assert L.nrq_rxset_want(st._h, 0, 0, 0, None, None, 0, None, None) == -1 and b"h_n is NULL" in err()
        assert L.nrq_rxset_held(st._h, None, None, 0, None, None) == -1 and b"h_n is NULL" in err()
        assert L.nrq_rxset_want(None, 0, 0, 0, None, None, 0, None, C.byref(n)) == -1
        assert L.nrq_rxset_held(None, None, None, 0, None, C.byref(n)) == -1
        n.value = 7
        assert L.nrq_rxset_want(empty._h, 0, 2, 0, p, p, 0, None, C.byref(n)) == 0 and n.value == 0   # an empty set
        for r in (empty.want(per_block=True), empty.held(per_block=True)):
            assert r[0].numel() == r[1].numel() == 0 and len(r[2]) == 0
        ctx.sync()
        assert (buf.cpu().numpy() == 0x5A5A5A5A).all()
        keys, tags = st.want(source=True)
        assert _u32(keys).tolist() == [1] * 20 + [2] * 20
        assert _u32(tags).tolist() == [tag(s, e) for s in range(4) for e in range(10)]
        assert st.held()[1].numel() == 0
        st.close()                                                                  # a set destroyed before its members:
        assert rxs[0].want(source=True).numel() == 20                               # they stay ordinary receptions
        empty.attach(1, rxs[0])                                                     # ... free to join another set
        assert _u32(empty.want(source=True)[0]).tolist() == [1] * 20
    finally:
        for h in [st, empty] + rxs:
            h.close()


# ---------------------------------------------------------------------------------------------- a failing runtime call ----
def test_a_failing_runtime_call(torch):
    """fail_after on a context of its own: the n-th checked runtime call of ReceiverSet.want -- the count call of nrq_rxset_want,
    then its fill call -- fails, for n = 1, 2, ... up to the first n at which both succeed.  The call returns the error, the
    members' books are unchanged, and the same call afterwards gives the full list."""
    import gpu_support as G
    G.ctx()  # (torch first, as every context of this process)
    fctx = nanorq_amd.Context(0)
    tb = None
    try:
        tb = _mix_table(fctx, torch, MIX4, 1500, 35)
        ref_k, ref_t, ref_c = tb.st.want(extra=2, per_block=True)
        ref_k, ref_t = _u32(ref_k), _u32(ref_t)
        books = tb.st.lists()
        assert len(ref_t) > 8
        failed = 0
        for n_fail in range(1, 33):
            fctx.set_option("fail_after", n_fail)
            try:
                got = tb.st.want(extra=2, per_block=True)
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
            k, t, c = tb.st.want(extra=2, per_block=True)
            assert np.array_equal(_u32(k), ref_k) and np.array_equal(_u32(t), ref_t) and np.array_equal(c, ref_c), (n_fail, err)
        print("failed calls", failed)
        assert failed >= 9 and err is None   # (hipSetDevice, two error checks, the download and the wait of each call at least)
        assert np.array_equal(_u32(got[1]), ref_t)
    finally:
        if tb:
            tb.close()
        fctx.close()
