"""GPU tier of a reception set's counts, lists and decode (nrq_rxset_blocks / _counts / _lists / _decode, ReceiverSet.blocks /
counts / lists / decode): against the members' own calls, against twin Receivers decoded one by one (verdicts, rows, books, later
packets, relays), an object through the set, a group of more than 256 blocks, the want -> emit -> add -> decode loop, the
argument and lifetime rules, and a failing runtime call."""
import ctypes as C

import numpy as np
import pytest

import nanorq_amd
from nanorq_amd import NrqError
from rx_support import ADDED, IGN
from rxset_decode_support import CHUNK, block_order, predicted_chunks, selected
from rxset_support import MIX4, MIX360, UNTOUCHED, keyed_payloads, keyed_stream, rep_cap_of, tag
from util import payload

pytestmark = pytest.mark.gpu
T = 16


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


def _add(torch, ctx, h, pl, tags, keys=None):
    """one add of host-built packets (payload rows, tags, and keys for a set) -> the result codes"""
    res = torch.full((len(tags),), UNTOUCHED, dtype=torch.int32, device="cuda")
    p_d, t_d = _dev(torch, pl), _i32(torch, tags)
    kw = {} if keys is None else dict(keys=_i32(torch, keys))
    torch.cuda.synchronize()
    h.add(p_d, tags=t_d, results=res, **kw)
    ctx.sync()
    return res.cpu().numpy()


def _concat_lists(rxs):
    """what set.lists() must give for these receivers in this order, from their own counts() and lists()"""
    nl, nr, words = [], [], []
    for rx in rxs:
        a, b = rx.counts()
        lost, reps = rx.lists()
        nl.append(a); nr.append(b)
        for x, y in zip(reps, lost):
            words += [x, y]
    return np.concatenate(nl), np.concatenate(nr), np.concatenate(words) if words else np.zeros(0, np.uint32)


# ------------------------------------------------------------------------------------- blocks, counts, lists ----
# MIX4 and a member of one block of 257 seen words: the list fill's second round (one live lane, the offset carried over)
MIX4_K8200 = MIX4 + [(7, 8200, 1, 0)]


@pytest.mark.parametrize("small_cap", [True, False])
@pytest.mark.parametrize("mix", [MIX4, MIX360, MIX4_K8200], ids=["mix4", "mix360", "mix4_k8200"])
def test_blocks_counts_lists_against_the_members(ctx, torch, mix, small_cap):
    rng = np.random.default_rng(len(mix) * 10 + small_cap)
    kps = [nanorq_amd.params(m[1])["Kp"] for m in mix]
    st = nanorq_amd.ReceiverSet(ctx, T)
    rxs = []
    try:
        for key, K, nblk, sbn0 in reversed(mix):   # (attached in another order than the block order)
            rxs.append((key, nanorq_amd.Receiver(ctx, K, T, nblk, rep_cap_of(K, small_cap), sbn0=sbn0)))
            st.attach(key, rxs[-1][1])
        for n in (1500, 20000):
            keys, tags = keyed_stream(rng, mix, kps, n)
            _add(torch, ctx, st, keyed_payloads(keys, tags, T), tags, keys)

        def check(members):
            order = block_order(members)
            k, s = st.blocks()
            assert k.dtype == s.dtype == np.uint32
            assert list(zip(k.tolist(), s.tolist())) == [(key, rx.sbn0 + b) for key, rx, b in order]
            in_order = [rx for _, rx in sorted(members, key=lambda m: (m[0], m[1].sbn0))]
            nl, nr, words = _concat_lists(in_order)
            c = st.counts()
            assert np.array_equal(c[0], nl) and np.array_equal(c[1], nr)
            l = st.lists()
            assert np.array_equal(l[0], nl) and np.array_equal(l[1], nr) and np.array_equal(l[2], words)
            assert nr.any() and len(words) == int(nl.sum()) + int(nr.sum())
            return nl
        assert check(rxs).any()
        for _, rx in rxs:
            if rx.K > 8192:  # (the second round has ESIs to place, behind those of the first)
                lost = rx.lists()[0][0]
                assert lost.min() < 32 and lost.max() >= 8192
        gone = mix[0][0]
        st.detach(gone)
        check([m for m in rxs if m[0] != gone])
    finally:
        st.close()
        for _, r in rxs:
            r.close()


# ------------------------------------------------------------------------------------------ decode against twins ----
class _Flow:
    """one reception's worth of packets from a Sender of this library: per block a reception pattern (ng lost source symbols,
    nr repair symbols) -> payload rows and tags in a fixed shuffled order"""

    def __init__(self, ctx, torch, rng, K, nblk, sbn0, patterns, Kp=0, T=T, seed=0):
        self.K, self.nblk, self.sbn0 = K, nblk, sbn0
        self.data = np.stack([payload(K * T, seed=100 + seed, block=sbn0 + b).reshape(K, T) for b in range(nblk)])
        tags = []
        for b, (ng, nr) in enumerate(patterns):
            lost = rng.choice(K, ng, replace=False)
            tags += [tag(sbn0 + b, e) for e in range(K) if e not in lost] + [tag(sbn0 + b, K + q) for q in range(nr)]
        self.tags = np.array(tags, np.uint32)[rng.permutation(len(tags))]
        src = _dev(torch, self.data)
        torch.cuda.synchronize()
        with nanorq_amd.Sender(ctx, K, T, nblk, src, sbn0=sbn0, Kp=Kp) as tx:
            tx.encode()
            self.rows = tx.emit(_i32(torch, self.tags))
            ctx.sync()
            self.rows = self.rows.cpu().numpy()


CASES = {"complete": lambda K: (0, 1), "plus2": lambda K: (2, 4), "plus0": lambda K: (2, 2), "short": lambda K: (3, 2),
         "lazy": lambda K: (2, 7)}


def test_decode_against_twins(ctx, torch):
    """Six receptions in four decode groups -- (K 10), (K 100, relay), (K 100), (K 26 with a larger K') -- against one fresh
    Receiver per member, fed the same packets and decoded on its own.  The clause `nr - ng > max_esi - K` cannot be reached
    through an ingest (a block has max_esi - K + 1 repair ESIs at most and ng >= 1 of a selected block: nr - ng <= max_esi - K), so
    the reception with max_esi = K + 3 gets a block AT the bound (ng = 1, nr = 4); the clause itself is covered value by value in
    tests/test_rxset_decode_emu.py::test_groups."""
    rng = np.random.default_rng(20)
    kp26 = nanorq_amd.params(nanorq_amd.params(26)["Kp"] + 1)["Kp"]
    assert kp26 > nanorq_amd.params(26)["Kp"]
    #        key K   nblk sbn0 Kp    max_esi relay
    spec = [(1, 10, 3, 0, 0, 0, False), (1, 10, 3, 3, 0, 0, False), (2, 10, 3, 0, 0, 13, False),
            (2, 100, 4, 3, 0, 0, True), (3, 100, 4, 0, 0, 0, False), (4, 26, 2, 0, kp26, 0, False)]
    names = list(CASES)
    drawn = [names[i] for i in rng.permutation(np.arange(16) % len(names))]
    assert set(drawn) == set(names)
    st = nanorq_amd.ReceiverSet(ctx, T)
    mem, twins, flows, kinds, hs = [], [], [], [], []
    try:
        for i, (key, K, nblk, sbn0, Kp, max_esi, relay) in enumerate(spec):
            kind = ["plus2", "bound", "short"] if max_esi else [drawn.pop() for _ in range(nblk)]
            pat = [(1, 4) if k == "bound" else CASES[k](K) for k in kind]
            kinds.append(kind)
            flows.append(_Flow(ctx, torch, rng, K, nblk, sbn0, pat, Kp=Kp, seed=i))
            mk = lambda: nanorq_amd.Receiver(ctx, K, T, nblk, K // 2 + 12, sbn0=sbn0, max_esi=max_esi, Kp=Kp)
            mem.append(mk()); twins.append(mk())
            hs += [mem[-1], twins[-1]]
        relays = {i: (mem[i].relay(), twins[i].relay()) for i, s in enumerate(spec) if s[6]}
        hs = [r for pair in relays.values() for r in pair] + hs
        for i in (4, 2, 0, 5, 3, 1):
            st.attach(spec[i][0], mem[i])
        order = block_order([(s[0], m) for s, m in zip(spec, mem)])
        idx = {(id(rx), b): j for j, (_, rx, b) in enumerate(order)}
        keys = np.concatenate([np.full(len(f.tags), s[0], np.uint32) for s, f in zip(spec, flows)])
        tags, rows = np.concatenate([f.tags for f in flows]), np.concatenate([f.rows for f in flows])
        perm = rng.permutation(len(tags))
        keys, tags, rows = keys[perm], tags[perm], rows[perm]
        own = [np.flatnonzero((keys == s[0]) & ((tags >> 24) >= s[3]) & ((tags >> 24) < s[3] + s[2])) for s in spec]
        first = _add(torch, ctx, st, rows, tags, keys)
        for i, tw in enumerate(twins):
            assert np.array_equal(_add(torch, ctx, tw, rows[own[i]], tags[own[i]]), first[own[i]])
        nl, nr = st.counts()
        status, used = st.decode()
        seen_kinds = set()
        for i, (m, tw, f) in enumerate(zip(mem, twins, flows)):
            t_st, t_used = tw.decode()
            j = [idx[(id(m), b)] for b in range(m.nblk)]
            print(i, spec[i][:3], kinds[i], "status", status[j], t_st, "used", used[j], t_used)
            assert np.array_equal(status[j], t_st) and np.array_equal(used[j], t_used), i
            ctx.sync()
            got = m.source.cpu().numpy()
            for b in range(m.nblk):
                ng, nrp = int(nl[j[b]]), int(nr[j[b]])
                exp_sel = bool(selected(ng, nrp, m.K, spec[i][5] or 2 * (spec[i][4] or nanorq_amd.params(m.K)["Kp"])))
                assert (kinds[i][b] in ("plus2", "plus0", "lazy", "bound")) == exp_sel
                if kinds[i][b] == "complete":
                    assert status[j[b]] == 1 and used[j[b]] == 0
                if kinds[i][b] == "short":
                    assert status[j[b]] == 0
                if kinds[i][b] in ("plus2", "lazy", "bound"):
                    assert status[j[b]] == 1           # (two symbols of overhead: a failure is about one in 10^6)
                if status[j[b]]:
                    assert np.array_equal(got[b], f.data[b]), (i, b)
                seen_kinds.add(kinds[i][b])
            for a, b_ in zip(m.counts(), tw.counts()):
                assert np.array_equal(a, b_)
            assert np.array_equal(m.counts()[0] == 0, status[j] == 1)
            assert np.array_equal(m.want(extra=0).cpu().numpy(), tw.want(extra=0).cpu().numpy())
            for a, b_ in zip(m.lists(), tw.lists()):
                assert all(np.array_equal(x, y) for x, y in zip(a, b_))
        assert seen_kinds == set(names) | {"bound"}
        again = _add(torch, ctx, st, rows, tags, keys)
        for i, tw in enumerate(twins):
            r = _add(torch, ctx, tw, rows[own[i]], tags[own[i]])
            assert np.array_equal(r, again[own[i]])
            done = np.isin(tags[own[i]] >> 24, [spec[i][3] + b for b in range(tw.nblk) if status[idx[(id(mem[i]), b)]]])
            assert (r[done] == IGN).all() and done.any()
        for i, (ra, rb) in relays.items():
            ready = ra.ready()
            j = [idx[(id(mem[i]), b)] for b in range(mem[i].nblk)]
            decoded = np.array([kinds[i][b] != "complete" and status[j[b]] == 1 for b in range(mem[i].nblk)])
            assert np.array_equal(ready, rb.ready()) and np.array_equal(ready, decoded) and ready.any()
            K, sbn0 = spec[i][1], spec[i][3]
            fresh = _i32(torch, np.array([tag(sbn0 + b, K + 50 + q) for b in np.flatnonzero(ready) for q in range(3)], np.uint32))
            torch.cuda.synchronize()
            pa, pb = ra.emit(fresh), rb.emit(fresh)
            ctx.sync()
            assert np.array_equal(pa.cpu().numpy(), pb.cpu().numpy())
            with nanorq_amd.Sender(ctx, K, T, mem[i].nblk, _dev(torch, flows[i].data), sbn0=sbn0) as tx:   # ... and the sender's own
                tx.encode()
                po = tx.emit(fresh)
                ctx.sync()
                assert np.array_equal(pa.cpu().numpy(), po.cpu().numpy())
    finally:
        st.close()
        for h in hs:
            h.close()


# ------------------------------------------------------------------------------------------------------ objects ----
OBJ_T = 64
OBJ = (0x1001, 213 * OBJ_T - 5, dict(Z=5))   # two block classes: 3 blocks of 43, 2 of 42 (the first shape of test_gpu_rxset.OBJECTS)
OBJ2 = (7, 300 * OBJ_T, dict(Z=2))           # one class, K = 150


def _be(a, n):
    return np.ascontiguousarray(a, np.uint32).astype(">u4").view(np.uint8).reshape(n, 4)


def _keyed(torch, key, n, emit):
    """n packets of a sender as key | FEC Payload ID | payload, rows of OBJ_T + 8 bytes; emit(out) fills them behind the key"""
    buf = torch.zeros((n, OBJ_T + 8), dtype=torch.uint8, device="cuda")
    buf[:, :4] = _dev(torch, _be(np.full(n, key, np.uint32), n))
    torch.cuda.synchronize()
    emit(buf[:, 4:])
    return buf


def test_an_object_through_the_set(ctx, torch):
    """an object of both block classes and a plain reception under another key: one set.decode()"""
    rng = np.random.default_rng(31)
    key, F, kw = OBJ
    data = payload(F, seed=F)
    K2 = 10
    data2 = payload(2 * K2 * OBJ_T, seed=5).reshape(2, K2, OBJ_T)
    hs = []
    try:
        tx = nanorq_amd.ObjectSender(ctx, _dev(torch, data), OBJ_T, **kw)
        tx2 = nanorq_amd.Sender(ctx, K2, OBJ_T, 2, _dev(torch, data2), sbn0=7)
        hs += [tx, tx2]
        tx.encode(); tx2.encode()
        assert tx.params.ZL and tx.params.ZS
        t2 = _i32(torch, np.array([tag(7 + b, e) for b in range(2) for e in range(K2 + 6)], np.uint32))
        torch.cuda.synchronize()
        pk = torch.cat([_keyed(torch, key, tx.count_all(12), lambda out: tx.emit_all(12, inline=True, out=out)),
                        _keyed(torch, 99, len(t2), lambda out: tx2.emit(t2, out=out, inline=True))])
        ctx.sync()
        pk = pk.cpu().numpy()
        pk = pk[rng.permutation(len(pk))]
        pk = pk[rng.random(len(pk)) >= 0.10]
        keys = pk[:, :4].copy().view(">u4").reshape(-1)
        rx, twin = nanorq_amd.ObjectReceiver(ctx, *tx.oti, rep_cap=24), nanorq_amd.ObjectReceiver(ctx, *tx.oti, rep_cap=24)
        plain = nanorq_amd.Receiver(ctx, K2, OBJ_T, 2, 8, sbn0=7)
        st = nanorq_amd.ReceiverSet(ctx, OBJ_T)
        hs += [st, rx, twin, plain]
        st.attach(99, plain)
        st.attach(key, rx)
        p_d = _dev(torch, pk)
        own = _dev(torch, pk[keys == key][:, 4:])
        torch.cuda.synchronize()
        st.add(p_d, inline=True, key_inline=True)
        twin.add(own, inline=True)
        assert (rx.counts()[0] > 0).any()
        k, s = st.blocks()
        assert list(zip(k.tolist(), s.tolist())) == [(99, 7), (99, 8)] + [(key, b) for b in range(rx.Z)]
        status, used = st.decode()
        t_st, t_used = twin.decode()
        assert np.array_equal(status[2:], t_st) and np.array_equal(used[2:], t_used) and t_st.all() and status[:2].all()
        out, left = rx.write()
        ctx.sync()
        assert left == 0 and np.array_equal(out.cpu().numpy(), data)
        assert np.array_equal(plain.source.cpu().numpy(), data2)
    finally:
        for h in reversed(hs):
            h.close()


def test_more_than_256_blocks_of_one_code(ctx, torch):
    """360 blocks of K = 10 in six members, every block two symbols lost and four repair symbols: one group, two decode calls"""
    rng = np.random.default_rng(41)
    flows = [_Flow(ctx, torch, rng, K, nblk, sbn0, [(2, 4)] * nblk, seed=50 + i) for i, (_, K, nblk, sbn0) in enumerate(MIX360)]
    mem = [nanorq_amd.Receiver(ctx, K, T, nblk, 6, sbn0=sbn0) for _, K, nblk, sbn0 in MIX360]
    twins = [nanorq_amd.Receiver(ctx, K, T, nblk, 6, sbn0=sbn0) for _, K, nblk, sbn0 in MIX360]
    st = nanorq_amd.ReceiverSet(ctx, T)
    try:
        for (key, _, _, _), m in zip(MIX360, mem):
            st.attach(key, m)
        keys = np.concatenate([np.full(len(f.tags), m[0], np.uint32) for m, f in zip(MIX360, flows)])
        _add(torch, ctx, st, np.concatenate([f.rows for f in flows]), np.concatenate([f.tags for f in flows]), keys)
        for tw, f in zip(twins, flows):
            _add(torch, ctx, tw, f.rows, f.tags)
        ctx.ktime_enable(True)
        status, used = st.decode()
        n_set = len(ctx.ktime_read())
        for tw in twins:
            assert tw.decode()[0].all()
        n_twins = len(ctx.ktime_read())
        ctx.ktime_enable(False)
        print("solve launches: set", n_set, "six receivers", n_twins)
        assert status.all() and len(status) == 360
        for m, f in zip(mem, flows):                  # (MIX360 is in block order: members follow each other)
            assert np.array_equal(m.source.cpu().numpy(), f.data)
            assert not m.counts()[0].any()
        assert n_set == predicted_chunks({(10, 10, 0): 360}) == 2
        assert n_set < n_twins
    finally:
        ctx.ktime_enable(False)
        st.close()
        for h in mem + twins:
            h.close()


def test_the_loop_of_two_objects_closes_through_one_decode(ctx, torch):
    """want() of both receivers -> emit from the senders upstream -> ONE set.add of the merged answer -> ONE set.decode()"""
    rng = np.random.default_rng(77)
    two = [OBJ, OBJ2]
    txs, datas = [], []
    for key, F, kw in two:
        datas.append(payload(F, seed=F + 1))
        txs.append(nanorq_amd.ObjectSender(ctx, _dev(torch, datas[-1]), OBJ_T, **kw))
        txs[-1].encode()
    rxs = [nanorq_amd.ObjectReceiver(ctx, *tx.oti, rep_cap=64) for tx in txs]
    st = nanorq_amd.ReceiverSet(ctx, OBJ_T)
    try:
        for (key, _, _), rx in zip(two, rxs):
            st.attach(key, rx)
        first = torch.cat([_keyed(torch, key, tx.count_all(0), lambda out: tx.emit_all(0, inline=True, out=out))
                           for (key, _, _), tx in zip(two, txs)])
        ctx.sync()
        first = first[_dev(torch, np.flatnonzero(rng.random(len(first)) >= 0.2))].contiguous()  # a fifth of the source symbols lost
        torch.cuda.synchronize()
        st.add(first, inline=True, key_inline=True)
        assert all((rx.counts()[0] > 0).any() for rx in rxs)
        assert not st.decode()[0].all()                 # (nothing to decode with yet: no repair symbol has arrived)
        wants = [rx.want(extra=2) for rx in rxs]
        assert all(w.numel() > 0 for w in wants)
        answer = torch.cat([_keyed(torch, key, int(w.numel()), lambda out: tx.emit(w, out=out, inline=True))
                            for (key, _, _), tx, w in zip(two, txs, wants)])
        ctx.sync()
        answer = answer[_dev(torch, rng.permutation(len(answer)))].contiguous()
        res = torch.full((len(answer),), UNTOUCHED, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        st.add(answer, inline=True, key_inline=True, results=res)
        ctx.sync()
        assert (res.cpu().numpy() == ADDED).all()
        assert all(rx.want(extra=2).numel() == 0 for rx in rxs)
        status, _ = st.decode()
        assert status.all() and len(status) == sum(rx.Z for rx in rxs)
        for rx, data in zip(rxs, datas):
            out, left = rx.write()
            ctx.sync()
            assert left == 0 and np.array_equal(out.cpu().numpy(), data)
    finally:
        st.close()
        for h in rxs + txs:
            h.close()


# ------------------------------------------------------------------------------------------------------ the API ----
def test_argument_and_lifetime_rules(ctx, torch):
    L = ctx._L
    err = lambda: L.nrq_ctx_error(ctx._h)
    u32p = C.POINTER(C.c_uint32)
    rng = np.random.default_rng(61)
    flows = [_Flow(ctx, torch, rng, 10, 2, sbn0, [(2, 4), (1, 3)], seed=70 + sbn0) for sbn0 in (0, 4, 8)]
    rxs = [nanorq_amd.Receiver(ctx, 10, T, 2, 6, sbn0=f.sbn0) for f in flows]
    st, empty = nanorq_amd.ReceiverSet(ctx, T), nanorq_amd.ReceiverSet(ctx, T)
    try:
        assert L.nrq_rxset_decode(empty._h, None, None) == -1 and b"h_status is NULL" in err()
        for a in empty.blocks() + empty.counts() + empty.lists() + empty.decode():
            assert len(a) == 0                                      # an empty set: 0 from every call, nothing to report
        for key, rx in zip((3, 2, 1), rxs):                         # block order: flows 2, 1, 0
            st.attach(key, rx)
        keys = np.concatenate([np.full(len(f.tags), k, np.uint32) for k, f in zip((3, 2, 1), flows)])
        _add(torch, ctx, st, np.concatenate([f.rows for f in flows]), np.concatenate([f.tags for f in flows]), keys)
        n, total = C.c_uint32(0), C.c_size_t(0)
        k6, s6, big = np.zeros(6, np.uint32), np.zeros(6, np.uint32), np.zeros(64, np.uint32)
        p = lambda a: a.ctypes.data_as(u32p)
        assert L.nrq_rxset_blocks(st._h, p(k6), p(s6), 5, C.byref(n)) == -1 and n.value == 6 and b"6 blocks" in err()
        assert L.nrq_rxset_blocks(st._h, None, None, 0, C.byref(n)) == 0 and n.value == 6
        assert L.nrq_rxset_blocks(st._h, p(k6), None, 6, C.byref(n)) == 0 and list(k6) == [1, 1, 2, 2, 3, 3]
        assert L.nrq_rxset_lists(st._h, None, None, p(big), 29, C.byref(total)) == -1 and total.value == 30 and b"30 words" in err()
        assert not big.any()
        assert L.nrq_rxset_lists(st._h, None, None, p(big), 30, C.byref(total)) == 0 and not big[30:].any()
        assert np.array_equal(big[:30], st.lists()[2]) and len(np.unique(big[:30])) > 5
        assert L.nrq_rxset_counts(st._h, None, None) == 0 and L.nrq_rxset_decode(st._h, None, None) == -1
        st.detach(2)                                                # decode covers only the rest ...
        status, _ = st.decode()
        assert list(status) == [1] * 4 and list(rxs[1].counts()[0]) == [2, 1]
        assert list(rxs[0].counts()[0]) == [0, 0] and list(rxs[2].counts()[0]) == [0, 0]
        st.attach(2, rxs[1])
        rxs[2].close()                                              # ... and a member closed while attached drops out of the order
        k, s = st.blocks()
        assert list(zip(k.tolist(), s.tolist())) == [(2, 4), (2, 5), (3, 0), (3, 1)]
        status, used = st.decode()
        assert list(status) == [1] * 4 and list(used[2:]) == [0, 0] and used[:2].all()
        assert np.array_equal(rxs[1].source.cpu().numpy(), flows[1].data)
    finally:
        for h in [st, empty] + rxs:
            h.close()


def test_a_failing_runtime_call(torch):
    """fail_after on a context of its own: the n-th checked runtime call of nrq_rxset_decode fails, for n = 1, 2, ... up to the
    first n at which the call succeeds.  Whatever failed, a block's gaps are 0 only if its rows hold the data; a second decode
    completes what twins complete.  Three groups (K 10, K 26, K 100 with a relay), so a failure can fall between two decode calls."""
    import gpu_support as G
    G.ctx()  # (torch first, as every context of this process)
    fctx = nanorq_amd.Context(0)
    rng = np.random.default_rng(91)
    spec = [(1, 10, 3, 0), (2, 26, 2, 0), (3, 100, 2, 5), (4, 10, 2, 9)]
    hs = []
    try:
        flows = [_Flow(fctx, torch, rng, K, nblk, sbn0, [(2, 4), (3, 3), (1, 6)][:nblk], seed=80 + i) for i, (_, K, nblk, sbn0) in enumerate(spec)]
        mem = [nanorq_amd.Receiver(fctx, K, T, nblk, 8, sbn0=sbn0) for _, K, nblk, sbn0 in spec]
        twins = [nanorq_amd.Receiver(fctx, K, T, nblk, 8, sbn0=sbn0) for _, K, nblk, sbn0 in spec]
        relay = mem[2].relay()
        hs = [relay] + mem + twins
        st = nanorq_amd.ReceiverSet(fctx, T)
        hs.insert(0, st)
        for (key, _, _, _), m in zip(spec, mem):
            st.attach(key, m)
        keys = np.concatenate([np.full(len(f.tags), s[0], np.uint32) for s, f in zip(spec, flows)])
        rows, tags = np.concatenate([f.rows for f in flows]), np.concatenate([f.tags for f in flows])
        for tw, f in zip(twins, flows):
            _add(torch, fctx, tw, f.rows, f.tags)
        t_status = np.concatenate([tw.decode()[0] for tw in twins])
        assert t_status.sum() >= 7
        failed, partial = 0, 0
        for n_fail in range(1, 65):
            for m in mem:
                m.reset()
                m.source.zero_()
            torch.cuda.synchronize()
            _add(torch, fctx, st, rows, tags, keys)
            fctx.set_option("fail_after", n_fail)
            try:
                status, _ = st.decode()
                err = None
            except NrqError as e:
                err = str(e)
            fctx.set_option("fail_after", 0)
            fctx.sync()
            if err is None:
                break  # (the call makes fewer than n_fail checked runtime calls)
            failed += 1
            gaps = np.concatenate([m.counts()[0] for m in mem])
            for m, f, g in zip(mem, flows, [m.counts()[0] for m in mem]):
                got = m.source.cpu().numpy()
                for b in range(m.nblk):
                    assert g[b] != 0 or np.array_equal(got[b], f.data[b]), (n_fail, err)
            partial += 0 < int((gaps == 0).sum()) < int(t_status.sum())
            status, _ = st.decode()                                  # the second call finishes the job
            assert np.array_equal(status, t_status), (n_fail, err)
            for m, f in zip(mem, flows):
                got = m.source.cpu().numpy()
                assert all(np.array_equal(got[b], f.data[b]) for b in range(m.nblk) if m.counts()[0][b] == 0)
            assert np.array_equal(np.concatenate([m.counts()[0] for m in mem]) == 0, t_status == 1)
        print("failed calls", failed, "of them with some chunks marked and others not", partial)
        assert failed >= 3
    finally:
        for h in hs:
            h.close()
        fctx.close()
