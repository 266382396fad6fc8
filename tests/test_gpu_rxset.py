"""GPU tier of the reception sets (nrq_rxset_*, nanorq_amd.ReceiverSet): the set's ingest kernels against their CPU emulation
(nanorq_amd/csrc/rxset_emu.cpp) byte for byte (the members' row tables prefilled and between guard rows, compared whole; the copy
kernel's 16-byte, 4-byte and byte forms also at the symbol sizes that fill a trip of its loop and start the next), against fresh Receivers fed the packets of their key through Receiver.add, whole
objects through one set call and back, the want -> emit -> add -> decode loop of two objects through a set, the API's refusals,
lifetimes, and a failed scratch allocation."""
import ctypes as C

import numpy as np
import pytest

import nanorq_amd
from nanorq_amd import EXT_SUBBLOCKS, NrqError
from rx_support import ADDED, ERR, FULL, IGN
from rxset_support import MIX4, MIX360, UNKNOWN_KEY, UNTOUCHED, EmuRx, EmuSet, keyed_payloads, keyed_stream, packets, rep_cap_of, tag
from tx_support import FILL, copy_forms
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


def _kps(mix):
    return [nanorq_amd.params(m[1])["Kp"] for m in mix]


def _guarded_rows(torch, nblk, rows, T):
    """[nblk, rows, T] row tables prefilled with FILL, a slice of one tensor with a guard row of FILL before and after it ->
    (the whole tensor, the table)"""
    whole = torch.full((nblk * rows + 2, T), FILL, dtype=torch.uint8, device="cuda")
    return whole, whole[1:-1].view(nblk, rows, T)


class _Members:
    """the receivers of a mix on the device, each over torch tensors for its rows (prefilled with FILL, between guard rows),
    attached to one set"""

    def __init__(self, ctx, torch, mix, T, small_cap, attach=True):
        self.ctx, self.mix, self.T = ctx, mix, T
        self.set = nanorq_amd.ReceiverSet(ctx, T) if attach else None
        self.rx, self.src, self.rep, self.whole = [], [], [], []
        for key, K, nblk, sbn0 in mix:
            cap = rep_cap_of(K, small_cap)
            for table, rows in ((self.src, K), (self.rep, cap)):
                w, t = _guarded_rows(torch, nblk, rows, T)
                self.whole.append(w)
                table.append(t)
            torch.cuda.synchronize()
            self.rx.append(nanorq_amd.Receiver(ctx, K, T, nblk, cap, sbn0=sbn0, src=self.src[-1], src_stride=K * T, rep=self.rep[-1],
                                               rep_stride=cap * T))
            if attach:
                self.set.attach(key, self.rx[-1])

    def close(self):
        if self.set is not None:
            self.set.close()
        for r in self.rx:
            r.close()

    def books(self, i):
        """(lost lists, repair lists, source rows, repair rows) of member i"""
        lost, reps = self.rx[i].lists()
        nl, nr = self.rx[i].counts()
        assert list(nl) == [len(x) for x in lost] and list(nr) == [len(x) for x in reps]
        return lost, reps, self.src[i].cpu().numpy(), self.rep[i].cpu().numpy()

    def guards_whole(self):
        return all(bool((w[0] == FILL).all()) and bool((w[-1] == FILL).all()) for w in self.whole)


def _emu_members(mix, T, small_cap):
    st, mem = EmuSet(), []
    for (key, K, nblk, sbn0), Kp in zip(mix, _kps(mix)):
        mem.append(EmuRx(K, T, nblk, rep_cap_of(K, small_cap), sbn0, Kp=Kp))
        mem[-1].src[:] = FILL  # (as the device tables: a row no packet landed in keeps it)
        mem[-1].rep[:] = FILL
        st.attach(key, mem[-1])
    return st, mem


def _set_add(torch, ctx, st, pk, keys, tags, inl, kinl, check=None):
    """one ReceiverSet.add of host-built packets -> the result codes (numpy); check: called with the packets' device address"""
    res = torch.full((pk.shape[0],), UNTOUCHED, dtype=torch.int32, device="cuda")
    pk_d = _dev(torch, pk)
    if check is not None:
        check(pk_d.data_ptr())
    k_d = None if keys is None else _i32(torch, keys)
    t_d = None if tags is None else _i32(torch, tags)
    torch.cuda.synchronize()
    st.add(pk_d, keys=k_d, tags=t_d, inline=inl, key_inline=kinl, results=res)
    ctx.sync()
    return res.cpu().numpy()


def _against_emulation(ctx, torch, mix, T, n, carrier, small_cap, calls=2, stride_extra=None, forms=None):
    """ReceiverSet.add calls of a keyed stream against the emulated set ingest: codes, lists, every member's source and repair
    tables whole and the guard rows around them.  stride_extra: bytes behind the packet (default: 16 or 4 times the call's number);
    forms: the forms of nrq_ing_copy_kernel the packets must take, by its rule on the addresses handed over"""
    rng = np.random.default_rng(n * 31 + T)
    kps = _kps(mix)
    dev = _Members(ctx, torch, mix, T, small_cap)
    emu, emem = _emu_members(mix, T, small_cap)
    codes = set()
    try:
        for call in range(calls):
            keys, tags = keyed_stream(rng, mix, kps, n, exact=n < 1000)
            if carrier == "nokeys":
                keys = np.zeros_like(keys)
            pl = keyed_payloads(keys, tags, T)
            extra = (16 if carrier == "arrays" else 4) * call if stride_extra is None else stride_extra
            pk, k_arg, t_arg, inl, kinl = packets(pl, keys, tags, carrier, stride_extra=extra)
            check = None
            if forms is not None:
                tables = [t.data_ptr() for t in dev.src + dev.rep]

                def check(ptr):
                    assert copy_forms(ptr, pk.shape[1], 8 if kinl else 4 if inl else 0, len(pk), T, tables) == forms
            r_dev = _set_add(torch, ctx, dev.set, pk, k_arg, t_arg, inl, kinl, check)
            r_emu = emu.add(pk, k_arg, t_arg, kinl)
            assert np.array_equal(r_dev, r_emu), np.flatnonzero(r_dev != r_emu)[:10]
            codes |= set(np.unique(r_dev).tolist())
            for i, e in enumerate(emem):
                lost, reps, s, r = dev.books(i)
                for b in range(e.nblk):
                    assert np.array_equal(lost[b], e.lost(b)) and np.array_equal(reps[b], e.rep_list(b)), (i, b)
                assert np.array_equal(s, e.src) and np.array_equal(r, e.rep), i
            assert dev.guards_whole(), "guard rows"
    finally:
        dev.close()
    return codes


CARRIERS = ("arrays", "nokeys", "inline", "keyinline")


@pytest.mark.parametrize("T,n,carrier", [(T, n, CARRIERS[(i + j) % 4]) for i, T in enumerate((16, 36, 13)) for j, n in enumerate((1, 256, 257, 3000))]
                         + [(16, 3000, c) for c in CARRIERS if c != "keyinline"])
def test_device_matches_emulation(ctx, torch, T, n, carrier):
    """the four-member mix at T = 16, 36 and 13 (the 16-byte, 4-byte and byte copy paths), every carrier of keys and tags"""
    _against_emulation(ctx, torch, MIX4, T, n, carrier, small_cap=n == 257)


# the sizes at which a form of nrq_ing_copy_kernel fills a trip of its loop or starts the next (64 lanes, two accesses in flight:
# 16-byte form 1024 + 1024 bytes a trip, dword form 256 + 256, byte form 64): (T, carrier, bytes behind the packet, forms)
COPY_EDGES = [(T, "arrays", 16, {"v16"}) for T in (1024, 1040, 2048, 2064)]                  # tags beside rows of a 16-byte stride
COPY_EDGES += [(T, "inline", (12 - T) % 16, {"dword"}) for T in (256, 260, 512, 516)]        # the payload at 4 (mod 16)
COPY_EDGES += [(T, "keyinline", (8 - T) % 16, {"dword"}) for T in (256, 260, 512, 516)]      # the payload at 8 (mod 16)
COPY_EDGES += [(63, "arrays", 0, {"byte"}), (65, "keyinline", 0, {"byte"}),
               (64, "arrays", 3, {"byte", "dword", "v16"})]  # an odd stride: three packets in four by bytes, exactly one trip; the
#                                                              others land on a 4- or 16-byte boundary and take that form


@pytest.mark.parametrize("T,carrier,extra,forms", COPY_EDGES, ids=["%d-%s" % c[:2] for c in COPY_EDGES])
def test_device_copy_at_trip_edges(ctx, torch, T, carrier, extra, forms):
    """one add of about 300 packets over the four-member mix at each edge size of the copy kernel's three forms"""
    codes = _against_emulation(ctx, torch, MIX4, T, 300, carrier, small_cap=False, calls=1, stride_extra=extra, forms=forms)
    assert ADDED in codes


def test_device_matches_emulation_360_blocks(ctx, torch):
    _against_emulation(ctx, torch, MIX360, 16, 3000, "arrays", small_cap=True)


def test_device_matches_emulation_many_tiles_and_rep_cap_overflow(ctx, torch):
    codes = _against_emulation(ctx, torch, MIX4, 16, 70000, "keyinline", small_cap=True, calls=1)
    assert FULL in codes and ERR in codes and IGN in codes


def test_device_against_receivers_alone(ctx, torch):
    """the same packets, filtered per key on the host, into fresh Receivers through Receiver.add: codes in their entries, rows and
    lists are identical; entries of foreign packets still hold the fill value"""
    T, mix = 16, MIX4
    rng = np.random.default_rng(4242)
    kps = _kps(mix)
    dev = _Members(ctx, torch, mix, T, small_cap=True)
    alone = _Members(ctx, torch, mix, T, small_cap=True, attach=False)
    try:
        for call in range(2):
            keys, tags = keyed_stream(rng, mix, kps, 3000)
            pl = keyed_payloads(keys, tags, T)
            got = _set_add(torch, ctx, dev.set, pl, keys, tags, False, False)
            exp = np.full(len(tags), UNTOUCHED, np.int32)
            for i, (key, _, _, _) in enumerate(mix):
                sel = np.flatnonzero(keys == key)
                res = torch.full((len(sel),), UNTOUCHED, dtype=torch.int32, device="cuda")
                p_d, t_d = _dev(torch, pl[sel]), _i32(torch, tags[sel])
                torch.cuda.synchronize()
                alone.rx[i].add(p_d, tags=t_d, results=res)
                ctx.sync()
                r = res.cpu().numpy()
                exp[sel[r != UNTOUCHED]] = r[r != UNTOUCHED]
            assert np.array_equal(got, exp)
            foreign = keys == UNKNOWN_KEY
            assert foreign.any() and (got[foreign] == UNTOUCHED).all() and (got == UNTOUCHED).sum() > foreign.sum()
            for i in range(len(mix)):
                a, b = dev.books(i), alone.books(i)
                assert all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))
                assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    finally:
        dev.close()
        alone.close()


# ------------------------------------------------------------------------------------------------------------------ objects ----
OBJ_T = 64
OBJECTS = [  # (key, F, ObjectSender arguments, flags)
    (0x1001, 213 * OBJ_T - 5, dict(Z=5), 0),                                      # two block classes: 3 blocks of 43, 2 of 42
    (7, 300 * OBJ_T, dict(Z=2), 0),                                               # one class, K = 150
    (0xFFFFFFFF, 90 * OBJ_T - 17, dict(Z=3, N=2, Al=8, flags=EXT_SUBBLOCKS), EXT_SUBBLOCKS),  # N > 1: sub-blocks
]


def _be(a, n):
    return np.ascontiguousarray(a, np.uint32).astype(">u4").view(np.uint8).reshape(n, 4)


def _keyed(torch, tx, key, n, emit):
    """n packets of a sender as key | FEC Payload ID | payload rows of OBJ_T + 8 bytes; emit(out, tags_out) fills them"""
    buf = torch.zeros((n, OBJ_T + 8), dtype=torch.uint8, device="cuda")
    buf[:, :4] = _dev(torch, _be(np.full(n, key, np.uint32), n))
    torch.cuda.synchronize()
    emit(buf[:, 4:])
    return buf


def _crafted(key, t):
    row = np.zeros((1, OBJ_T + 8), np.uint8)
    row[0, :4] = _be([key], 1)
    row[0, 4:8] = _be([t], 1)
    row[0, 8:] = 0xEE
    return row


def test_objects_round_trip(ctx, torch):
    """three objects' packets in one buffer, shuffled, a tenth dropped, some duplicated, with packets of SBN >= Z and of an unknown
    key: one ReceiverSet.add, then each object decodes and is written back; codes equal those of twin ObjectReceivers fed their own
    packets"""
    rng = np.random.default_rng(2024)
    nrep, rep_cap = 40, 48
    datas, otis, bufs, ps = [], [], [], []
    for key, F, kw, _ in OBJECTS:
        data = payload(F, seed=F)
        with nanorq_amd.ObjectSender(ctx, _dev(torch, data), OBJ_T, **kw) as tx:
            tx.encode()
            bufs.append(_keyed(torch, tx, key, tx.count_all(nrep), lambda out: tx.emit_all(nrep, inline=True, out=out)))
            ctx.sync()
            datas.append(data); otis.append(tx.oti); ps.append((tx.params.Z, tx.params.ZL, tx.params.ZS, tx.params.N, tx.params.max_esi))
    assert ps[0][1] and ps[0][2] and ps[2][3] > 1
    allp = torch.cat(bufs).cpu().numpy()
    n0 = len(allp)
    keep = np.flatnonzero(rng.random(n0) >= 0.10)
    pick = np.concatenate([keep, rng.choice(keep, int(0.03 * n0))])
    extra = [_crafted(OBJECTS[0][0], tag(ps[0][0], 0)), _crafted(OBJECTS[0][0], tag(200, ps[0][4] + 1)), _crafted(OBJECTS[1][0], tag(ps[1][0], 5)),
             _crafted(OBJECTS[2][0], tag(255, 0xFFFFFF))]
    unknown = allp[rng.choice(keep, 50)].copy()
    unknown[:, :4] = _be(np.full(50, UNKNOWN_KEY, np.uint32), 50)
    pk = np.concatenate([allp[pick]] + extra + [unknown])
    pk = pk[rng.permutation(len(pk))]
    keys = pk[:, :4].copy().view(">u4").reshape(-1).astype(np.uint32)
    tags = pk[:, 4:8].copy().view(">u4").reshape(-1).astype(np.uint32)
    rxs = [nanorq_amd.ObjectReceiver(ctx, *otis[i], flags=OBJECTS[i][3], rep_cap=rep_cap) for i in range(3)]
    twins = [nanorq_amd.ObjectReceiver(ctx, *otis[i], flags=OBJECTS[i][3], rep_cap=rep_cap) for i in range(3)]
    st = nanorq_amd.ReceiverSet(ctx, OBJ_T)
    try:
        for (key, _, _, _), rx in zip(OBJECTS, rxs):
            st.attach(key, rx)
        got = _set_add(torch, ctx, st, pk, None, None, True, True)
        assert (got[keys == UNKNOWN_KEY] == UNTOUCHED).all() and (got[keys != UNKNOWN_KEY] != UNTOUCHED).all()
        for i, (key, _, _, _) in enumerate(OBJECTS):
            sel = np.flatnonzero(keys == key)
            res = torch.full((len(sel),), UNTOUCHED, dtype=torch.int32, device="cuda")
            own = _dev(torch, pk[sel][:, 4:])
            torch.cuda.synchronize()
            twins[i].add(own, inline=True, results=res)
            ctx.sync()
            assert np.array_equal(got[sel], res.cpu().numpy()), i
            high = (tags[sel] >> 24) >= ps[i][0]
            assert high.any() and set(got[sel][high].tolist()) <= {ERR, IGN}
            for a, b in zip(rxs[i].counts(), twins[i].counts()):
                assert np.array_equal(a, b)
            assert rxs[i].decode()[0].all(), i
            out, left = rxs[i].write()
            ctx.sync()
            assert left == 0 and np.array_equal(out.cpu().numpy(), datas[i]), i
        assert {ERR, IGN} <= set(got[(keys == OBJECTS[0][0]) & ((tags >> 24) >= ps[0][0])].tolist())
    finally:
        st.close()
        for r in rxs + twins:
            r.close()


def test_the_loop_of_two_objects_closes_through_a_set(ctx, torch):
    """want() of both receivers -> emit from the senders upstream -> ONE set.add of the merged answer -> decode"""
    rng = np.random.default_rng(77)
    two = OBJECTS[:2]
    txs, datas = [], []
    for key, F, kw, _ in two:
        datas.append(payload(F, seed=F + 1))
        txs.append(nanorq_amd.ObjectSender(ctx, _dev(torch, datas[-1]), OBJ_T, **kw))
        txs[-1].encode()
    rxs = [nanorq_amd.ObjectReceiver(ctx, *tx.oti, rep_cap=64) for tx in txs]
    st = nanorq_amd.ReceiverSet(ctx, OBJ_T)
    try:
        for (key, _, _, _), rx in zip(two, rxs):
            st.attach(key, rx)
        first = torch.cat([_keyed(torch, tx, key, tx.count_all(0), lambda out: tx.emit_all(0, inline=True, out=out))
                           for (key, _, _, _), tx in zip(two, txs)])
        ctx.sync()
        first = first[_dev(torch, np.flatnonzero(rng.random(len(first)) >= 0.2))].contiguous()  # a fifth of the source symbols lost
        torch.cuda.synchronize()
        st.add(first, inline=True, key_inline=True)
        assert all((rx.counts()[0] > 0).any() for rx in rxs)
        wants = [rx.want(extra=2) for rx in rxs]
        assert all(w.numel() > 0 for w in wants)
        answer = torch.cat([_keyed(torch, tx, key, int(w.numel()), lambda out: tx.emit(w, out=out, inline=True))
                            for (key, _, _, _), tx, w in zip(two, txs, wants)])
        ctx.sync()
        answer = answer[_dev(torch, rng.permutation(len(answer)))].contiguous()
        res = torch.full((len(answer),), UNTOUCHED, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        st.add(answer, inline=True, key_inline=True, results=res)
        ctx.sync()
        assert (res.cpu().numpy() == ADDED).all()
        for rx, data in zip(rxs, datas):
            assert rx.want(extra=2).numel() == 0 and rx.decode()[0].all()
            out, left = rx.write()
            ctx.sync()
            assert left == 0 and np.array_equal(out.cpu().numpy(), data)
    finally:
        st.close()
        for h in rxs + txs:
            h.close()


# ------------------------------------------------------------------------------------------------------------------ the API ----
def _rx(ctx, nblk=1, sbn0=0, T=16, K=10):
    return nanorq_amd.Receiver(ctx, K, T, nblk, 2, sbn0=sbn0)


def test_attach_rules(ctx, torch):
    other = nanorq_amd.Context(0)
    hs = []

    def mk(*a, **k):
        hs.append(_rx(*a, **k))
        return hs[-1]
    st, st2 = nanorq_amd.ReceiverSet(ctx, 16), nanorq_amd.ReceiverSet(ctx, 16)
    tx = nanorq_amd.ObjectSender(ctx, _dev(torch, payload(213 * 16 - 5, seed=1)), 16, Z=5)
    orx = nanorq_amd.ObjectReceiver(ctx, *tx.oti)
    orx2 = nanorq_amd.ObjectReceiver(ctx, *tx.oti)
    try:
        a = mk(ctx, 4, 10)
        st.attach(1, a)
        with pytest.raises(NrqError, match="another context"):
            st.attach(2, mk(other))
        with pytest.raises(NrqError, match="is not the set's"):
            st.attach(2, mk(ctx, T=32))
        with pytest.raises(NrqError, match="in a set already"):
            st.attach(2, a)
        with pytest.raises(NrqError, match="in a set already"):
            st2.attach(2, a)
        for nblk, sbn0 in ((1, 10), (1, 13), (3, 8), (8, 12), (1, 12)):
            with pytest.raises(NrqError, match="overlap"):
                st.attach(1, mk(ctx, nblk, sbn0))
        st.attach(2, mk(ctx, 4, 10))   # the same span under another key
        st.attach(1, mk(ctx, 2, 14))   # another span under the same key, touching it on either side
        st.attach(1, mk(ctx, 10, 0))
        with pytest.raises(NrqError, match="owns its key"):
            st.attach(1, orx)          # an object under a key that has members
        st.attach(3, orx)
        with pytest.raises(NrqError, match="owns its key"):
            st.attach(3, mk(ctx, 1, 100))  # a member under an object's key, even beside its blocks
        with pytest.raises(NrqError, match="owns its key"):
            st.attach(3, orx2)
        with pytest.raises(NrqError, match="in a set already"):
            st2.attach(3, orx)
        with pytest.raises(NrqError, match="no member under key"):
            st.detach(99)
        st.detach(3)
        st2.attach(3, orx)             # detached: free to join another set
        st.detach(1)
        st.attach(7, a)
    finally:
        for h in [st, st2, orx, orx2, tx] + hs:
            h.close()
        other.close()


def test_caps(ctx, torch):
    hs = [_rx(ctx) for _ in range(nanorq_amd.RXSET_MAX_MEMBERS + 1)]
    big = [_rx(ctx, 256) for _ in range(4)] + [_rx(ctx, 1)]
    st, st2 = nanorq_amd.ReceiverSet(ctx, 16), nanorq_amd.ReceiverSet(ctx, 16)
    try:
        for i, h in enumerate(hs[:-1]):
            st.attach(i, h)
        with pytest.raises(NrqError, match="at most 64 receptions"):
            st.attach(1000, hs[-1])
        for i, h in enumerate(big[:-1]):
            st2.attach(i, h)
        with pytest.raises(NrqError, match="at most 1024 blocks"):
            st2.attach(1000, big[-1])
        # the full sets still ingest: one packet for the last member of each
        pl = keyed_payloads(np.array([63], np.uint32), np.array([tag(0, 3)], np.uint32), 16)
        assert _set_add(torch, ctx, st, pl, np.array([63], np.uint32), np.array([tag(0, 3)], np.uint32), False, False)[0] == ADDED
        assert _set_add(torch, ctx, st2, pl, np.array([3], np.uint32), np.array([tag(255, 3)], np.uint32), False, False)[0] == ADDED
        assert hs[63].counts()[0][0] == 9 and big[3].counts()[0][255] == 9
    finally:
        for h in [st, st2] + hs + big:
            h.close()


def test_add_argument_errors(ctx, torch):
    T = 16
    L = ctx._L
    a = _rx(ctx)
    st, empty = nanorq_amd.ReceiverSet(ctx, T), nanorq_amd.ReceiverSet(ctx, T)
    try:
        st.attach(0, a)
        pk = torch.zeros((4, T + 8), dtype=torch.uint8, device="cuda")
        kt = torch.zeros(4, dtype=torch.int32, device="cuda")
        res = torch.full((4,), UNTOUCHED, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        P, KT = C.c_void_p(pk.data_ptr()), C.c_void_p(kt.data_ptr())

        def add(stride, keys, tags, n, flags, s=st):
            return L.nrq_rxset_add(s._h, P, stride, keys, tags, n, flags, C.c_void_p(res.data_ptr()))
        TAG, KEY = nanorq_amd.RX_TAG_INLINE, nanorq_amd.RX_KEY_INLINE
        assert add(T + 8, None, KT, 4, KEY) == -1 and b"NRQ_RX_TAG_INLINE" in L.nrq_ctx_error(ctx._h)   # key inline without tag inline
        assert add(T + 8, KT, None, 4, KEY | TAG) == -1 and b"d_keys" in L.nrq_ctx_error(ctx._h)         # key inline and a key array
        assert add(T + 8, None, KT, 4, 4) == -1 and b"unknown flags" in L.nrq_ctx_error(ctx._h)
        assert add(T + 8, KT, None, 4, 0) == -1 and add(T + 8, KT, KT, 4, TAG) == -1                      # tags: either the array or inline
        assert add(T - 1, KT, KT, 4, 0) == -1 and add(T + 3, KT, None, 4, TAG) == -1 and add(T + 7, None, None, 4, TAG | KEY) == -1
        assert L.nrq_rxset_add(st._h, None, T, KT, KT, 4, 0, None) == -1
        assert add(T + 8, None, KT, 4, KEY, s=empty) == -1                                                  # flag errors come first
        assert add(T, KT, KT, 0, 0) == 0 and add(T, KT, KT, 4, 0, s=empty) == 0                            # n == 0, an empty set
        ctx.sync()
        assert (res.cpu().numpy() == UNTOUCHED).all() and a.counts()[0][0] == 10
        assert add(T, KT, KT, 4, 0) == 0 and add(T + 4, KT, None, 4, TAG) == 0 and add(T + 8, None, None, 4, TAG | KEY) == 0
        st.add(pk, tags=kt, results=None)                                                                   # d_results may be NULL
        ctx.sync()
        assert a.counts()[0][0] == 9
        with pytest.raises(ValueError):
            st.add(pk, keys=kt, inline=True, key_inline=True)
        with pytest.raises(ValueError):
            st.add(pk, tags=kt, key_inline=True)
    finally:
        for h in (st, empty, a):
            h.close()


def test_lifetimes(ctx, torch):
    """after detach that key's packets leave results untouched; a member closed before the set no longer receives; the set closed
    before its members leaves them usable"""
    T = 16
    a, b, c = _rx(ctx, 2, 0), _rx(ctx, 2, 0), _rx(ctx, 2, 0)
    st = nanorq_amd.ReceiverSet(ctx, T)
    keys = np.array([1, 2, 3, 1, 2, 3], np.uint32)
    try:
        for k, h in ((1, a), (2, b), (3, c)):
            st.attach(k, h)

        def add(esi):
            tags = np.array([tag(0, esi)] * 3 + [tag(1, esi)] * 3, np.uint32)
            return _set_add(torch, ctx, st, keyed_payloads(keys, tags, T), keys, tags, False, False).tolist()
        U = UNTOUCHED
        assert add(0) == [ADDED] * 6
        st.detach(2)
        assert add(1) == [ADDED, U, ADDED, ADDED, U, ADDED]
        c.close()
        assert add(2) == [ADDED, U, U, ADDED, U, U]
        st.attach(3, b)  # (the key of the closed member is free again)
        assert add(3) == [ADDED, U, ADDED, ADDED, U, ADDED]
        st.close()
        assert list(a.counts()[0]) == [6, 6] and list(b.counts()[0]) == [8, 8]
        for h, left in ((a, 5), (b, 7)):   # the former members are ordinary receptions: their own add, and another set
            tags = np.array([tag(0, 9), tag(1, 9)], np.uint32)
            res = torch.full((2,), U, dtype=torch.int32, device="cuda")
            p_d, t_d = _dev(torch, keyed_payloads(np.zeros(2, np.uint32), tags, T)), _i32(torch, tags)
            torch.cuda.synchronize()
            h.add(p_d, tags=t_d, results=res)
            ctx.sync()
            assert res.cpu().tolist() == [ADDED, ADDED] and list(h.counts()[0]) == [left, left]
        with nanorq_amd.ReceiverSet(ctx, T) as st3:
            st3.attach(1, a)
    finally:
        for h in (st, a, b, c):
            h.close()


def test_failed_scratch_allocation(torch):
    """fail_after on a context of its own: the n-th checked runtime call of nrq_rxset_add fails.  A failure before the kernels are
    enqueued -- the scratch allocation among them -- returns an error and leaves every member's books as they were; the next call
    succeeds and gives what the emulation gives."""
    import gpu_support as G
    G.ctx()  # (torch first, as every context of this process)
    T, mix = 16, MIX4
    rng = np.random.default_rng(5)
    kps = _kps(mix)
    hit_alloc = False
    fctx = None
    try:
        for n_fail in range(1, 8):
            fctx = nanorq_amd.Context(0)  # (a pool of its own, empty: the scratch allocation reaches the runtime)
            dev = _Members(fctx, torch, mix, T, small_cap=False)
            emu, emem = _emu_members(mix, T, False)
            try:
                keys, tags = keyed_stream(rng, mix, kps, 1500)
                pl = keyed_payloads(keys, tags, T)
                res = torch.full((len(tags),), UNTOUCHED, dtype=torch.int32, device="cuda")
                p_d, k_d, t_d = _dev(torch, pl), _i32(torch, keys), _i32(torch, tags)
                torch.cuda.synchronize()
                fctx.set_option("fail_after", n_fail)
                try:
                    dev.set.add(p_d, keys=k_d, tags=t_d, results=res)
                    err = None
                except NrqError as e:
                    err = str(e)
                fctx.set_option("fail_after", 0)
                fctx.sync()
                if err is None:
                    break  # (the call makes fewer than n_fail checked runtime calls)
                if "hipGetLastError" in err:
                    break  # (the check behind the launches: the kernels are enqueued by then)
                hit_alloc |= "hipMalloc" in err
                assert (res.cpu().numpy() == UNTOUCHED).all(), err
                for i, e in enumerate(emem):
                    lost, reps, _, _ = dev.books(i)
                    assert all(len(x) == e.K for x in lost) and all(len(x) == 0 for x in reps), err
                dev.set.add(p_d, keys=k_d, tags=t_d, results=res)
                fctx.sync()
                assert np.array_equal(res.cpu().numpy(), emu.add(pl, keys, tags)), err
                for i, e in enumerate(emem):
                    lost, reps, s, r = dev.books(i)
                    assert all(np.array_equal(lost[b], e.lost(b)) and np.array_equal(reps[b], e.rep_list(b)) for b in range(e.nblk))
                    assert np.array_equal(s, e.src) and np.array_equal(r, e.rep)
            finally:
                dev.close()
                fctx.close()
        assert hit_alloc
    finally:
        if fctx is not None:
            fctx.close()
