"""GPU tier of the sets' packets of several symbols (nrq_rxset_add_syms / nrq_txset_emit_syms; ReceiverSet.add_syms,
SenderSet.emit_syms): the device against the CPU emulation of the same bodies (nanorq_amd/csrc/syms_set_emu.cpp) and against
each member's own emit_syms / add_syms, byte for byte, on every payload path (asserted through the exported path rule) and every
copy word; a device-only round trip against the same symbols through the one-symbol set calls; a relay member; the refusals."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import nanorq_amd
import rx_support as R
import syms_set_support as SS
import syms_support as S
import tx_support as X
from txset_support import FILL, FOREIGN, NOT_READY, Seg

pytestmark = pytest.mark.gpu

K = 100
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


# torch and the library each have a HIP runtime of their own, so nothing orders their streams: torch.cuda.synchronize() before
# the library reads what torch wrote, ctx.sync() before torch reads what the library wrote
def _dev(torch, a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _i32(torch, a):
    return _dev(torch, np.ascontiguousarray(a, np.uint32).view(np.int32))


def _L(Kp):
    return nanorq_amd.params(Kp)["L"]


def _guarded(torch, n, stride):
    buf = torch.full((n + 2, stride), FILL, dtype=torch.uint8, device="cuda")
    return buf, buf[1:n + 1]


def _guards_whole(buf):
    return bool((buf[0] == FILL).all()) and bool((buf[-1] == FILL).all())


def _stride(T, G, hdr):
    """the smallest stride that keeps the packets as aligned as T allows, plus one slack unit of that alignment"""
    al = 16 if T % 16 == 0 else 4 if T % 4 == 0 else 1
    return (G * T + hdr + al - 1) // al * al + al


# ------------------------------------------------------------------------------------------------------------------ emit ----
OBJ_KEY, OBJ_Z, RELAY_KEY = 7, 3, 11


class _EmitSet:
    """two senders with the same SBN span under different keys, a relay with block 0 ready and block 1 not, and -- where the
    object layer accepts T -- an object of two block classes (103 / 102 / 102 symbols), attached to one SenderSet.  segs: the
    senders' and the relay's table for the emulation, with the intermediate symbols the device made."""

    def __init__(self, ctx, torch, T, seed):
        rng = np.random.default_rng(seed)
        self.ctx, self.T = ctx, T
        self.set = nanorq_amd.SenderSet(ctx, T)
        self.members, self.segs, self.rows, self.hs = {}, [], [], []
        self.src = {}
        for key, nblk, sbn0 in ((5, 2, 3), (9, 3, 3)):
            Kp = nanorq_amd.params(K)["Kp"]
            src = rng.integers(0, 256, (nblk, K, T), dtype=np.uint8)
            src_d = _dev(torch, src)
            tx = nanorq_amd.Sender(ctx, K, T, nblk, src_d, sbn0=sbn0)
            tx.encode()
            ctx.sync()
            inter = ctx.download(tx.inter_ptr, nblk * _L(Kp) * T).reshape(nblk, _L(Kp), T)
            self.segs.append(Seg(key, K, Kp, T, sbn0, src, inter))
            self.rows += [(src_d.data_ptr(), K * T), (tx.inter_ptr, _L(Kp) * T)]
            self.members[key] = (tx, [SimpleNamespace(key=key, K=K, nblk=nblk, sbn0=sbn0)])
            self.src[key] = src
            self.set.attach(key, tx)
            self.hs += [tx, src_d]
        # the relay: block 0 receives every source symbol, block 1 half of them
        Kp = nanorq_amd.params(K)["Kp"]
        src = rng.integers(0, 256, (2, K, T), dtype=np.uint8)
        rx = nanorq_amd.Receiver(ctx, K, T, 2, 8)
        tags = np.array([R.tag(0, e) for e in range(K)] + [R.tag(1, e) for e in range(0, K, 2)], np.uint32)
        pl = np.stack([src[int(t) >> 24, int(t) & HI] for t in tags])
        p_d, t_d = _dev(torch, pl), _i32(torch, tags)
        rx.add(p_d, tags=t_d)
        relay = rx.relay()
        relay.encode()
        ctx.sync()
        ready = relay.ready()
        assert ready[0] and not ready[1]
        inter = ctx.download(relay.inter_ptr, 2 * _L(Kp) * T).reshape(2, _L(Kp), T)
        self.segs.append(Seg(RELAY_KEY, K, Kp, T, 0, src, inter, ready=ready))
        self.rows += [(rx.src_ptr, K * T), (relay.inter_ptr, _L(Kp) * T)]
        self.members[RELAY_KEY] = (relay, [SimpleNamespace(key=RELAY_KEY, K=K, nblk=2, sbn0=0)])
        self.set.attach(RELAY_KEY, relay)
        self.hs += [relay, rx]
        # the object
        Al = 8 if T % 8 == 0 else 4
        self.obj = None
        if T % 4 == 0 and nanorq_amd.obj_params_enc(307 * T, T, Z=OBJ_Z, Al=Al) is not None:
            data = _dev(torch, rng.integers(0, 256, 307 * T, dtype=np.uint8))
            otx = nanorq_amd.ObjectSender(ctx, data, T, Z=OBJ_Z, Al=Al)
            assert [k for k, _ in otx.blocks] == [103, 102, 102]
            otx.encode()
            ctx.sync()
            self.obj = otx
            self.rows += [(data.data_ptr(), T)]
            self.members[OBJ_KEY] = (otx, [SimpleNamespace(key=OBJ_KEY, K=103, nblk=1, sbn0=0), SimpleNamespace(key=OBJ_KEY, K=102, nblk=2, sbn0=1)])
            self.set.attach(OBJ_KEY, otx)
            self.hs += [otx, data]

    def spans(self):
        return [sp for _, sps in self.members.values() for sp in sps]

    def close(self):
        self.set.close()
        for h in self.hs:
            if hasattr(h, "close"):
                h.close()


def _set_emit(torch, ctx, st, keys, tags, nsym, G, hdr, stride, path=None, rows=()):
    """one SenderSet.emit_syms into a FILLed buffer between guard rows -> (packets, results) as numpy"""
    n = len(tags)
    buf, out = _guarded(torch, n, stride)
    if path is not None:
        assert SS.emit_path(out.data_ptr(), stride, st.T, hdr, rows) == path
    res = torch.full((n,), 77, dtype=torch.int32, device="cuda")
    k_d, t_d = _i32(torch, keys), _i32(torch, tags)
    ns_d = None if nsym is None else _dev(torch, nsym)
    torch.cuda.synchronize()
    got = st.emit_syms(k_d, t_d, G, nsym=ns_d, out=out, inline=hdr >= 4, key_inline=hdr == 8, results=res)
    ctx.sync()
    assert got is out
    assert _guards_whole(buf), "guard rows"
    return out.cpu().numpy(), res.cpu().numpy()


# (T, G, hdr, path): one row per payload path at the sizes where a boundary can go wrong
EMIT_ROWS = [
    (64, 16, 8, "TXS_V16_KEY"),     # one trip of the wave per packet
    (48, 3, 8, "TXS_V16_KEY"),      # symbol boundaries inside the run
    (16, 64, 8, "TXS_V16_KEY"),     # one lane per symbol, G at its maximum
    (1040, 2, 8, "TXS_V16_KEY"),    # the boundary and the carry in the second trip
    (64, 16, 0, "TX_V16"),
    (48, 3, 4, "TX_V16_SHIFT"),
    (20, 4, 8, "TX_DWORD"),
    (260, 2, 8, "TX_DWORD"),        # second trip
    (13, 5, 8, "TX_BYTE"),
    (65, 2, 4, "TX_BYTE"),          # second trip
    (1280, 1, 8, "TXS_V16_KEY"),    # G = 1: equals SenderSet.emit byte for byte
]


@pytest.mark.parametrize("T,G,hdr,path", EMIT_ROWS)
def test_device_emit_matches_emulation_and_members(ctx, torch, orc, T, G, hdr, path):
    m = _EmitSet(ctx, torch, T, seed=T * 100 + G)
    try:
        rng = np.random.default_rng(T + G + hdr)
        spans = m.spans()
        cases = SS.emit_cases(spans, G, rng)  # more than one wave at any G, every result code of a sender
        cases += [(RELAY_KEY, R.tag(1, 0), None), (RELAY_KEY, R.tag(1, K + 1), min(2, G))]  # the relay's block that is not ready
        if m.obj is not None:
            cases += [(OBJ_KEY, R.tag(OBJ_Z, 1), 1), (OBJ_KEY, R.tag(200, 5), None)]  # SBN >= Z: no member
        stride = _stride(T, G, hdr)
        koff = 4 if hdr == 8 else 0
        for given in (True, False):
            keys, tags, nsym = SS.case_arrays(spans, cases, G, given)
            pk, res = _set_emit(torch, ctx, m.set, keys, tags, nsym, G, hdr, stride, path=path, rows=m.rows)
            # (by the rule a packet of one symbol is never out of range: TX_BAD_RANGE needs a given count at G = 1)
            assert set(res.tolist()) == {0, FOREIGN, NOT_READY} | ({S.BAD_RANGE} if given or G > 1 else set())
            # the emulation, over the packets of the members it has tables of (a packet's bytes do not depend on the others)
            sel = np.flatnonzero(keys != OBJ_KEY)
            epk, eres, _ = SS.emu_txset_emit_syms(m.segs, keys[sel], tags[sel], None if nsym is None else nsym[sel], G, hdr, stride)
            assert np.array_equal(res[sel], eres), np.flatnonzero(res[sel] != eres)[:10]
            bad = np.flatnonzero((pk[sel] != epk).any(1))
            assert len(bad) == 0, (bad[:8], tags[sel][bad[:8]])
            # every member's own emit_syms over the packets of its key
            owned = np.zeros(len(tags), bool)
            for key, (tx, _) in m.members.items():
                ms = np.flatnonzero(keys == key)
                owned[ms] = True
                mstride = stride - koff
                mbuf, mout = _guarded(torch, len(ms), mstride)
                mres = torch.full((len(ms),), 77, dtype=torch.int32, device="cuda")
                t_d = _i32(torch, tags[ms])
                ns_d = None if nsym is None else _dev(torch, nsym[ms])
                torch.cuda.synchronize()
                tx.emit_syms(t_d, G, nsym=ns_d, out=mout, inline=hdr > 0, results=mres)
                ctx.sync()
                mpk, mres = mout.cpu().numpy(), mres.cpu().numpy()
                assert np.array_equal(res[ms], mres), key
                assert np.array_equal(pk[ms, koff:], mpk), key
                if hdr == 8:
                    ok = ms[mres == 0]
                    assert np.array_equal(pk[ok, :4], SS.be32(keys[ok])) and (pk[ms[mres != 0], :4] == FILL).all()
            assert (res[~owned] == FOREIGN).all() and (pk[~owned] == FILL).all() and (~owned).any()
            assert (pk[res != 0] == FILL).all()  # no packet is half written
            if given:  # the bytes behind hdr + c_k * T
                for k in np.flatnonzero(res == 0):
                    assert (pk[k, hdr + int(nsym[k]) * T:] == FILL).all(), k
            if G == 1 and not given:  # SenderSet.emit byte for byte
                buf1, out1 = _guarded(torch, len(tags), stride)
                res1 = torch.full((len(tags),), 77, dtype=torch.int32, device="cuda")
                k_d, t_d = _i32(torch, keys), _i32(torch, tags)
                m.set.emit(k_d, t_d, out=out1, inline=hdr >= 4, key_inline=hdr == 8, results=res1)
                ctx.sync()
                ok = res == 0
                assert np.array_equal(out1.cpu().numpy()[ok], pk[ok]) and np.array_equal(res1.cpu().numpy()[ok], res[ok])
        if (T, G, hdr) == (64, 16, 8):  # the oracle, symbol by symbol, for the first sender
            key, seg = 5, m.segs[0]
            src = m.src[key].reshape(seg.nblk, -1)
            reps = list(range(K, K + 64 + 40)) + list(range(HI - G, HI + 1))
            blocks = X.oracle_blocks(orc, src, K, T, seg.Kp, [reps] * seg.nblk)
            n_checked = 0
            for k in np.flatnonzero((keys == key) & (res == 0)):
                t = int(tags[k])
                b, e = (t >> 24) - seg.sbn0, t & HI
                assert bytes(pk[k, :8]) == int(key).to_bytes(4, "big") + t.to_bytes(4, "big")
                for i in range(S.rule(K, e, G)):
                    assert np.array_equal(pk[k, 8 + i * T: 8 + (i + 1) * T], X.expected_payload(src, blocks, K, T, b, e + i)), (k, i)
                    n_checked += 1
            assert n_checked > 100
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------------------------ ingest ----
class _IngestSet:
    """the shared members (syms_set_support.MEMBERS) on the device, twice: attached to a ReceiverSet, and as twins that are fed
    alone; and in the emulated set.  The object is there where the object layer accepts T."""

    def __init__(self, ctx, torch, T):
        self.set = nanorq_amd.ReceiverSet(ctx, T)
        self.emu = SS.EmuSetSyms()
        self.dev, self.twin, self.emus, self.hs = {}, {}, {}, []
        Al = 8 if T % 8 == 0 else 4
        self.has_obj = T % 4 == 0 and nanorq_amd.obj_params_enc(307 * T, T, Z=SS.OBJ_Z, Al=Al) is not None
        oti = None
        if self.has_obj:
            data = torch.zeros(307 * T, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            with nanorq_amd.ObjectSender(ctx, data, T, Z=SS.OBJ_Z, Al=Al) as otx:
                oti = otx.oti
        for spec in SS.MEMBERS:
            name, key, _, _, _, objZ, _ = spec
            p = SS.member_params(spec)
            if objZ:
                if not self.has_obj:
                    continue
                e = S.EmuRxSyms(p["K"], T, p["nblk"], p["rep_cap"], sbn0=p["sbn0"], max_esi=p["max_esi"], Kp=p["Kp"])
                self.emu.attach(key, e, objZ)
                self.emus[name] = e
                if name == "oL":
                    for which in (self.dev, self.twin):
                        which["obj"] = nanorq_amd.ObjectReceiver(ctx, *oti, rep_cap=p["rep_cap"])
                        assert which["obj"].params.max_esi == SS.obj_max_esi()
                        self.hs.append(which["obj"])
                    self.set.attach(key, self.dev["obj"])
                continue
            e = S.EmuRxSyms(p["K"], T, p["nblk"], p["rep_cap"], sbn0=p["sbn0"], Kp=p["Kp"])
            self.emu.attach(key, e)
            self.emus[name] = e
            for which in (self.dev, self.twin):
                src = torch.zeros((p["nblk"], p["K"], T), dtype=torch.uint8, device="cuda")
                rep = torch.zeros((p["nblk"], p["rep_cap"], T), dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                rx = nanorq_amd.Receiver(ctx, p["K"], T, p["nblk"], p["rep_cap"], sbn0=p["sbn0"], src=src, src_stride=p["K"] * T, rep=rep,
                                         rep_stride=p["rep_cap"] * T)
                which[name] = (rx, src, rep)
                self.hs.append(rx)
            self.set.attach(key, self.dev[name][0])

    def rows(self):
        return [(t.data_ptr(), t.shape[1] * t.shape[2]) for v in self.dev.values() if isinstance(v, tuple) for t in v[1:]]

    def close(self):
        self.set.close()
        for h in self.hs:
            h.close()


# (G, T, hdr, counts given, copy word): a row at each copy word; G = 3: a packet across the tile edge (slots 255..257)
INGEST_ROWS = [(3, 16, 0, True, 16), (16, 64, 8, True, 4), (4, 20, 4, False, 4), (5, 13, 8, True, 1), (3, 48, 4, False, 4),
               (64, 16, 0, False, 16)]


@pytest.mark.parametrize("G,T,hdr,given,word", INGEST_ROWS)
def test_device_ingest_matches_emulation_and_twins(ctx, torch, G, T, hdr, given, word):
    m = _IngestSet(ctx, torch, T)
    try:
        al = 16 if word == 16 else 4 if T % 4 == 0 else 1
        stride = (hdr + G * T + al - 1) // al * al + al
        codes = set()
        for call, (keys, tags, nsym) in enumerate(SS.ingest_calls(G, T, given)):
            counts = nsym if nsym is not None else np.full(len(tags), G, np.uint8)
            pkts = SS.build_packets(keys, tags, counts, G, T, hdr, stride, salt=call)
            n = len(tags)
            car = SS.carrier(keys, tags, hdr)
            pk_d = _dev(torch, pkts)
            assert SS.copy_word(pk_d.data_ptr(), stride, hdr, T, m.rows()) == word
            res = torch.full((n * G,), R.UNTOUCHED, dtype=torch.int32, device="cuda")
            k_d = None if car["keys"] is None else _i32(torch, car["keys"])
            t_d = None if car["tags"] is None else _i32(torch, car["tags"])
            ns_d = None if nsym is None else _dev(torch, nsym)
            torch.cuda.synchronize()
            m.set.add_syms(pk_d, G, keys=k_d, tags=t_d, nsym=ns_d, inline=hdr > 0, key_inline=hdr == 8, results=res)
            ctx.sync()
            got = res.cpu().numpy()
            want = m.emu.add_syms(pkts, G, key_inline=hdr == 8, nsym=nsym, **car)
            assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
            codes |= set(got.tolist())
            # each twin alone with its own add_syms over the packets of its key
            exp = np.full(n * G, R.UNTOUCHED, np.int32)
            for name, twin in m.twin.items():
                key = SS.OBJ_KEY if name == "obj" else [s[1] for s in SS.MEMBERS if s[0] == name][0]
                sel = np.flatnonzero(keys == key)
                view, inline = SS.member_view(pkts, sel, hdr)
                v_d = _dev(torch, view)
                r_d = torch.full((len(sel) * G,), R.UNTOUCHED, dtype=torch.int32, device="cuda")
                tt_d = None if inline else _i32(torch, tags[sel])
                nn_d = None if nsym is None else _dev(torch, nsym[sel])
                torch.cuda.synchronize()
                (twin if name == "obj" else twin[0]).add_syms(v_d, G, tags=tt_d, nsym=nn_d, inline=inline, results=r_d)
                ctx.sync()
                r = r_d.cpu().numpy()
                slots = (sel[:, None] * G + np.arange(G)[None, :]).reshape(-1)
                hit = r != R.UNTOUCHED
                assert (exp[slots[hit]] == R.UNTOUCHED).all()
                exp[slots[hit]] = r[hit]
                dev = m.dev[name]
                if name == "obj":
                    assert all(np.array_equal(a, b) for a, b in zip(dev.counts(), twin.counts()))
                    continue
                (lost, reps), (tlost, treps) = dev[0].lists(), twin[0].lists()
                e = m.emus[name]
                for b in range(e.nblk):  # the same lists, the repair list in slot order
                    assert np.array_equal(lost[b], tlost[b]) and np.array_equal(reps[b], treps[b]), (name, b)
                    assert np.array_equal(lost[b], e.lost(b)) and np.array_equal(reps[b], e.rep_list(b)), (name, b)
                for i in (1, 2):  # the same rows
                    assert bool((dev[i] == twin[i]).all()), (name, i)
                assert np.array_equal(dev[1].cpu().numpy(), e.src) and np.array_equal(dev[2].cpu().numpy(), e.rep), name
            assert np.array_equal(got, exp), np.flatnonzero(got != exp)[:10]
            if m.has_obj:
                nl, nr = m.dev["obj"].counts()
                eo = [m.emus["oL"], m.emus["oS"]]
                assert nl.tolist() == [int(g) for e in eo for g in e.gaps] and nr.tolist() == [int(x) for e in eo for x in e.nrep]
            unknown = np.flatnonzero(keys == SS.UNKNOWN_KEY)
            assert (got.reshape(-1, G)[unknown] == R.UNTOUCHED).all()
            if call == 0 and G == 3:
                assert got[255:258].tolist() == [R.ADDED] * 3
        assert {R.ADDED, R.DUP, R.IGN, R.ERR, R.FULL, R.UNTOUCHED} <= codes
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------------------------ round trip ----
MEMBERS_RT = [(1, 2, 0), (2, 3, 5)]  # (key, blocks, first SBN)


@pytest.mark.parametrize("seed", [1, 2])
def test_round_trip_equals_the_one_symbol_route(ctx, torch, seed):
    """SenderSet.emit_syms(key_inline) -> whole packets dropped -> ReceiverSet.add_syms -> decode, against the same symbols in the
    same order through SenderSet.emit -> ReceiverSet.add -> decode: status, used and source rows, member by member.  Per block K + 32
    ESIs are sent in packets of 16 and one source packet (16 symbols at most) is dropped: at least 16 symbols of overhead are left,
    and the one-symbol route recovers every block."""
    T, G, nrep = 64, 16, 32
    rng = np.random.default_rng(seed)
    sset = nanorq_amd.SenderSet(ctx, T)
    hs, srcs = [], []
    try:
        ks, ts, cs = [], [], []
        for key, nblk, sbn0 in MEMBERS_RT:
            src = rng.integers(0, 256, (nblk, K, T), dtype=np.uint8)
            srcs.append(src)
            src_d = _dev(torch, src)
            tx = nanorq_amd.Sender(ctx, K, T, nblk, src_d, sbn0=sbn0)
            tx.encode()
            sset.attach(key, tx)
            hs += [tx]
            t, c = S.range_list([K] * nblk, sbn0, 0, [K + nrep] * nblk, G, True)
            keep = np.ones(len(t), bool)
            for b in range(nblk):  # one source packet of every block is lost
                mine = np.flatnonzero(((t >> 24) == sbn0 + b) & ((t & HI) < K))
                keep[rng.choice(mine)] = False
            ks.append(np.full(int(keep.sum()), key, np.uint32))
            ts.append(t[keep])
            cs.append(c[keep])
        keys, tags, cnt = np.concatenate(ks), np.concatenate(ts), np.concatenate(cs)
        perm = rng.permutation(len(tags))
        keys, tags, cnt = keys[perm], tags[perm], cnt[perm]

        def receivers():
            rset, rxs = nanorq_amd.ReceiverSet(ctx, T), []
            for key, nblk, sbn0 in MEMBERS_RT:
                rx = nanorq_amd.Receiver(ctx, K, T, nblk, 40, sbn0=sbn0)
                rset.attach(key, rx)
                rxs.append(rx)
            return rset, rxs

        # packets of several symbols, the buffer as emitted
        k_d, t_d = _i32(torch, keys), _i32(torch, tags)
        res_tx = torch.full((len(tags),), 77, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        out = sset.emit_syms(k_d, t_d, G, inline=True, key_inline=True, results=res_tx)
        rset, rxs = receivers()
        hs += rxs + [rset]
        res_rx = torch.full((len(tags) * G,), R.UNTOUCHED, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        rset.add_syms(out, G, inline=True, key_inline=True, results=res_rx)
        ctx.sync()
        assert (res_tx.cpu().numpy() == 0).all()
        got = res_rx.cpu().numpy().reshape(-1, G)
        for k in range(len(tags)):
            assert (got[k, :cnt[k]] == R.ADDED).all() and (got[k, cnt[k]:] == R.UNTOUCHED).all(), k
        st_a, used_a = rset.decode()
        # the same symbols in the same order, one per packet
        _, sbn, esi = S.expansion(tags, cnt.tolist(), G)
        tags1 = np.array([R.tag(b, e) for b, e in zip(sbn, esi)], np.uint32)
        keys1 = np.repeat(keys, cnt)
        k1_d, t1_d = _i32(torch, keys1), _i32(torch, tags1)
        out1 = sset.emit(k1_d, t1_d, inline=True, key_inline=True)
        rset1, rxs1 = receivers()
        hs += rxs1 + [rset1]
        rset1.add(out1, inline=True, key_inline=True)
        st_b, used_b = rset1.decode()
        ctx.sync()
        assert st_b.all(), "the one-symbol route recovers every block"
        assert np.array_equal(st_a, st_b) and np.array_equal(used_a, used_b)
        for rx_a, rx_b, src in zip(rxs, rxs1, srcs):
            a, b = rx_a.source.cpu().numpy(), rx_b.source.cpu().numpy()
            assert np.array_equal(a, b) and np.array_equal(a, src)
    finally:
        sset.close()
        for h in hs[::-1]:
            h.close()


# ------------------------------------------------------------------------------------------------------------------ a relay ----
def test_relay_member_before_and_after_the_decode(ctx, torch):
    """a reception in a ReceiverSet, its relay in a SenderSet: before the decode a packet of its block gets TX_NOT_READY and stays
    untouched; after it, with no call on the SenderSet, its packets equal the original sender's"""
    T, G, nblk, key = 48, 3, 2, 3
    rng = np.random.default_rng(5)
    src = rng.integers(0, 256, (nblk, K, T), dtype=np.uint8)
    src_d = _dev(torch, src)
    orig = nanorq_amd.Sender(ctx, K, T, nblk, src_d)
    orig.encode()
    rx = nanorq_amd.Receiver(ctx, K, T, nblk, 24)
    relay = rx.relay()
    rset, sset_o, sset_r = nanorq_amd.ReceiverSet(ctx, T), nanorq_amd.SenderSet(ctx, T), nanorq_amd.SenderSet(ctx, T)
    try:
        rset.attach(key, rx)
        sset_o.attach(key, orig)
        sset_r.attach(key, relay)
        ask = np.array([R.tag(b, e) for b in range(nblk) for e in (0, 4, K - 2, K, K + 30, K + 33)], np.uint32)
        ask_k = np.full(len(ask), key, np.uint32)
        stride = _stride(T, G, 8)
        pk, res = _set_emit(torch, ctx, sset_r, ask_k, ask, None, G, 8, stride)
        assert (res == NOT_READY).all() and (pk == FILL).all()
        # feed: every block's ESIs 9 .. K + 20 in packets of G from the original sender (the first nine source symbols are lost)
        feed = np.array([R.tag(b, e) for b in range(nblk) for e in list(range(9, K - 1, G)) + list(range(K, K + 21, G))], np.uint32)
        f_k = np.full(len(feed), key, np.uint32)
        k_d, t_d = _i32(torch, f_k), _i32(torch, feed)
        out = sset_o.emit_syms(k_d, t_d, G, inline=True, key_inline=True)
        rset.add_syms(out, G, inline=True, key_inline=True)
        st, _ = rset.decode()
        assert st.all()
        pk, res = _set_emit(torch, ctx, sset_r, ask_k, ask, None, G, 8, stride)
        opk, ores = _set_emit(torch, ctx, sset_o, ask_k, ask, None, G, 8, stride)
        assert (res == 0).all() and np.array_equal(res, ores) and np.array_equal(pk, opk)
    finally:
        for h in (sset_r, sset_o, rset, relay, rx, orig):
            h.close()


# ------------------------------------------------------------------------------------------------------------------ refusals ----
def test_refusals_enqueue_nothing(ctx, torch):
    T, G = 16, 4
    L = ctx._L
    src = torch.zeros((1, 10, T), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    tx = nanorq_amd.Sender(ctx, 10, T, 1, src)
    tx.encode()
    rx = nanorq_amd.Receiver(ctx, 10, T, 1, 4)
    sset, rset = nanorq_amd.SenderSet(ctx, T), nanorq_amd.ReceiverSet(ctx, T)
    try:
        sset.attach(0, tx)
        rset.attach(0, rx)
        pk = torch.full((4, G * T + 8), FILL, dtype=torch.uint8, device="cuda")
        kt = torch.zeros(4, dtype=torch.int32, device="cuda")
        res = torch.full((4 * G,), 77, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        P, KT, RES = C.c_void_p(pk.data_ptr()), C.c_void_p(kt.data_ptr()), C.c_void_p(res.data_ptr())
        err = lambda: L.nrq_ctx_error(ctx._h)
        TAG, HELD, KEY = nanorq_amd.TX_TAG_INLINE, nanorq_amd.TX_HELD, nanorq_amd.TX_KEY_INLINE

        def emit(stride, keys, tags, n, g, flags, pkts=P):
            return L.nrq_txset_emit_syms(sset._h, keys, tags, n, g, None, pkts, stride, flags, RES)
        assert emit(G * T + 8, KT, KT, 4, G, TAG | KEY | HELD) == -1 and b"NRQ_TX_HELD" in err()
        assert emit(G * T + 8, KT, KT, 4, G, KEY) == -1 and b"NRQ_TX_TAG_INLINE" in err()
        assert emit(G * T + 8, KT, KT, 4, G, 8) == -1 and b"unknown flags" in err()
        assert emit(G * T + 8, KT, KT, 4, 0, 0) == -1 and emit(G * T + 8, KT, KT, 4, 65, 0) == -1 and b"outside 1..64" in err()
        assert emit(G * T - 1, KT, KT, 4, G, 0) == -1 and emit(G * T + 3, KT, KT, 4, G, TAG) == -1 and emit(G * T + 7, KT, KT, 4, G, TAG | KEY) == -1
        assert b"shorter than a packet of 4 symbols" in err()
        assert emit(G * T, KT, KT, 0x7FFFFFFF // G + 1, G, 0) == -1 and b"bad tags" in err()
        assert emit(G * T, KT, KT, 4, G, 0, pkts=None) == -1 and emit(G * T, KT, None, 4, G, 0) == -1

        RTAG, RKEY = nanorq_amd.RX_TAG_INLINE, nanorq_amd.RX_KEY_INLINE

        def add(stride, keys, tags, n, g, flags):
            return L.nrq_rxset_add_syms(rset._h, P, stride, keys, tags, n, g, None, flags, RES)
        assert add(G * T + 8, KT, KT, 4, 0, 0) == -1 and add(G * T + 8, KT, KT, 4, 65, 0) == -1 and b"outside 1..64" in err()
        assert add(G * T - 1, KT, KT, 4, G, 0) == -1 and add(G * T + 3, KT, None, 4, G, RTAG) == -1 and add(G * T + 7, None, None, 4, G, RTAG | RKEY) == -1
        assert b"shorter than a packet of 4 symbols" in err()
        assert add(G * T, KT, KT, 0x7FFFFFFF // G + 1, G, 0) == -1 and b"bad packets" in err()
        assert add(G * T + 8, KT, None, 4, G, RTAG | RKEY) == -1 and b"either d_keys or NRQ_RX_KEY_INLINE" in err()
        assert add(G * T + 8, KT, None, 4, G, RKEY) == -1 and b"NRQ_RX_TAG_INLINE" in err()
        assert add(G * T + 8, KT, KT, 4, G, RTAG) == -1 and add(G * T + 8, KT, None, 4, G, 0) == -1 and b"either d_tags or" in err()
        assert add(G * T + 8, KT, KT, 4, G, 16) == -1 and b"unknown flags" in err()
        ctx.sync()
        assert (res.cpu().numpy() == 77).all() and (pk.cpu().numpy() == FILL).all()  # nothing was enqueued: the buffers keep their fill
        assert rx.counts()[0].tolist() == [10]
        assert emit(G * T, KT, KT, 0, G, 0) == 0 and add(G * T, KT, KT, 0, G, 0) == 0  # n == 0
        with pytest.raises(nanorq_amd.NrqError, match="outside 1..64"):
            sset.emit_syms(kt, kt, 65)
    finally:
        for h in (sset, rset, tx, rx):
            h.close()
