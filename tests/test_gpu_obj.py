"""Whole RFC 6330 objects on the device (nrq_obj_params_*, nrq_otx_* / nanorq_amd.ObjectSender, nrq_orx_* /
nanorq_amd.ObjectReceiver): the parameters against the object layer's constructors, packets against nanorq_encode of
nanorq_encoder_new_ext, result codes and decode verdicts against a host decoder, cross-decoding both ways, and device-only round
trips of the headline two-class object with and without sub-blocking."""
import ctypes as C
import hashlib
import itertools

import numpy as np
import pytest

import nanorq_amd
from capi import EXT_PER_BLOCK_KP, EXT_RFC_OTI, EXT_SUBBLOCKS, api, mem_io

ALL_FLAGS = list(range(8))
FILL = 0xA5
GUARD = 64


def _partition(I, J):
    IL, IS = -(-I // J), I // J
    JL = I - IS * J
    return (IL if JL else 0), IS, JL, J - JL


def _check_params(L, rq, p):
    Z = L.nanorq_blocks(rq)
    assert p.Z == Z and p.ZL + p.ZS == Z
    for sbn in range(Z):
        K = p.KL if sbn < p.ZL else p.KS
        assert L.nanorq_block_symbols(rq, sbn) == K, sbn
        assert L.nanorq_block_kprime(rq, sbn) == (p.KpL if sbn < p.ZL else p.KpS), sbn
    assert L.nanorq_sub_blocks(rq) == p.N
    assert L.nanorq_oti_common(rq) == p.oti_common
    assert L.nanorq_oti_scheme_specific(rq) == p.oti_specific
    uL, uS, NL, NS = _partition(p.T // p.Al, p.N)
    assert (p.NL, p.TL, p.NS, p.TS) == (NL, uL * p.Al, NS, uS * p.Al)
    assert p.Kt == p.ZL * p.KL + p.ZS * p.KS and (p.Kt - 1) * p.T < p.F <= p.Kt * p.T


def test_params_match_object_layer(monkeypatch):
    """nrq_obj_params_enc / _oti against nanorq_encoder_new_ext / nanorq_decoder_new_ext over a grid with every combination of the
    three ext flags; refused exactly where the constructors return NULL (no GPU needed)"""
    monkeypatch.setenv("NANORQ_HIP_LAZY", "1")  # (the constructors' GPU warm-up is not what is compared)
    L = api()
    n_ok = n_bad = 0
    grid = itertools.product((1, 999, 12345, 301 * 64 - 5, 70000), (16, 64, 1283, 1280), (0, 7, 100), (0, 3, 300), (1, 2, 3, 5, 700),
                             (0, 1, 4, 8), ALL_FLAGS)
    for F, T, K, Z, N, Al, flags in grid:
        rq = L.nanorq_encoder_new_ext(F, T, K, Z, N, Al, flags)
        p = nanorq_amd.obj_params_enc(F, T, K, Z, N, Al, flags)
        assert (p is None) == (not rq), (F, T, K, Z, N, Al, flags)
        if not rq:
            n_bad += 1
            continue
        n_ok += 1
        try:
            _check_params(L, rq, p)
            assert p.max_esi == 2 * L.nanorq_block_kprime(rq, 0)
            c, s = L.nanorq_oti_common(rq), L.nanorq_oti_scheme_specific(rq)
            dq = L.nanorq_decoder_new_ext(c, s, flags)
            q = nanorq_amd.obj_params_oti(c, s, flags)
            assert (q is None) == (not dq)
            if dq:
                _check_params(L, dq, q)
                assert q.as_dict() == p.as_dict()
                L.nanorq_free(dq)
        finally:
            L.nanorq_free(rq)
    assert n_ok > 500 and n_bad > 50
    rng = np.random.default_rng(9)
    for _ in range(3000):  # arbitrary OTI words, mostly refused
        c = (int(rng.integers(0, 1 << 20)) << 24) | int(rng.integers(0, 1 << 16))
        s = int(rng.integers(0, 1 << 32, dtype=np.uint64))
        if rng.random() < 0.5:
            s = (s & 0xFF00FF00) | int(rng.choice([1, 2, 4, 8]))
        flags = int(rng.integers(0, 8))
        dq = L.nanorq_decoder_new_ext(c, s, flags)
        q = nanorq_amd.obj_params_oti(c, s, flags)
        assert (q is None) == (not dq), (hex(c), hex(s), flags)
        if dq:
            _check_params(L, dq, q)
            L.nanorq_free(dq)


# ------------------------------------------------------------------------------------------------------------ GPU tier ----
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


# (F, T, K, Z, N, Al, flags): two block classes throughout; 16-byte, dword and byte emit paths; 16/8/4/1-byte layout pieces;
# the N = 1 sender in place with and without a staged last block
CASES = [
    (301 * 64 - 5, 64, 0, 3, 1, 8, 0),
    (23 * 1280 - 700, 1280, 0, 4, 3, 8, EXT_SUBBLOCKS | EXT_PER_BLOCK_KP),
    (23 * 1280, 1280, 0, 4, 4, 8, EXT_SUBBLOCKS | EXT_RFC_OTI),
    (57 * 52 - 30, 52, 0, 5, 2, 4, EXT_SUBBLOCKS | EXT_RFC_OTI | EXT_PER_BLOCK_KP),
    (40 * 13 - 3, 13, 0, 3, 2, 1, EXT_SUBBLOCKS),
    (1000 * 48 - 1, 48, 0, 2, 1, 8, EXT_PER_BLOCK_KP),
    (301 * 64, 64, 0, 3, 1, 8, 0),                 # N = 1, F = Kt*T: every block read in place, nothing staged
    (302 * 64 - 5, 64, 0, 3, 1, 8, EXT_RFC_OTI),   # class S of one block: its segment is only the staged last block
]


def _host_encoder(L, data, case):
    F, T, K, Z, N, Al, flags = case
    rq = L.nanorq_encoder_new_ext(F, T, K, Z, N, Al, flags)
    assert rq
    io = mem_io(data)
    for sbn in range(L.nanorq_blocks(rq)):
        assert L.nanorq_generate_symbols(rq, sbn, io)
    return rq, io


def _host_payload(L, rq, io, T, tag, buf):
    assert L.nanorq_encode(rq, buf, tag & 0xFFFFFF, tag >> 24, io) == T
    return bytes(buf)


def _tags(rng, blocks, n):
    Z = len(blocks)
    out = []
    for _ in range(n):
        u = rng.random()
        sbn = int(rng.integers(0, Z))
        K = blocks[sbn][0]
        if u < 0.4:
            esi = int(rng.integers(0, K))
        elif u < 0.75:
            esi = int(rng.integers(K, K + 40))
        elif u < 0.9:
            esi = int(rng.integers((1 << 24) - 30, 1 << 24))
        else:
            sbn, esi = int(rng.integers(Z, 256)), int(rng.integers(0, 50))
        out.append((sbn << 24) | esi)
    return np.array(out, np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_emit_matches_host_encoder(ctx, torch, case):
    L = api()
    F, T = case[0], case[1]
    rng = np.random.default_rng(F)
    data = rng.integers(0, 256, F, dtype=np.uint8)
    rq, io = _host_encoder(L, data, case)
    buf = (C.c_uint8 * T)()
    cache = {}

    def want(tag):
        if tag not in cache:
            cache[tag] = _host_payload(L, rq, io, T, int(tag), buf)
        return cache[tag]

    try:
        with nanorq_amd.ObjectSender(ctx, _dev(torch, data), *case[1:]) as tx:
            assert tx.oti == (L.nanorq_oti_common(rq), L.nanorq_oti_scheme_specific(rq))
            assert tx.blocks == [(L.nanorq_block_symbols(rq, b), L.nanorq_block_kprime(rq, b)) for b in range(L.nanorq_blocks(rq))]
            tx.encode()
            Z = len(tx.blocks)
            tags = _tags(rng, tx.blocks, 700)
            d_tags = _dev(torch, tags.view(np.int32))
            for inline, extra in itertools.product((False, True), (0, 3, 16)):
                stride = T + (4 if inline else 0) + extra
                out = torch.full((len(tags), stride), FILL, dtype=torch.uint8, device="cuda")
                res = torch.full((len(tags),), 77, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                tx.emit(d_tags, out=out, inline=inline, results=res)
                ctx.sync()
                out, res = out.cpu().numpy(), res.cpu().numpy()
                o = 4 if inline else 0
                for k, t in enumerate(tags):
                    if (int(t) >> 24) >= Z:
                        assert res[k] == -1 and (out[k] == FILL).all(), k
                        continue
                    assert res[k] == 0, k
                    assert bytes(out[k, o:o + T]) == want(int(t)), (k, hex(int(t)), inline, stride)
                    if inline:
                        assert bytes(out[k, :4]) == int(t).to_bytes(4, "big")
                    assert (out[k, o + T:] == FILL).all()
            nrep = 5
            bm = [(b << 24) | e for b, (K, _) in enumerate(tx.blocks) for e in range(K + nrep)]
            il = sorted(bm, key=lambda t: (t & 0xFFFFFF, t >> 24))
            for interleave, inline in itertools.product((False, True), (False, True)):
                n = tx.count_all(nrep)
                assert n == len(bm)
                tags_out = torch.zeros(n, dtype=torch.int32, device="cuda")
                out = tx.emit_all(nrep, interleave=interleave, inline=inline, tags_out=tags_out)
                ctx.sync()
                got = tags_out.cpu().numpy().view(np.uint32)
                assert list(got) == (il if interleave else bm)
                out = out.cpu().numpy()
                o = 4 if inline else 0
                for k, t in enumerate(got):
                    assert bytes(out[k, o:o + T]) == want(int(t)), (k, hex(int(t)))
                    if inline:
                        assert bytes(out[k, :4]) == int(t).to_bytes(4, "big")
    finally:
        L.nanorq_free(rq)
        io.contents.destroy(io)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_receiver_matches_host_decoder(ctx, torch, case):
    """host-encoded packets (duplicates, SBN >= Z, ESI > max_esi, packets after completion) into ObjectReceiver and a host
    decoder: the same codes packet for packet, the same decode verdicts; write() gives back the object, nothing past F"""
    L = api()
    F, T, flags = case[0], case[1], case[6]
    rng = np.random.default_rng(F + 1)
    data = rng.integers(0, 256, F, dtype=np.uint8)
    rq, io = _host_encoder(L, data, case)
    c, s = L.nanorq_oti_common(rq), L.nanorq_oti_scheme_specific(rq)
    dq = L.nanorq_decoder_new_ext(c, s, flags)
    out_host = np.zeros(F, np.uint8)
    oio = mem_io(out_host)
    buf = (C.c_uint8 * T)()
    try:
        Z = L.nanorq_blocks(rq)
        blocks = [(L.nanorq_block_symbols(rq, b), L.nanorq_block_kprime(rq, b)) for b in range(Z)]
        max_esi = 2 * blocks[0][1]
        # round 1: block 0 complete from source alone, the others lose ~20 % and get repair; plus junk and duplicates
        pk = []
        for b, (K, _) in enumerate(blocks):
            lost = set() if b == 0 else set(rng.choice(K, max(1, K // 5), replace=False).tolist())
            pk += [(b << 24) | e for e in range(K) if e not in lost]
            if b:
                pk += [(b << 24) | e for e in range(K, K + len(lost) + 2 + b % 2)]
        pk += [(Z << 24) | 1, (255 << 24) | 3, (Z << 24) | (max_esi + 5), (1 << 24) | (max_esi + 1), (0 << 24) | max_esi,
               (1 << 24) | ((1 << 24) - 1)]
        pk += [pk[i] for i in rng.choice(len(pk), 20)]
        rng.shuffle(pk)
        round2 = [(b << 24) | e for b, (K, _) in enumerate(blocks) for e in (0, K + 50, K + 51)]  # after the decode: IGN

        def host_codes(tags):
            return [L.nanorq_decoder_add_symbol(dq, _payload(t), t, oio) for t in tags]

        def _payload(t):
            if (t >> 24) >= Z:
                return bytes(T)
            return _host_payload(L, rq, io, T, t, buf)

        with nanorq_amd.ObjectReceiver(ctx, c, s, flags=flags, rep_cap=max(K for K, _ in blocks)) as rx:
            assert rx.blocks == blocks
            for ri, tags in enumerate((pk, round2)):
                tags = np.array(tags, np.uint32)
                inline = ri == 1
                stride = T + 4 + 7 if inline else T + 5
                pkts = np.full((len(tags), stride), FILL, np.uint8)
                for k, t in enumerate(tags):
                    o = 4 if inline else 0
                    pkts[k, o:o + T] = np.frombuffer(_payload(int(t)), np.uint8)
                    if inline:
                        pkts[k, :4] = np.frombuffer(int(t).to_bytes(4, "big"), np.uint8)
                want = host_codes([int(t) for t in tags])
                res = torch.full((len(tags),), 77, dtype=torch.int32, device="cuda")
                d_pk = _dev(torch, pkts)
                half = len(tags) // 2  # (two calls: the codes carry over)
                if inline:
                    rx.add(d_pk, inline=True, results=res)
                else:
                    d_tags = _dev(torch, tags.view(np.int32))
                    rx.add(d_pk[:half], tags=d_tags[:half], results=res[:half])
                    rx.add(d_pk[half:], tags=d_tags[half:], results=res[half:])
                ctx.sync()
                got = res.cpu().numpy()
                bad = [(k, hex(int(tags[k])), int(got[k]), want[k]) for k in range(len(tags)) if got[k] != want[k]]
                assert not bad, (ri, bad[:8])
                if ri == 0:
                    nl, nr = rx.counts()
                    assert list(nl) == [L.nanorq_num_missing(dq, b) for b in range(Z)]
                    assert list(nr) == [L.nanorq_num_repair(dq, b) for b in range(Z)]
                    st, _ = rx.decode()
                    hst = [int(L.nanorq_repair_block(dq, oio, b)) for b in range(Z)]
                    assert list(st) == hst
            assert all(hst)
            out = torch.full((F + GUARD,), FILL, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            _, left = rx.write(out)
            ctx.sync()
            assert left == 0
            got = out.cpu().numpy()
            assert np.array_equal(got[:F], data) and (got[F:] == FILL).all()
            assert np.array_equal(out_host, data)
    finally:
        L.nanorq_free(rq)
        L.nanorq_free(dq)
        io.contents.destroy(io)
        oio.contents.destroy(oio)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [CASES[1], CASES[3], CASES[5]])
def test_sender_packets_decode_on_host(ctx, torch, case):
    """ObjectSender.emit_all packets, 15 % lost, into nanorq_decoder_new_ext: the object comes back"""
    L = api()
    F, T, flags = case[0], case[1], case[6]
    rng = np.random.default_rng(F + 2)
    data = rng.integers(0, 256, F, dtype=np.uint8)
    with nanorq_amd.ObjectSender(ctx, _dev(torch, data), *case[1:]) as tx:
        tx.encode()
        nrep = max(K for K, _ in tx.blocks) // 4 + 4
        tags_out = torch.zeros(tx.count_all(nrep), dtype=torch.int32, device="cuda")
        pk = tx.emit_all(nrep, interleave=True, inline=False, tags_out=tags_out)
        ctx.sync()
        pk, tags = pk.cpu().numpy(), tags_out.cpu().numpy().view(np.uint32)
        c, s = tx.oti
    dq = L.nanorq_decoder_new_ext(c, s, flags)
    out = np.zeros(F, np.uint8)
    oio = mem_io(out)
    try:
        for k in rng.permutation(len(tags)):
            if rng.random() < 0.15:
                continue
            L.nanorq_decoder_add_symbol(dq, pk[k].ctypes.data_as(C.c_void_p), int(tags[k]), oio)
        for b in range(L.nanorq_blocks(dq)):
            assert L.nanorq_repair_block(dq, oio, b), b
        assert np.array_equal(out, data)
    finally:
        L.nanorq_free(dq)
        oio.contents.destroy(oio)


HEAD_F = 256 * 8192 * 1280 - 128077


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 4])
def test_headline_round_trip(ctx, torch, N):
    """the headline object (156 blocks of K=8192, 100 of K=8191; N = 1 and N = 4): emit_all (interleaved, inline) -> 10 % of
    every block's packets lost, the rest shuffled, in torch -> ObjectReceiver -> decode -> write: SHA-256 equal"""
    g = torch.Generator(device="cuda").manual_seed(N)
    obj = torch.randint(0, 256, (HEAD_F,), dtype=torch.uint8, device="cuda", generator=g)
    want = hashlib.sha256(obj.cpu().numpy().tobytes()).hexdigest()
    torch.cuda.synchronize()
    flags = EXT_SUBBLOCKS if N > 1 else 0
    nrep = 920
    with nanorq_amd.ObjectSender(ctx, obj, 1280, Z=256, N=N, Al=8, flags=flags) as tx:
        p = tx.params
        assert (p.ZL, p.KL, p.ZS, p.KS) == (156, 8192, 100, 8191)
        assert N == 1 or (p.TL, p.TS) == (0, 320) or (p.TL, p.TS) == (320, 320)
        tx.encode()
        n = tx.count_all(nrep)
        tags = torch.zeros(n, dtype=torch.int32, device="cuda")
        pk = tx.emit_all(nrep, interleave=True, inline=True, tags_out=tags)
        ctx.sync()
        common, specific = tx.oti
    sbn = (tags.view(torch.int32) >> 24) & 0xFF
    key = sbn.double() + torch.rand(n, generator=g, device="cuda", dtype=torch.float64) * 0.5
    order = torch.argsort(key)
    per = torch.bincount(sbn.long(), minlength=256)
    start = torch.cumsum(per, 0) - per
    rank = torch.arange(n, device="cuda") - start[sbn[order].long()]
    keep = per - per // 10
    kept = order[rank < keep[sbn[order].long()]]
    kept = kept[torch.randperm(len(kept), generator=g, device="cuda")]
    rx_pk = pk[kept].contiguous()
    del pk
    torch.cuda.synchronize()
    with nanorq_amd.ObjectReceiver(ctx, common, specific, flags=flags, rep_cap=nrep) as rx:
        rx.add(rx_pk, inline=True)
        st, _ = rx.decode()
        assert st.all(), np.flatnonzero(st == 0)
        out, left = rx.write()
        ctx.sync()
        assert left == 0
        assert hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest() == want


@pytest.mark.gpu
def test_headline_round_trip_on_a_default_context(torch):
    """test_headline_round_trip (N = 1) on a context with no option set: the launch choices an ObjectReceiver user gets"""
    import gpu_support as G
    test_headline_round_trip(G.default_ctx(), torch, 1)


@pytest.mark.gpu
def test_inconsistent_params_refused(ctx, torch):
    """hand-made parameter sets that break a partition (or its sums) are refused by create, before any kernel sees them"""
    F, T = 302 * 64 - 5, 64
    obj = torch.zeros(F, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    L = ctx._L
    good = nanorq_amd.obj_params_enc(F, T, 0, 3, 2, 8, EXT_SUBBLOCKS)
    kp = nanorq_amd.params(102)["Kp"]
    # sums and rows consistent, partitions not (the first one is what emit_all's index maps rely on); then plain inconsistencies
    edits = [dict(KL=102, KS=99, Kt=303, F=303 * 64 - 5, KpL=kp, KpS=kp, max_esi=2 * kp), dict(NL=1, NS=1, TL=40, TS=24),
             dict(NL=2, NS=0, TL=32, TS=32), dict(Kt=303), dict(F=F + 64), dict(max_esi=50)]
    for e in edits:
        p = nanorq_amd.ObjParams.from_buffer_copy(good)
        for k, v in e.items():
            setattr(p, k, v)
        h = C.c_void_p()
        assert L.nrq_otx_create(ctx._h, C.byref(p), C.c_void_p(obj.data_ptr()), C.byref(h)) != 0, e
        assert L.nrq_orx_create(ctx._h, C.byref(p), 16, C.byref(h)) != 0, e
    h = C.c_void_p()
    assert L.nrq_otx_create(ctx._h, C.byref(good), C.c_void_p(obj.data_ptr()), C.byref(h)) == 0
    L.nrq_otx_destroy(h)
