"""-m gpu tier: receptions whose repair ESIs are not one run from K -- gaps, sparse ESIs up to 2^24 - 1 (so that the ISI
ESI + K' - K of an object's larger K' row passes 2^24), any arrival order, a duplicate -- decoded by the device planner, the host
planner and a product-default context (which plans a lone small block on the host: nrq_decode_blocks_lazy "host_small"), against
the oracle's decode of the same symbols in the same order."""
import ctypes as C

import numpy as np
import pytest

import nanorq_amd
from util import loss_pattern, payload

pytestmark = pytest.mark.gpu

HIGH = [65535, 65536, 1 << 20, (1 << 24) - 1]
MAX_ESI = (1 << 24) - 1  # the device ABI's bound (the oracle's default is the object layer's, 2 K')


@pytest.fixture(scope="module", params=["device", "host", "default"])
def P(request):
    """(gpu_support kind, planner): the forced context with its device planner or with the host planner, or a default context"""
    import gpu_support
    kind = "default" if request.param == "default" else "forced"
    c = gpu_support.ctx(kind)
    host = request.param == "host"
    if host:
        c.set_planner(False)
    yield kind, c
    if host:
        c.set_planner(True)


def _esi_sets(K, n, seed):
    rng = np.random.default_rng(seed)
    gaps = np.array([K + i for i in range(3 * n + 3) if i % 3 != 2][:n], np.uint32)
    lo = max(K, 1)
    rest = rng.choice(np.arange(lo, 1 << 24, 997, dtype=np.uint64), max(n - len(HIGH), 1), replace=False).astype(np.uint32)
    sparse = np.sort(np.unique(np.concatenate([rest, [h for h in HIGH if h >= K]]).astype(np.uint32)))
    dup = np.insert(gaps, n // 2, gaps[n // 3])
    return {"gaps": gaps, "sparse": sparse, "gaps_shuffled": rng.permutation(gaps), "sparse_shuffled": rng.permutation(sparse),
            "duplicate": dup}


def _case(K, big_kp):
    Kp = nanorq_amd.params(K + K // 8 + 3)["Kp"] if big_kp else 0
    return Kp


@pytest.mark.parametrize("big_kp", [False, True], ids=["own_kp", "larger_kp"])
@pytest.mark.parametrize("K", [10, 100, 1000, 8192])
def test_scattered_repair_esis_match_oracle(P, orc, K, big_kp):
    import gpu_support as G
    kind, c = P
    T = 16
    Kp = _case(K, big_kp)
    src = payload(K * T, seed=K + big_kp, block=0).reshape(K, T)
    lost = loss_pattern(K, 0.2, seed=K, block=1)
    if len(lost) == 0:
        lost = np.array([K // 2], np.uint32)
    keep = np.setdiff1d(np.arange(K, dtype=np.uint32), lost)
    work = src.copy()
    work[lost] = 0x66
    for oh in (0, 2):
        for name, esis in _esi_sets(K, len(lost) + oh, seed=K * 3 + oh).items():
            rep, _, _ = orc.encode_block(src, K, T, esis, Kp=Kp)
            ok, r_out, _ = orc.decode_block(np.concatenate([keep, esis]), np.concatenate([src[keep], rep]), K, T, Kp=Kp,
                                         max_esi=MAX_ESI)
            st, out, _ = G.gpu_decode(work.reshape(1, K, T), K, T, [lost], [esis], [rep], Kp=Kp, kind=kind)
            what = (K, Kp, oh, name)
            assert bool(st[0]) == ok, what
            if ok:
                assert np.array_equal(out[0], r_out) and np.array_equal(out[0], src), what
            else:
                assert np.array_equal(out[0], work), what


@pytest.mark.parametrize("K", [10, 1000])
def test_repair_esi_below_k_fails_the_block(P, orc, K):
    """a 'repair' ESI < K is no repair symbol: the block fails and is left untouched, its neighbour decodes"""
    import gpu_support as G
    kind, c = P
    T = 16
    src = np.stack([payload(K * T, seed=7, block=b).reshape(K, T) for b in range(2)])
    lost = [loss_pattern(K, 0.2, seed=8, block=b) for b in range(2)]
    lost = [l if len(l) else np.array([1], np.uint32) for l in lost]
    esis = [np.arange(K, K + len(l) + 2, dtype=np.uint32) for l in lost]
    reps = [orc.encode_block(src[b], K, T, esis[b])[0] for b in range(2)]
    bad = esis[0].copy()
    bad[len(bad) // 2] = K - 1
    work = src.copy()
    for b in range(2):
        work[b][lost[b]] = 0x99
    st, out, _ = G.gpu_decode(work, K, T, lost, [bad, esis[1]], reps, kind=kind)
    assert st[0] == 0 and np.array_equal(out[0], work[0])
    assert st[1] == 1 and np.array_equal(out[1], src[1])


@pytest.mark.parametrize("K", [100, 1000])
def test_lazy_decode_of_scattered_esis_matches_oracle_on_the_prefix_used(P, orc, K):
    """decode_blocks_lazy with spare sparse repair symbols: the verdict and bytes equal the oracle's on the repair symbols the call
    reports it used (a prefix of the list, in arrival order)"""
    kind, c = P
    T, nblk = 16, 3
    src = np.stack([payload(K * T, seed=11, block=b).reshape(K, T) for b in range(nblk)])
    lost = [loss_pattern(K, 0.2, seed=12, block=b) for b in range(nblk)]
    lost = [l if len(l) else np.array([2], np.uint32) for l in lost]
    sets = [_esi_sets(K, len(l) + 6, seed=b)["sparse_shuffled"] for b, l in enumerate(lost)]
    reps = [orc.encode_block(src[b], K, T, sets[b])[0] for b in range(nblk)]
    lost_cap, rep_cap = max(len(l) for l in lost), max(len(s) for s in sets)
    lost_a = np.zeros((nblk, lost_cap), np.uint32)
    resi = np.zeros((nblk, rep_cap), np.uint32)
    rep_a = np.zeros((nblk, rep_cap, T), np.uint8)
    work = src.copy()
    for b in range(nblk):
        lost_a[b, :len(lost[b])] = lost[b]
        resi[b, :len(sets[b])] = sets[b]
        rep_a[b, :len(sets[b])] = reps[b]
        work[b][lost[b]] = 0x42
    nlost = np.array([len(l) for l in lost], np.uint32)
    d_src, d_rep = c.alloc(nblk * K * T), c.alloc(nblk * rep_cap * T)
    try:
        c.upload(d_src, work)
        c.upload(d_rep, rep_a)
        st, used = c.decode_blocks_lazy(K, T, nblk, d_src, K * T, lost_a, nlost, resi, nlost, [len(s) for s in sets], d_rep,
                                        rep_cap * T)
        c.sync()
        out = c.download(d_src, nblk * K * T).reshape(nblk, K, T)
    finally:
        c.free(d_src); c.free(d_rep)
    for b in range(nblk):
        u = int(used[b])
        assert len(lost[b]) <= u <= len(sets[b]) or (st[b] == 0 and u <= len(sets[b])), (b, u)
        keep = np.setdiff1d(np.arange(K, dtype=np.uint32), lost[b])
        ok, r_out, _ = orc.decode_block(np.concatenate([keep, sets[b][:u]]), np.concatenate([src[b][keep], reps[b][:u]]), K, T,
                                         max_esi=MAX_ESI)
        assert bool(st[b]) == ok, (b, u)
        assert np.array_equal(out[b], r_out if ok else work[b]), b


def test_object_api_sparse_high_esis():
    """the object API (product contexts) with max_esi raised to 2^24 - 1: nanorq_encode sends sparse repair ESIs up to 2^24 - 1 in
    place of the lost source symbols, nanorq_decoder_add_symbols + nanorq_repair_all must give back the object"""
    from capi import api, mem_io
    L = api()
    T = 64
    F = 2 * 700 * T - 333
    data = np.random.default_rng(3).integers(0, 256, F, dtype=np.uint8)
    rq = L.nanorq_encoder_new_ex(F, T, 0, 2, 8)
    assert rq
    io = mem_io(data)
    assert L.nanorq_set_max_esi(rq, (1 << 24) - 1)
    buf = (C.c_uint8 * T)()
    rng = np.random.default_rng(4)
    tags, blobs = [], []
    for sbn in range(L.nanorq_blocks(rq)):
        assert L.nanorq_generate_symbols(rq, sbn, io)
        K = L.nanorq_block_symbols(rq, sbn)
        lost = set(int(x) for x in rng.choice(K, K // 5, replace=False))
        esis = [e for e in range(K) if e not in lost]
        esis += sorted(set(int(x) for x in rng.integers(K, 1 << 24, len(lost) + 1)) | {65535, (1 << 24) - 1})
        for esi in esis:
            assert L.nanorq_encode(rq, buf, esi, sbn, io) == T, (sbn, esi)
            tags.append(L.nanorq_tag(sbn, esi))
            blobs.append(bytes(buf))
    oti = (L.nanorq_oti_common(rq), L.nanorq_oti_scheme_specific(rq))
    L.nanorq_free(rq)
    io.contents.destroy(io)
    order = rng.permutation(len(tags))
    tag_a = np.array([tags[i] for i in order], np.uint32)
    blob = np.frombuffer(b"".join(blobs[i] for i in order), np.uint8).copy()
    dq = L.nanorq_decoder_new(*oti)
    assert dq and L.nanorq_set_max_esi(dq, (1 << 24) - 1)
    out = np.zeros(F, np.uint8)
    oio = mem_io(out)
    try:
        res = np.full(len(tag_a), 77, np.int32)
        added = L.nanorq_decoder_add_symbols(dq, blob.ctypes.data_as(C.c_void_p), tag_a.ctypes.data_as(C.POINTER(C.c_uint32)),
                                             len(tag_a), res.ctypes.data_as(C.POINTER(C.c_int)), oio)
        assert added == len(tag_a) and (res == 0).all(), np.unique(res)
        assert L.nanorq_repair_all(dq, oio) == L.nanorq_blocks(dq)
        assert np.array_equal(out, data)
    finally:
        L.nanorq_free(dq)
        oio.contents.destroy(oio)
