"""-m gpu tier: every kernel variant the ledger (tests/variant_ledger.py) marks "default", run at its shape on a context with NO
option set -- the launch choices a product caller gets.  Each test asserts from the call stats that the launch took the row's
variant and compares the results with the CPU oracle byte for byte: intermediate and repair symbols (a high ESI among them) of
an encode, and the verdict, the recovered bytes and the untouched undecodable blocks of a decode at overhead 0 and 2.  The last
test checks that every default row was seen, running any row this session has not run yet."""
import ctypes as C

import numpy as np
import pytest

import variant_ledger as V
from util import loss_pattern, payload

pytestmark = pytest.mark.gpu

SEEN = set()


@pytest.fixture(scope="module")
def D():
    import gpu_support
    return gpu_support.default_ctx()


def _solve_key(st):
    return (st["strip_bytes"], st["wg_threads"], st["wg_waves_per_simd"], 1, bool(st["movers_aligned"]))


def _encode(D, orc, K, T, nblk, seed):
    """encode on D; the intermediate symbols and repair symbols (ESI K.., and 2^24 - 1) of the first and last block against
    the oracle.  Returns (src, repair [nblk, nrep, T] for ESIs K.., stats)."""
    import gpu_support as G
    src = np.stack([payload(K * T, seed=seed, block=b).reshape(K, T) for b in range(nblk)])
    nrep = int(K * 0.45) + 8
    esis = np.concatenate([np.arange(K, K + nrep), [(1 << 24) - 1]]).astype(np.uint32)
    rep, inter = G.gpu_encode(src, K, T, esis, want_inter=True, kind="default")
    st = D.stats()
    for b in sorted({0, nblk - 1}):
        r_rep, r_int, _ = orc.encode_block(src[b], K, T, esis, want_inter=True)
        assert np.array_equal(inter[b], r_int), "intermediate symbols (K=%d T=%d block %d)" % (K, T, b)
        assert np.array_equal(rep[b], r_rep), "repair symbols (K=%d T=%d block %d)" % (K, T, b)
    return src, rep[:, :nrep], st


def _decode(D, orc, src, rep, K, T, loss, oh, seed):
    """decode every block from its received source symbols and the first len(lost) + oh repair symbols; verdict and bytes of
    every block against the oracle on the same symbols.  Returns the stats."""
    import gpu_support as G
    nblk = src.shape[0]
    lost = [loss_pattern(K, loss, seed=seed, block=b) for b in range(nblk)]
    use = [len(l) + oh for l in lost]
    assert max(use) <= rep.shape[1]
    work = src.copy()
    for b in range(nblk):
        work[b][lost[b]] = 0x3C
    esis = [np.arange(K, K + n, dtype=np.uint32) for n in use]
    st_, out, _ = G.gpu_decode(work, K, T, lost, esis, [rep[b][:use[b]] for b in range(nblk)], kind="default")
    st = D.stats()
    for b in range(nblk):
        keep = np.setdiff1d(np.arange(K, dtype=np.uint32), lost[b])
        ok, r_out, _ = orc.decode_block(np.concatenate([keep, esis[b]]), np.concatenate([src[b][keep], rep[b][:use[b]]]), K, T)
        assert bool(st_[b]) == ok, "verdict (K=%d T=%d loss=%g oh=%d block %d)" % (K, T, loss, oh, b)
        if ok:
            assert np.array_equal(out[b], r_out) and np.array_equal(out[b], src[b]), (K, T, oh, b)
        else:
            assert np.array_equal(out[b], work[b]), (K, T, oh, b, "undecodable block touched")
    return st


def _run_shape(D, orc, shape, seed):
    """encode + decode at overhead 0 and 2; returns (encode stats, [decode stats])"""
    K, T, nblk, loss = shape["K"], shape["T"], shape["nblk"], shape["loss"]
    src, rep, est = _encode(D, orc, K, T, nblk, seed)
    dst = [_decode(D, orc, src, rep, K, T, loss, oh, seed + oh) for oh in (0, 2)]
    return est, dst


def _check_solve(D, orc, key):
    row = V.SOLVE[key]
    est, dst = _run_shape(D, orc, row["shape"], seed=sum(key[:3]))
    assert (_solve_key(est), est["backsub_strip"]) == (key, row.get("backsub", 0)), ("encode", est)
    for oh, st in zip((0, 2), dst):
        # (a decode plan's inactive columns set the back-substitution strip: near K'=56403 either form occurs)
        assert _solve_key(st) == key and st["strip_bytes_b"] == 0, ("decode oh=%d" % oh, st)
        assert st["backsub_strip"] in ((16, 32) if row.get("backsub") else (0,)), ("decode oh=%d" % oh, st)
        if st["backsub_strip"]:
            SEEN.add(("backsub", st["backsub_strip"]))
    SEEN.add(("solve", key))
    if row.get("backsub"):
        SEEN.add(("backsub", row["backsub"]))


def _check_plan(D, orc, key):
    row = V.PLAN[key]
    _, dst = _run_shape(D, orc, row["shape"], seed=key[0] + key[1])
    for st in dst:
        assert (st["planner"], st["plan_wg_threads"], st["plan_compact_state"], st["host_planned"]) == (1,) + key + (0,), st
    SEEN.add(("plan", key))


def _check_feature(D, orc, name):
    row = V.FEATURES[name]
    est, dst = _run_shape(D, orc, row["shape"], seed=len(name))
    if name == "host_small":
        for st in dst:
            assert (st["planner"], st["plan_wg_threads"]) == (0, 0), st
    elif name == "plan_segmented":
        for st in dst:
            assert (st["planner"], st["plan_wg_threads"], st["plan_compact_state"], st["plan_segmented"]) == (1, 1024, 1, 1), st
    elif name == "encplan_device":
        assert est["encplan_device"] == 1, est
    SEEN.add(("feature", name))


def _check_backsub(D, orc, sb):
    """a row's decode at its exact reception (loss pattern seed, overhead): the back-substitution strip follows the decode plan's
    inactive columns (more than 640: 16-byte strips)"""
    row = V.BACKSUB[sb]
    if "via" in row:
        return _check_solve(D, orc, row["via"])
    sh = row["shape"]
    K, T = sh["K"], sh["T"]
    src, rep, _ = _encode(D, orc, K, T, sh["nblk"], seed=sb)
    st = _decode(D, orc, src, rep, K, T, sh["loss"], sh["oh"], seed=sh["seed"])
    if row.get("racy"):
        assert st["backsub_strip"] in (16, 32), st
        SEEN.add(("backsub", st["backsub_strip"]))
        return
    assert st["backsub_strip"] == sb, st
    SEEN.add(("backsub", sb))


BACKSUB_DEFAULT = [k for k, r in V.BACKSUB.items() if r["status"] == "default"]
SOLVE_DEFAULT = [k for k, r in V.SOLVE.items() if r["status"] == "default"]
PLAN_DEFAULT = [k for k, r in V.PLAN.items() if r["status"] == "default"]
FEATURE_DEFAULT = [k for k, r in V.FEATURES.items() if r["status"] == "default"]


def _id(key):
    return "-".join(str(x) for x in key)


@pytest.mark.parametrize("key", SOLVE_DEFAULT, ids=_id)
def test_solve_variant(D, orc, key):
    _check_solve(D, orc, key)


@pytest.mark.parametrize("sb", BACKSUB_DEFAULT)
def test_backsub_variant(D, orc, sb):
    _check_backsub(D, orc, sb)


@pytest.mark.parametrize("key", PLAN_DEFAULT, ids=_id)
def test_planner_variant(D, orc, key):
    _check_plan(D, orc, key)


@pytest.mark.parametrize("name", FEATURE_DEFAULT)
def test_launch_feature(D, orc, name):
    _check_feature(D, orc, name)


def _object(torch, case, seed):
    F = case[0]
    data = np.random.default_rng(seed).integers(0, 256, F, dtype=np.uint8)
    return data, torch.from_numpy(data).cuda()


def test_object_emit_modes(D, torch_mod, orc):
    """nrq_emit_kernel<MODE, true> (a table of three segments: class L, class S, the staged last block) in each of its four
    modes (the alignment of the packet rows picks it: tx_launch), against nanorq_encode of the object layer: byte rows (odd
    stride), 4-byte rows, 16-byte rows, 16-byte rows behind an inline header"""
    from capi import api
    from test_gpu_obj import FILL, _host_encoder, _host_payload, _tags
    import nanorq_amd
    torch = torch_mod
    L = api()
    case = (301 * 64 - 5, 64, 0, 3, 1, 8, 0)
    T = case[1]
    data, obj = _object(torch, case, 5)
    rq, io = _host_encoder(L, data, case)
    buf = (C.c_uint8 * T)()
    try:
        with nanorq_amd.ObjectSender(D, obj, *case[1:]) as tx:
            tx.encode()
            tags = _tags(np.random.default_rng(6), tx.blocks, 300)
            tags = tags[(tags >> 24) < len(tx.blocks)]
            d_tags = torch.from_numpy(tags.view(np.int32)).cuda()
            # (inline, row stride): TX_BYTE, TX_DWORD, TX_V16, TX_V16_SHIFT
            for inline, stride in [(False, T + 3), (True, T + 4), (False, T + 16), (True, T + 16)]:
                o = 4 if inline else 0
                big = torch.full((len(tags), stride), FILL, dtype=torch.uint8, device="cuda")
                out = big[:, :T + o]
                torch.cuda.synchronize()
                tx.emit(d_tags, out=out, inline=inline)
                D.sync()
                got = big.cpu().numpy()
                for k, t in enumerate(tags):
                    assert bytes(got[k, o:o + T]) == _host_payload(L, rq, io, T, int(t), buf), (k, hex(int(t)), inline, stride)
                    if inline:
                        assert bytes(got[k, :4]) == int(t).to_bytes(4, "big")
                    assert (got[k, o + T:] == FILL).all()
    finally:
        L.nanorq_free(rq)
        io.contents.destroy(io)


def test_object_layout_widths(D, torch_mod):
    """nrq_obj_layout_kernel at 2-byte pieces (T = 28 in two sub-blocks of 14 bytes, Al = 2) -- the one width no other GPU test
    lays out -- and at 16 (N = 1): the sender's packets through the object receiver back into the object"""
    import nanorq_amd
    from capi import EXT_SUBBLOCKS
    torch = torch_mod
    for case in [(40 * 28 - 3, 28, 0, 3, 2, 2, EXT_SUBBLOCKS), (40 * 32 - 3, 32, 0, 3, 1, 8, 0)]:
        data, obj = _object(torch, case, case[1])
        with nanorq_amd.ObjectSender(D, obj, *case[1:]) as tx:
            p = tx.params
            assert case[4] == 1 or (p.TL, p.TS) in ((0, 14), (14, 14))  # (2-byte pieces: 28 | TL | TS)
            tx.encode()
            nrep = 12
            tags = torch.zeros(tx.count_all(nrep), dtype=torch.int32, device="cuda")
            pk = tx.emit_all(nrep, interleave=True, inline=True, tags_out=tags)
            D.sync()
            common, specific = tx.oti
        # every block loses its first four source packets; the repair packets stand in for them
        t = tags.cpu().numpy().view(np.uint32)
        keep = torch.from_numpy(np.flatnonzero((t & 0xFFFFFF) >= 4)).cuda()
        rx_pk = pk[keep].contiguous()
        torch.cuda.synchronize()
        with nanorq_amd.ObjectReceiver(D, common, specific, flags=case[6], rep_cap=nrep) as rx:
            rx.add(rx_pk, inline=True)
            st, _ = rx.decode()
            out, left = rx.write()
            D.sync()
        assert st.all() and left == 0
        assert np.array_equal(out.cpu().numpy(), data), case


@pytest.fixture(scope="module")
def torch_mod():
    import torch as t
    assert t.cuda.is_available()
    return t


def test_every_default_row_was_seen(D, orc):
    """every "default" row of the ledger has been run and seen at its variant -- rows not run yet in this session run now"""
    for key in SOLVE_DEFAULT:
        if ("solve", key) not in SEEN:
            _check_solve(D, orc, key)
    for key in PLAN_DEFAULT:
        if ("plan", key) not in SEEN:
            _check_plan(D, orc, key)
    for name in FEATURE_DEFAULT:
        if ("feature", name) not in SEEN:
            _check_feature(D, orc, name)
    for sb, row in V.BACKSUB.items():
        if row["status"] == "default" and ("backsub", sb) not in SEEN:
            _check_backsub(D, orc, sb)
            assert row.get("racy") or ("backsub", sb) in SEEN, sb
