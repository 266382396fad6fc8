"""-m gpu tier: seeded random shapes through the C ABI -- block size, symbol size (incl. sizes whose last 128-byte line
group is partial and single bytes), block count, loss rate and overhead drawn at random; every decodable block must come
back bit-exact, undecodable ones untouched, and one block per case is compared with the CPU oracle byte for byte
(repair symbols, intermediate symbols, decode verdict)."""
import numpy as np
import pytest

from util import loss_pattern, payload, received_set

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import gpu_support
    gpu_support.ctx()
    return gpu_support


@pytest.fixture(scope="module")
def GD():
    """gpu_support bound to a product-default context (no option set): the *_on_a_default_context tests run the same cases there"""
    import gpu_support
    return gpu_support.bound("default")


@pytest.mark.parametrize("seed", range(8))
def test_random_shapes(G, orc, seed):
    """(Seeds 6 and 7 with 12-byte strips forced -- the width of K ~ 8500-12000 -- on these small shapes: every symbol size that ends
    inside a strip or a dword goes through its movers, byte-wise and aligned forms alike.)"""
    if seed >= 6:
        G.ctx().set_option("max_wb", 12)
    try:
        _random_shapes(G, orc, seed)
    finally:
        G.ctx().set_option("max_wb", 16)


@pytest.mark.parametrize("seed", range(8))
def test_random_shapes_on_a_default_context(GD, orc, seed):
    test_random_shapes(GD, orc, seed)


def _random_shapes(G, orc, seed):
    rng = np.random.default_rng(4000 + seed)
    for trial in range(30):
        K = int(rng.choice([1, 2, 7, 10, 11, 26, 55, 100, 101, 257, 400, 777, 1024, 1500, 2049, 2600, 3100]))
        T = int(rng.choice([1, 2, 3, 5, 8, 15, 16, 17, 31, 40, 64, 100, 128, 129, 200, 272]))
        nblk = int(rng.choice([1, 2, 3, 7, 8, 9, 16, 33]))
        if K * T * nblk > 24 << 20:
            nblk = max(1, (24 << 20) // (K * T))
        p = float(rng.choice([0.02, 0.1, 0.3, 0.6]))
        oh = int(rng.choice([0, 0, 1, 2, 5]))
        src = np.stack([payload(K * T, seed=seed * 100 + trial, block=b).reshape(K, T) for b in range(nblk)])
        lost = [loss_pattern(K, p, seed=seed * 977 + trial, block=b) for b in range(nblk)]
        nrep = max(len(l) for l in lost) + oh
        esis = np.arange(K, K + nrep, dtype=np.uint32)
        rep, inter = G.gpu_encode(src, K, T, esis, want_inter=True)
        b0 = int(rng.integers(nblk))
        r_rep, r_int, _ = orc.encode_block(src[b0], K, T, esis, want_inter=True)
        assert np.array_equal(rep[b0], r_rep) and np.array_equal(inter[b0], r_int), (K, T, nblk, "encode")
        work = src.copy()
        for b in range(nblk):
            work[b][lost[b]] = 0x77
        use = [len(l) + (oh if len(l) else 0) for l in lost]
        st, out, _ = G.gpu_decode(work, K, T, lost, [esis[:n] for n in use], [rep[b][:use[b]] for b in range(nblk)])
        for b in range(nblk):
            if st[b]:
                assert np.array_equal(out[b], src[b]), (K, T, nblk, p, oh, b)
            else:
                assert np.array_equal(out[b], work[b]), (K, T, nblk, p, oh, b, "undecodable block touched")
        # the verdict of one block against the reference algorithm
        rx = received_set(K, lost[b0], oh if len(lost[b0]) else 0)
        syms = np.concatenate([src[b0][rx[rx < K]], rep[b0][:use[b0]]]) if use[b0] else src[b0][rx[rx < K]]
        ok, _, _ = orc.decode_block(rx, syms, K, T)
        assert bool(st[b0]) == ok, (K, T, nblk, p, oh, b0, "verdict")


@pytest.mark.parametrize("K,T,nblk,p,iters", [(700, 32, 2048, 0.1, 6), (2000, 32, 1024, 0.2, 4), (8192, 16, 256, 0.1, 3), (9400, 16, 64, 0.1, 2)])
def test_many_reception_patterns_through_the_device_planner(K, T, nblk, p, iters):
    """Thousands of different reception patterns per launch through the device planner -- the chained peel, the batched
    inactivation events and the forms of the peeling state by block size (planner_body.h) race by design (who claims a column
    first, in which order the list fills), so their check is volume: every block of every launch must decode to its source.  (One
    in ~20 000 plans of K=700 / 2000 was wrong while a list entry could be seen before its row was marked assigned; the full
    sweep over all sizes is tools/stress_sweep.sh.)  The reference has no counterpart: its elimination is sequential
    (precode.c:115-203)."""
    import torch
    import nanorq_amd
    dev = torch.device("cuda", 0)
    ctx = nanorq_amd.Context(0, torch.cuda.current_stream(dev).cuda_stream)
    src = torch.randint(0, 256, (nblk, K, T), dtype=torch.uint8, device=dev, generator=torch.Generator(device=dev).manual_seed(K))
    for it in range(iters):
        lost = [loss_pattern(K, p, seed=7000 + it, block=b) for b in range(nblk)]
        ml = max(len(x) for x in lost)
        nrep = ml + 3
        esis = np.arange(K, K + nrep, dtype=np.uint32)
        rep = torch.empty((nblk, nrep, T), dtype=torch.uint8, device=dev)
        ctx.encode_blocks(K, T, nblk, src.data_ptr(), K * T, rep.data_ptr(), nrep * T, esis, 0, 0)
        work = src.clone()
        la = np.zeros((nblk, ml + 1), np.uint32)
        for b in range(nblk):
            la[b, :len(lost[b])] = lost[b]
            work[b, torch.from_numpy(lost[b].astype(np.int64)).to(dev)] = 0xEE
        nl = np.array([len(x) for x in lost], np.uint32)
        st, used = ctx.decode_blocks_lazy(K, T, nblk, work.data_ptr(), K * T, la, nl, np.tile(esis, (nblk, 1)), nl, nl + 3, rep.data_ptr(), nrep * T)
        torch.cuda.synchronize()
        st = np.asarray(st)
        assert st.all(), (K, it, int((st == 0).sum()))
        wrong = (~(work == src).flatten(1).all(1)).cpu().numpy()
        assert not wrong.any(), (K, it, np.nonzero(wrong)[0][:8])
        assert ctx.stats().get("host_planned", 0) == 0
    ctx.close()


STRESS_CASES = [  # K, T, blocks, loss, iterations -- the sizes every planner form covers (tools/stress_sweep.sh, same table)
    (8192, 64, 256, 0.1, 60), (8192, 64, 256, 0.3, 30), (9400, 32, 256, 0.1, 30), (2000, 32, 1024, 0.2, 40), (5000, 32, 512, 0.06, 40),
    (20000, 16, 64, 0.1, 15), (56403, 8, 8, 0.2, 10), (56403, 8, 8, 0.45, 6), (700, 32, 2048, 0.1, 30), (1000, 32, 2048, 0.5, 20),
    (100, 32, 8192, 0.2, 20), (10, 32, 8192, 0.3, 20),
    # 12-byte strips: T = whole strips / strips + 8 bytes / not a multiple of 4 (byte-wise movers)
    (11000, 36, 128, 0.2, 15), (10000, 44, 128, 0.06, 20), (9000, 50, 128, 0.1, 15)]


@pytest.mark.skipif(__import__("os").environ.get("NANORQ_STRESS") != "1", reason="long sweep: NANORQ_STRESS=1 enables it (~8 GPU-minutes)")
@pytest.mark.parametrize("K,T,nblk,p,iters", STRESS_CASES)
def test_stress_sweep(K, T, nblk, p, iters):
    """tools/stress_decode.py as a gated test (NANORQ_STRESS=1): ~0.5 M block decodes with fresh reception patterns over every
    form of the device planner -- none may fail, come out wrong, or need the host planner (a block the plan check of
    planner_body.h pl_check_* sends there counts as a defect of the peel, not as a pass)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "stress_decode.py"), str(K), str(T), str(nblk), str(p), str(iters)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-1500:]
    assert "done: %d iterations x %d blocks, 0 bad" % (iters, nblk) in out and "host planner took" not in out, out[-1500:]


def test_failure_rates_match_rfc6330_design():
    """10^5 random receptions of a K=100 block per overhead 0 / 1 / 2 (loss 10-50 %, random repair ESIs) through the device
    planner: RFC 6330's design figures are ~1 % / ~0.01 % / ~1e-4 % failures -- a mis-restated generator or a planner that
    loses rank lands far away from them.  Bounds are wide (Poisson: ~10 expected at overhead 1): 0.2-2 %, < 0.1 %, < 0.01 %.
    No block reported decoded may differ from its source.  (tools/failure_rates.py; the table for K = 100 and 1000 is
    profiles/r6_failure_rates.txt.)  Reference verdict: lib/nanorq.c:620-623, lib/precode.c:264-315."""
    import os
    import sys
    import torch
    import nanorq_amd
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import failure_rates
    dev = torch.device("cuda", 0)
    ctx = nanorq_amd.Context(0, torch.cuda.current_stream(dev).cuda_stream)
    r = failure_rates.rates(ctx, dev, 100, 8, 100000, [0.1, 0.3, 0.5])
    ctx.close()
    assert all(v["decoded_wrong"] == 0 for v in r.values()), r
    assert 0.002 < r[0]["rate"] < 0.02, r
    assert r[1]["rate"] < 0.001, r
    assert r[2]["rate"] < 0.0001, r


def test_single_small_blocks_through_the_host_planner_rule(G, orc):
    """What an unchanged caller of the reference API does: one block per call.  With the product's default ("host_plan_auto") such
    calls are planned on the host when the block is small and by the planner kernel otherwise; 80 random calls across the rule's
    boundary (K = 1 ... 2500, one or two blocks), every block back to its source or -- with too few symbols -- refused and untouched,
    and the verdict of a few of them against the reference algorithm."""
    c = G.ctx()
    rng = np.random.default_rng(90210)
    took = {0: 0, 1: 0}
    try:
        c.set_option("host_plan_auto", 1)
        for trial in range(80):
            K = int(rng.choice([1, 2, 10, 11, 55, 100, 101, 256, 500, 777, 1000, 1400, 1990, 2010, 2300, 2500]))
            T = int(rng.choice([1, 8, 16, 40, 64, 100]))
            nblk = int(rng.choice([1, 1, 1, 2]))
            p = float(rng.choice([0.05, 0.2, 0.5]))
            oh = int(rng.choice([0, 1, 2]))
            src = np.stack([payload(K * T, seed=trial, block=b).reshape(K, T) for b in range(nblk)])
            lost = [loss_pattern(K, p, seed=trial * 31, block=b) for b in range(nblk)]
            nrep = max(len(l) for l in lost) + oh
            esis = np.arange(K, K + nrep, dtype=np.uint32)
            rep, _ = G.gpu_encode(src, K, T, esis)
            work = src.copy()
            for b in range(nblk):
                work[b][lost[b]] = 0x11
            use = [len(l) + (oh if len(l) else 0) for l in lost]
            st, out, _ = G.gpu_decode(work, K, T, lost, [esis[:n] for n in use], [rep[b][:use[b]] for b in range(nblk)])
            took[c.stats()["planner"]] += 1
            for b in range(nblk):
                assert np.array_equal(out[b], src[b] if st[b] else work[b]), (K, T, nblk, p, oh, b)
            if trial % 6 == 0:
                rx = received_set(K, lost[0], oh if len(lost[0]) else 0)
                syms = np.concatenate([src[0][rx[rx < K]], rep[0][:use[0]]]) if use[0] else src[0][rx[rx < K]]
                ok, _, _ = orc.decode_block(rx, syms, K, T)
                assert bool(st[0]) == ok, (K, T, p, oh)
    finally:
        c.set_option("host_plan_auto", 0)
    assert took[0] > 20 and took[1] > 6, took   # both sides of the rule were exercised
