"""CPU tier: host plans at a forced number of inactive columns (nanorq_amd.host_plan(..., extra_inact=n); the context option
"plan_force_inact"; tests/forced_inact_support.py).

The solve kernel picks its back-substitution by the plan's W-row width wpr = ceil(u / 32): four unrolled classes and a plain loop,
each in a form for big and one for small workgroups, and for 16-, 12- and 8-byte strips with a body that exists on the device only.
Nothing but the hook chooses u.  Here, without a GPU: the hook switched off changes no plan; a forced plan is a correct plan of the
same system -- the oracle's reference executor over it gives the oracle's intermediate symbols, the verdict is the oracle's, also
with every column of V inactive (no pivot at all) and for a rank-deficient reception; the generic code of the kernel (the CPU
emulation runs the lines under the device-only bodies) solves the same plans at every strip width, beyond 24 words too; whatever
solve_shape picks for a forced plan fits the LDS; and every row of the GPU case table is what the host planner and solve_shape
give.  The fenced launch emulation of the same cases: tests/test_launch_bounds_emu.py, groups forced_*."""
import numpy as np
import pytest

import nanorq_amd
import forced_inact_support as F
from emu_support import ROW_ZERO, emu_solve, lt_lists
from util import loss_pattern, payload, received_set, undecodable

# the receptions of test_planner_emu.py::test_decode_emulated_matches_oracle: (K, loss, overhead), seeds 1 .. 3 each
PLANNER_TABLE = [(10, 0.3, 0), (100, 0.06, 0), (100, 0.06, 2), (100, 0.5, 30), (1024, 0.05, 0), (1024, 0.06, 52), (8192, 0.1, 0),
                 (8192, 0.1, 2), (1024, 0.05, 0), (100, 0.3, 3)]
KS = (10, 100, 1000, 3000)
T = 20   # strips of 16 + 4, 12 + 8, 8 + 8 + 4 bytes, five of 4, ten of 2


@pytest.mark.parametrize("K,loss,oh", PLANNER_TABLE)
def test_hook_off_is_byte_identical(orc, K, loss, oh):
    kc = F.kconst(K)
    for seed in range(1, 4):
        lost = loss_pattern(K, loss, seed)
        rep_esis = received_set(K, lost, oh)
        rep_esis = rep_esis[rep_esis >= K]
        isis = F.decode_setup(orc, K, lost, rep_esis)[0]
        assert nanorq_amd.host_plan(K, isis, kc, extra_inact=0) == nanorq_amd.host_plan(K, isis, kc)
    isis = F.encode_isis(K)
    assert nanorq_amd.host_plan(K, isis, kc, extra_inact=0) == nanorq_amd.host_plan(K, isis, kc)


def _systems(orc, K):
    """(name, isis, rowsrc, lost, repair ESIs) of the encode and of four receptions"""
    p = orc.params(K)
    rowsrc = np.full(p["L"], ROW_ZERO, np.uint32)
    rowsrc[p["S"] + p["H"]:p["S"] + p["H"] + K] = np.arange(K, dtype=np.uint32)
    out = [("encode", F.encode_isis(K), rowsrc, np.zeros(0, np.uint32), np.zeros(0, np.uint32))]
    for loss in (0.1, 0.3):
        for oh in (0, 2):
            lost, esis, isis, rs = F.reception(orc, K, loss, oh, seed=int(loss * 100) + oh + K)
            out.append(("decode %g +%d" % (loss, oh), isis, rs, lost, esis))
    return out


def _ns_by_wpr(K, isis):
    """{wpr: n} for the widths of F.WPRS this system can have: from its own width without the hook up to ceil(L / 32).  n is taken
    from the bound u >= P + n and corrected by what the peel still inactivates."""
    p = nanorq_amd.params(K)
    lo, hi = F.header(K, isis)["wpr"], F.wpr_of(p["L"])
    out = {}
    for wpr in F.WPRS:
        if wpr < lo or wpr > hi:
            continue
        if wpr == lo:
            out[wpr] = 0
            continue
        goal = min(32 * wpr - 6, p["L"])
        n = max(0, goal - p["P"])
        for _ in range(6):
            u = F.header(K, isis, n)["u"]
            if F.wpr_of(u) == wpr:
                out[wpr] = n
                break
            n = max(0, n - (u - goal)) if u > goal else n + 4
    return out


@pytest.fixture(scope="module")
def forced_plans(orc):
    """every (K, system, wpr) plan of this file, built once: {K: [(name, wpr, n, plan, rowsrc, lost, esis)]}, with the oracle's block"""
    plans, ref, widths = {}, {}, {}
    for K in KS:
        src = payload(K * T, seed=K).reshape(K, T)
        ref[K] = (src, orc.encode_block(src, K, T, [], want_inter=True)[1])
        plans[K] = []
        for name, isis, rowsrc, lost, esis in _systems(orc, K):
            ns = _ns_by_wpr(K, isis)
            lo, hi = F.header(K, isis)["wpr"], F.wpr_of(nanorq_amd.params(K)["L"])
            assert sorted(ns) == [w for w in F.WPRS if lo <= w <= hi], (K, name, ns)   # (no class the block can have is left out)
            widths.setdefault(K, {})[name] = set(ns)
            for wpr, n in ns.items():
                plans[K].append((name, wpr, n, isis, F.plan(K, isis, n), rowsrc, lost, esis))
    # K = 10 and 100 begin at one word, K = 1000 at three, K = 3000 at four; K = 1000 ends at 34 words, K = 3000 has all ten
    assert [sorted(set().union(*widths[K].values())) for K in KS] == [[1], [1, 4], [4, 5, 8, 9, 12, 13, 24, 25], [4, 5, 8, 9, 12, 13, 24, 25, 40]]
    return plans, ref, widths


@pytest.mark.parametrize("K", KS)
def test_forced_plans_are_correct_plans(orc, forced_plans, K):
    """the reference executor (oracle/plan_exec_ref.c: whole rows, plain loops) over every forced plan: the oracle's intermediate
    symbols and the recovered block, byte for byte; the verdict is orc.plan_probe's; u >= P + n; wpr = ceil(u / 32)"""
    plans, ref, widths = forced_plans
    src, inter = ref[K]
    p = orc.params(K)
    seen = set()
    for name, wpr, n, isis, plan, rowsrc, lost, esis in plans[K]:
        h = nanorq_amd.plan_header(plan)
        ok = orc.plan_probe(K, isis)[0] == 1
        assert (h["status"] == 0) == ok, (K, name, n)
        assert h["u"] >= p["P"] + min(n, p["W"]) and h["wpr"] == F.wpr_of(h["u"]) == wpr and h["npiv"] + h["u"] == p["L"], (K, name, n, h["u"])
        assert h["nfree"] == F.header(K, isis)["nfree"], (K, name, n)
        if not ok:
            continue
        rep = orc.encode_block(src, K, T, esis)[0]
        r, C_ = orc.plan_exec(plan, F.exec_rows(plan, rowsrc, src, rep, T), T)
        assert r == 1 and np.array_equal(C_, inter), (K, name, n, "intermediate symbols")
        if len(lost):
            rx = received_set(K, lost, len(esis) - len(lost))
            ok2, out, _ = orc.decode_block(rx, np.concatenate([src[rx[rx < K]], rep]), K, T)
            assert ok2 and np.array_equal(F.source_from_inter(orc, K, C_, lost), out[lost]), (K, name, n, "recovered block")
        seen.add(wpr)
    assert seen == set().union(*widths[K].values()), seen


@pytest.mark.parametrize("wb", [16, 12, 8, 4, 2])
@pytest.mark.parametrize("K", KS)
def test_generic_backsub_solves_the_forced_plans(orc, forced_plans, K, wb):
    """emu_solve -- the kernel's phase code with the generic lines under the device-only bodies of backsub_one -- over the same plans
    at every strip width: every class of ph_backsub and its plain loop (wpr 25 and 40 at K = 1000 / 3000)"""
    plans, ref, widths = forced_plans
    src, inter = ref[K]
    L = orc.params(K)["L"]
    done = set()
    for name, wpr, n, isis, plan, rowsrc, lost, esis in plans[K]:
        if nanorq_amd.plan_header(plan)["status"] or name not in ("encode", "decode 0.1 +2", "decode 0.3 +0"):
            continue
        if name == "encode":
            out_isis = np.arange(K, K + 3, dtype=np.uint32) + (orc.params(K)["Kp"] - K)
            want = orc.encode_block(src, K, T, np.arange(K, K + 3, dtype=np.uint32))[0]
            out = np.zeros((3, T), np.uint8)
            r, got = emu_solve(plan, F.kconst(K), rowsrc, src, None, T, L, lt_lists(orc, K, out_isis, plan), np.arange(3), out, wb)
            assert r == 1 and np.array_equal(out, want), (K, name, wpr, "repair symbols")
        else:
            rep = orc.encode_block(src, K, T, esis)[0]
            work = src.copy()
            work[lost] = 0xEE
            r, got = emu_solve(plan, F.kconst(K), rowsrc, work, rep, T, L, lt_lists(orc, K, lost, plan), lost, work, wb)
            assert r == 1 and np.array_equal(work, src), (K, name, wpr, "recovered block")
        assert np.array_equal(got, inter), (K, name, wpr, "intermediate symbols")
        done.add(wpr)
    assert done == set().union(*widths[K].values()), done


@pytest.mark.parametrize("wb", [16, 12, 8, 4, 2])
def test_every_column_inactive_leaves_no_pivot(orc, wb):
    """K = 10 with all of V inactive from the start: npiv == 0, the peel, the op stream's level groups, ph_tables' last group and both
    back-substitution loops run zero times; the dense stage solves the whole system"""
    K = 10
    p = orc.params(K)
    src = payload(K * T, seed=4).reshape(K, T)
    inter = orc.encode_block(src, K, T, [], want_inter=True)[1]
    for name, isis, rowsrc, lost, esis in _systems(orc, K):
        for n in (p["W"], p["W"] + 9):   # (more than there are: all of them)
            plan = F.plan(K, isis, n)
            h = nanorq_amd.plan_header(plan)
            ok = orc.plan_probe(K, isis)[0] == 1
            assert (h["status"] == 0) == ok and h["npiv"] == 0 and h["u"] == p["L"] and h["nlev"] == 0, (name, h)
            if not ok:
                continue
            rep = orc.encode_block(src, K, T, esis)[0] if len(esis) else None
            r, C_ = orc.plan_exec(plan, F.exec_rows(plan, rowsrc, src, rep, T), T)
            assert r == 1 and np.array_equal(C_, inter), name
            work = src.copy()
            work[lost] = 0xEE
            r, got = emu_solve(plan, F.kconst(K), rowsrc, work, rep, T, p["L"], lt_lists(orc, K, lost, plan), lost, work, wb)
            assert r == 1 and np.array_equal(got, inter) and np.array_equal(work, src), name


@pytest.mark.parametrize("K", [10, 100, 1000])
def test_rank_deficient_reception_stays_refused(orc, K):
    """a reception whose system has rank < L (util.undecodable) is refused at every n: inactivating columns moves no rank"""
    p = orc.params(K)
    lost = undecodable(orc, K, 0)
    isis = F.decode_setup(orc, K, lost, np.arange(K, K + len(lost), dtype=np.uint32))[0]
    assert orc.plan_probe(K, isis)[0] == 0
    ns = sorted(set(list(range(0, 40)) + list(range(0, p["W"] + 1, max(1, p["W"] // 37))) + [p["W"] - 1, p["W"], p["W"] + 1]))
    for n in ns:
        h = F.header(K, isis, n)
        assert h["status"] == 1, (K, n)


def test_what_solve_shape_picks_for_a_forced_plan_fits_the_lds(orc, forced_plans):
    """the forced plans' headers through solve_lists / solve_shape, on the forced context's options and at every width cap: the
    dynamic LDS of the launch is within NRQ_LDS_MAX, and a split launch's tables are too -- or the shape is refused"""
    plans, _, _ = forced_plans
    for K in KS:
        L = orc.params(K)["L"]
        for name, wpr, n, isis, plan, rowsrc, lost, esis in plans[K]:
            if nanorq_amd.plan_header(plan)["status"]:
                continue
            for cap in (16, 12, 8, 4, 2):
                for ctx in ({}, F.GPU_FORCED, {"big_wg": 1}):
                    dec = name != "encode"
                    rec = F.launch_record([plan] * (F.NBLK if dec else 1), dict(ctx, max_wb=cap), F.NBLK, 48, L + len(lost) + 4, True, dec)
                    assert rec["err"] == 0 and 0 < rec["lds_bytes"] <= F.NRQ_LDS_MAX, (K, name, wpr, cap, rec)
                    assert rec["wb"] <= cap and (rec["backsub_strip"] != 0) == (rec["wb"] <= 4), rec
                    if rec["split"]:
                        assert nanorq_amd.plan_header(plan)["wpr"] * 8 * 16 * rec["backsub_strip"] <= F.NRQ_LDS_MAX, rec


def test_more_than_1280_inactive_columns(orc):
    """The host planner has no cap on u (1280 = 40 W words is the DEVICE planner's capacity).  Beyond it everything downstream is
    sized by the header: the strip image by nrq_lds_plan (solve_lists moves to the width that fits, or refuses the block), the
    split solve's tables by wpr (sp_words goes round its batches of 20 words).  So: K = 3000 at 41 words and with all 3135 columns
    inactive (98 words) solves in the emulation; the launch of the 98-word plan is a 4-byte split whose tables (98 * 2 KiB) exceed
    the LDS -- solve_shape answers SHAPE_BACKSUB_TABLES (launch_solve turns that into a status before anything is launched); capped
    at 2 bytes it is the same; and without the split it is a plain 4-byte launch within the LDS."""
    K = 3000
    p = orc.params(K)
    src = payload(K * T, seed=K).reshape(K, T)
    inter = orc.encode_block(src, K, T, [], want_inter=True)[1]
    lost, esis, isis, rowsrc = F.reception(orc, K, 0.1, 2)
    rep = orc.encode_block(src, K, T, esis)[0]
    for n, u, wb in ((1195, 1281, 16), (1195, 1281, 4), (p["W"], p["L"], 8), (p["W"], p["L"], 2)):
        plan = F.plan(K, isis, n)
        h = nanorq_amd.plan_header(plan)
        assert (h["status"], h["u"], h["wpr"]) == (0, u, F.wpr_of(u)), h
        r, C_ = orc.plan_exec(plan, F.exec_rows(plan, rowsrc, src, rep, T), T)
        assert r == 1 and np.array_equal(C_, inter)
        work = src.copy()
        work[lost] = 0xEE
        r, got = emu_solve(plan, F.kconst(K), rowsrc, work, rep, T, p["L"], lt_lists(orc, K, lost, plan), lost, work, wb)
        assert r == 1 and np.array_equal(got, inter) and np.array_equal(work, src), (n, wb)
    plan = F.plan(K, isis, p["W"])
    SHAPE_BACKSUB_TABLES = 3   # launch_shape.h ShapeErr
    for opts in ({}, {"max_wb": 2}):
        rec = F.launch_record([plan] * 2, opts, 2, 48, p["L"], True, True)
        assert rec["err"] == SHAPE_BACKSUB_TABLES, rec
    rec = F.launch_record([plan] * 2, {"no_split": 1}, 2, 48, p["L"], True, True)
    assert rec["err"] == 0 and rec["wb"] == 4 and rec["split"] == 0 and rec["lds_bytes"] <= F.NRQ_LDS_MAX, rec


@pytest.fixture(scope="module")
def case_plans(orc):
    out = {}
    for form, u, n_enc, n_dec, strip, threads, sb in F.GPU_CASES:
        K = F.FORMS[form]["K"]
        out[(form, u)] = (F.header(K, F.encode_isis(K), n_enc), F.header(K, F.gpu_reception(orc, K)[2], n_dec))
    return out


def test_gpu_case_table_is_what_planner_and_shape_give(orc, case_plans):
    """every row of F.GPU_CASES: the host planner at the row's n ends at the row's u (encode plan and decode plan), the decode is
    solvable, and each of the case's three calls gets the row's (strip_bytes, wg_threads, backsub_strip) from solve_shape -- the
    record the GPU test asserts from the call stats"""
    assert len({(c[0], c[1]) for c in F.GPU_CASES}) == len(F.GPU_CASES)
    for i, (form, u, n_enc, n_dec, strip, threads, sb) in enumerate(F.GPU_CASES):
        he, hd = case_plans[(form, u)]
        assert (he["status"], he["u"], hd["status"], hd["u"]) == (0, u, 0, u), (form, u, he["u"], hd["u"])
        for call in F.calls_of(i):
            rec = F.case_record(orc, form, n_enc, n_dec, *call)
            assert rec[:3] == (strip, threads, sb) and rec[3] <= F.NRQ_LDS_MAX, (form, u, call, rec)


def test_gpu_case_table_reaches_every_form():
    """(strip bytes, threads) x class of ph_backsub (0: the plain loop) that the cases run, against the list the issue of these tests
    set out to reach; and per class boundary u % 32 in {31, 0, 1}.  What no context reaches: see tests/test_gpu_backsub_forms.py."""
    reached = {}
    for form, u, n_enc, n_dec, strip, threads, sb in F.GPU_CASES:
        reached.setdefault((strip, threads), set()).add(F.nw_class(F.wpr_of(u)))
    assert reached[(16, 768)] >= {8, 12, 24, 0}
    assert reached[(16, 256)] >= {4, 8, 12, 24}
    assert reached[(16, 64)] == {4}
    assert reached[(12, 768)] >= {8, 12, 24, 0}
    assert reached[(8, 768)] >= {8, 12, 24, 0}
    assert reached[(8, 256)] >= {12, 24, 0} and reached[(8, 64)] >= {4, 8, 12}
    for b in (4, 8, 12, 24):
        for r in (31, 0, 1):
            assert any(u == 32 * b + (r if r < 31 else -1) for _, u, *_ in F.GPU_CASES), (b, r)
    split = {(strip, sb, F.wpr_of(u)) for _, u, _, _, strip, _, sb in F.GPU_CASES if sb}
    assert split >= {(4, 32, 20), (4, 16, 21), (4, 16, 40), (4, 16, 41), (2, 32, 20), (2, 16, 21), (2, 16, 40), (2, 16, 41)}
    npivs = {128 - u for form, u, *_ in F.GPU_CASES if form == "w16_k100"}
    assert npivs >= {0, 1, 63, 64, 65}   # (K = 100: L = 128; backsub_fixed's two register sets against a workgroup of 64)
