"""-m gpu tier: receptions that miss most or all of a block's source symbols, against the oracle's decode of the same symbols.

With more than 2 * qcap missing symbols the device planner lays their LT lists out in row order, offsets from a prefix scan
(planner_body.h pl_final_c2 .. pl_final_e: the "scan form"; else sorted by length from byte counters in the frontier queues).  qcap
goes with the planner instance plan_shape() picks: 2048 with 1024 threads, and for packed 256-thread workgroups 512 (L <= 1500) or
1024.  The sizes here are what tests/emu/shape_emu.cpp gives for the forced context (gpu_support.ctx(): plan_pack) on 256 compute
units: K = 1300 -> 256 threads, qcap 512; K = 2300 -> 256 threads, qcap 1024; K = 4200 and 5200 -> 1024 threads, qcap 2048; K = 100 ->
128 threads, qcap 256.  A plan says which form laid its lists out (nrq_plan_hdr scan_lists, written by the branch of pl_final_d that
ran); the call stats count such blocks (plan_scan_lists): here the counter must be non-zero exactly above 2 * qcap.

Every case compares verdict and bytes with the oracle (an undecodable block is left untouched), and asserts from the stats the planner
instance, the solve instance, the view the jobs ran on and the counter; host_planned == 0 keeps a silent capacity fallback from
standing in for the form under test.  tests/test_planner_emu.py runs the same receptions through the emulated planner at the
launched thread counts (u = 81 .. 166 inactive columns there: far below the planner's capacity).
GF arithmetic: everything byte for byte.  After a HIP error every later test of the file skips: nothing more is started on a device
that has just faulted."""
import numpy as np
import pytest

import nanorq_amd
import rx_support as R

pytestmark = pytest.mark.gpu

_BROKEN = []   # the test whose call returned an error from the HIP runtime: no further launch
LDS_MAX, LDS_GRANULE, NCU = 163840, 1280, 256   # launch_shape.h NRQ_LDS_MAX, NRQ_LDS_GRANULE; compute units of an MI355X
# K -> (planner threads, compact state, segmented, qcap) of the forced context, 3 blocks (see the head of the file)
PLAN = {100: (128, 0, 0, 256), 1300: (256, 0, 0, 512), 2300: (256, 0, 0, 1024), 4200: (1024, 0, 0, 2048), 5200: (1024, 0, 0, 2048)}
SEGMENTED = (1024, 1, 1, 2048)     # under plan_split_force: the full-size compact instance, in parts
BIG = (1024, 0, 0, 2048)           # the default context with at most a block per compute unit
# the rows of the edge: at 2 * qcap missing symbols the lists are still sorted by length, one more and the scan lays them out
ROWS = [(1300, (1024, 1025, 1300)), (2300, (2048, 2049, 2300)), (4200, (4096, 4097, 4200))]
RESET = {"max_wb": 16}             # option -> its default (every other one: 0)


@pytest.fixture(scope="module")
def G():
    import gpu_support
    gpu_support.ctx()
    return gpu_support


def _guard():
    if _BROKEN:
        pytest.skip("a call of %s returned a HIP error: no further launches" % (_BROKEN[0],))


_SRC = {}
_ORC = {}


def _blocks(orc, K, T, nblk):
    """per (K, T), once: nblk source blocks and the oracle's repair symbols of ESIs K .. 2 K + 1 (all missing, overhead 2)"""
    key = (K, T)
    if key not in _SRC or len(_SRC[key][0]) < nblk:
        src = np.stack([payload_of(K, T, b) for b in range(nblk)])
        esis = np.arange(K, 2 * K + 2, dtype=np.uint32)
        _SRC[key] = (src, esis, np.stack([orc.encode_block(src[b], K, T, esis)[0] for b in range(nblk)]))
    src, esis, rep = _SRC[key]
    return src[:nblk], esis, rep[:nblk]


def payload_of(K, T, b):
    from util import payload
    return payload(K * T, seed=K + 3, block=b).reshape(K, T)


def _lost(K, n, b):
    """exactly n missing source symbols of block b (all of them: n == K)"""
    if n == K:
        return np.arange(K, dtype=np.uint32)
    return np.sort(np.random.default_rng(100003 * K + 101 * n + b).permutation(K)[:n]).astype(np.uint32)


def _oracle(orc, K, T, b, src, rep, lost, oh):
    """the oracle's decode of block b's reception: surviving source symbols, then repair ESIs K .. K + len(lost) + oh - 1"""
    key = (K, T, b, lost.tobytes(), oh)
    if key not in _ORC:
        keep = np.setdiff1d(np.arange(K, dtype=np.uint32), lost)
        nr = len(lost) + oh if len(lost) else 0
        esis = np.concatenate([keep, np.arange(K, K + nr, dtype=np.uint32)])
        ok, out, _ = orc.decode_block(esis, np.concatenate([src[keep], rep[:nr]]), K, T, max_esi=4 * K)
        _ORC[key] = (bool(ok), out.copy())
    return _ORC[key]


def _solve_instance(s, K, T, nblk, forced):
    """(threads, waves per SIMD) solve_shape() gives a launch of stats s (launch_shape.h: single-wave workgroups where seven images
    fit a compute unit, 256-thread ones where two do, else the full-size one; 12-byte strips and a lone big block: the full-size one)"""
    alloc = -(-s["lds_bytes"] // LDS_GRANULE) * LDS_GRANULE
    wb = s["strip_bytes"]
    nstrips = -(-T // wb)
    lone = not forced and nblk * nstrips <= NCU and K >= 1200
    small = wb != 12 and 2 * alloc <= LDS_MAX and not lone
    tiny = small and 7 * alloc <= LDS_MAX and (forced or nblk * nstrips > 2 * NCU)
    return (64, 3) if tiny else (256, 4) if small else (768, 1)


def _run(G, orc, K, T, ns, oh, way="out", opts=None, kind="forced", host=False, plan=None, check=None, what=None):
    """One decode of len(ns) blocks, block b missing exactly ns[b] symbols, repair ESIs from K with overhead oh.  way: "out" (no
    intermediate symbols: the out view), "need" (the same under plan_no_out_view: the needed-pivot view), "inter" (with intermediate
    symbols, compared with the oracle's).  check: the blocks compared with the oracle (default all; the others with their source).
    Returns the call stats."""
    _guard()
    c = G.ctx(kind)
    nblk = len(ns)
    src, esis, rep = _blocks(orc, K, T, nblk)
    lost = [_lost(K, n, b) for b, n in enumerate(ns)]
    opts = dict(opts or {})
    if way == "need":
        opts["plan_no_out_view"] = 1
    work = src.copy()
    for b in range(nblk):
        work[b][lost[b]] = 0xEE
    try:
        try:
            for k, v in opts.items():
                c.set_option(k, v)
            if host:
                c.set_planner(False)
            st, out, inter = G.gpu_decode(work, K, T, lost, [esis[:len(l) + oh] if len(l) else esis[:0] for l in lost],
                                          [rep[b][:len(lost[b]) + oh] for b in range(nblk)], want_inter=(way == "inter"), kind=kind)
            s = c.stats()
        finally:
            for k in opts:
                c.set_option(k, RESET.get(k, 0))
            if host:
                c.set_planner(True)
    except nanorq_amd.NrqError:
        _BROKEN.append(what or (K, ns, oh, way, opts))
        raise
    what = (what or (K, tuple(ns) if nblk <= 8 else nblk, oh, way, opts, kind, "host" if host else "device"), s)
    print("high loss", what)
    # verdict and bytes
    ndec = nscan = 0
    threads, compact, seg, qcap = plan or PLAN[K]
    for b in range(nblk):
        if check is None or b in check:
            ok, ref = _oracle(orc, K, T, b, src[b], rep[b], lost[b], oh)
        else:
            ok, ref = True, src[b]   # (no case may pass with fewer decoded blocks than the oracle decodes: all of these at overhead 2)
        assert bool(st[b]) == ok, (what, "verdict of block", b, st)
        assert np.array_equal(out[b], ref if ok else work[b]), (what, "bytes of block", b)
        if ok and len(lost[b]):
            ndec += 1
            nscan += len(lost[b]) > 2 * qcap
            if way == "inter":
                key = ("inter", K, T, b)
                if key not in _ORC:
                    _ORC[key] = orc.encode_block(src[b], K, T, esis[:1], want_inter=True)[1]
                assert np.array_equal(inter[b], _ORC[key]), (what, "intermediate symbols of block", b)
    assert ndec >= 1, what
    # the planner instance and the form of the lists
    if host:
        assert (s["planner"], s["plan_wg_threads"], s["plan_compact_state"], s["plan_segmented"], s["plan_scan_lists"]) == (0, 0, 0, 0, 0), what
    else:
        assert (s["planner"], s["host_planned"]) == (1, 0), what
        assert (s["plan_wg_threads"], s["plan_compact_state"], s["plan_segmented"]) == (threads, compact, seg), what
        assert s["plan_scan_lists"] == nscan, (what, "blocks laid out by the scan", nscan)
    # the view the jobs ran on
    views = {"out": (ndec, 0), "need": (0, ndec), "inter": (0, 0)}[way]
    if host and way == "need":
        views = (ndec, 0)   # (the option is the device planner's: host-built plans bring their image all the same)
    assert (s["out_view"], s["need_view"]) == views, what
    assert (s["nneed"] > 0) == (views[1] > 0), what
    # the solve instance
    max_wb = opts.get("max_wb", 16)
    assert (s["strip_bytes"], s["strip_bytes_b"], s["blocks_b"]) == (max_wb, 0, 0), what
    assert (s["wg_threads"], s["wg_waves_per_simd"]) == _solve_instance(s, K, T, nblk, kind == "forced"), what
    assert (s["backsub_strip"] in (16, 32)) if max_wb <= 4 else s["backsub_strip"] == 0, what
    return s


# ---------------------------------------------------------------------------------------------------- the edge of the form ----
@pytest.mark.parametrize("oh", [2, 0])
@pytest.mark.parametrize("K,n", [(K, n) for K, ns in ROWS for n in ns])
def test_edge_of_the_scan_form(G, orc, K, n, oh):
    """exactly 2 * qcap, 2 * qcap + 1 and K missing symbols in each of three blocks: 2 * qcap must not count, one more must"""
    s = _run(G, orc, K, 16, [n] * 3, oh)
    assert (s["plan_scan_lists"] != 0) == (n > 2 * PLAN[K][3]), s


@pytest.mark.parametrize("oh", [2, 0])
@pytest.mark.parametrize("way", ["need", "inter"])
@pytest.mark.parametrize("K,n", [(K, n) for K, ns in ROWS for n in ns[1:]])
def test_scan_form_on_the_needed_pivot_view_and_with_intermediate_symbols(G, orc, K, n, way, oh):
    """the "+1" and "all" counts of each row without the out view (pl_final_e's marks through the scan's offsets, the back-substitution
    over the needed pivots) and with intermediate symbols (every pivot; compared with the oracle's)"""
    s = _run(G, orc, K, 16, [n] * 3, oh, way=way)
    assert s["plan_scan_lists"] == 3 or oh == 0, s   # (without overhead a block may be rank deficient: _run counted the decodable ones)


@pytest.mark.parametrize("oh", [2, 0])
def test_scan_form_of_a_segmented_run(G, orc, oh):
    """K = 4200, all missing, planned in parts: pl_final_c2 / c3 and pl_final_d run in part 2 on the restored state, the W' image is
    filled by nrq_wt_kernel from the lists the header names"""
    _run(G, orc, 4200, 16, [4200] * 3, oh, opts={"plan_split_force": 1}, plan=SEGMENTED)


@pytest.mark.parametrize("oh", [2, 0])
@pytest.mark.parametrize("K,n", [(K, n) for K, ns in ROWS for n in ns])
def test_host_planner_on_the_same_receptions(G, orc, K, n, oh):
    """the reference the device plans must agree with: the same receptions planned on the host (lists by out_lists.h)"""
    _run(G, orc, K, 16, [n] * 3, oh, host=True)


@pytest.mark.parametrize("oh", [2, 0])
@pytest.mark.parametrize("max_wb", [12, 8, 4])
@pytest.mark.parametrize("K", [1300, 4200])
def test_strip_widths_on_lists_in_row_order(G, orc, K, max_wb, oh):
    """all missing at 12- and 8-byte strips (the device-only t4_word bodies of ph_store on lists in row order) and at 4-byte strips
    (the split solve: nrq_backsub_kernel over every pivot, nrq_collect_kernel writes K rows per block)"""
    T = 32 if max_wb == 12 else 16   # (12-byte strips: a whole strip, then one of 8 bytes)
    _run(G, orc, K, T, [K] * 3, oh, opts={"max_wb": max_wb})


# ------------------------------------------------------------------------------------------------ the store phase's passes ----
@pytest.mark.parametrize("oh", [2, 0])
@pytest.mark.parametrize("K,threads", [(100, 64), (1300, 256), (5200, 768)])
def test_store_phase_at_a_list_per_source_symbol(G, orc, K, threads, oh):
    """whole-block loss: K lists per block through ph_store, 100 on 64 threads, 1300 on 256, 5200 on 768 (seven passes)"""
    s = _run(G, orc, K, 32, [K] * 3, oh)
    assert s["wg_threads"] == threads, s


@pytest.mark.parametrize("oh", [2, 0])
def test_lost_block_beside_a_near_complete_and_a_complete_one(G, orc, oh):
    """one call: a wholly lost block (scan form), a block missing one symbol (sorted form), a complete block (no job)"""
    s = _run(G, orc, 1300, 16, [1300, 1, 0], oh)
    assert s["plan_scan_lists"] == 1 or oh == 0, s


# ------------------------------------------------------------------------------------------------------ the default context ----
def test_default_context_more_blocks_than_compute_units(G, orc):
    """260 blocks of K = 1300, each missing 1100 .. 1300 symbols: more blocks than compute units, the only way a product caller gets
    the 256-thread planner (qcap 512: every block above the edge).  First, middle and last block against the oracle, the rest against
    their source."""
    ns = [1100 + (37 * b) % 201 for b in range(260)]
    ns[0], ns[130], ns[259] = 1300, 1187, 1300
    s = _run(G, orc, 1300, 16, ns, 2, kind="default", check=(0, 130, 259), what="260 blocks")
    assert s["plan_scan_lists"] == 260, s


@pytest.mark.parametrize("oh", [2, 0])
def test_default_context_whole_block_loss_of_big_blocks(G, orc, oh):
    """3 blocks of K = 4200, all missing: the 1024-thread planner a batch of at most a block per compute unit gets"""
    _run(G, orc, 4200, 16, [4200] * 3, oh, kind="default", plan=BIG)


# --------------------------------------------------------------------------------------------------------- the resident layer ----
def _np(t):
    return t.cpu().numpy().view(np.uint32)


def test_receptions_fed_repair_packets_only(G, orc):
    """A Receiver of two blocks of K = 1300 that never sees a source packet, and an ObjectReceiver whose first block does not: counts,
    lists, want in source and in repair mode, decode (the scan form on the 256-thread planner), the recovered rows."""
    _guard()
    import torch
    c = G.ctx()
    K, T, nblk, cap = 1300, 16, 2, 1300 + 8
    src, esis, rep = _blocks(orc, K, T, 3)
    for b in range(nblk):
        ok, ref = _oracle(orc, K, T, b, src[b], rep[b], np.arange(K, dtype=np.uint32), 2)
        assert ok and np.array_equal(ref, src[b])
    tags_of = lambda es: np.array([R.tag(b, e) for b in range(nblk) for e in es], np.uint32)

    def dev(a):
        t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        torch.cuda.synchronize()   # (torch's stream and the library's are not ordered)
        return t

    try:
        with nanorq_amd.Receiver(c, K, T, nblk, cap, max_esi=4 * K) as rx:
            def feed(lo, hi):   # repair ESIs K + lo .. K + hi - 1 of both blocks, interleaved by block
                t = np.array([R.tag(b, K + i) for i in range(lo, hi) for b in range(nblk)], np.uint32)
                rx.add(dev(np.stack([rep[b][i] for i in range(lo, hi) for b in range(nblk)])), tags=dev(t.view(np.int32)))

            feed(0, K - 3)
            nl, nr = rx.counts()
            assert nl.tolist() == [K] * nblk and nr.tolist() == [K - 3] * nblk
            lost, reps = rx.lists()
            for b in range(nblk):
                assert np.array_equal(lost[b], np.arange(K)) and np.array_equal(reps[b], np.arange(K, 2 * K - 3))
            assert np.array_equal(_np(rx.want(source=True)), tags_of(range(K)))            # source mode: all K tags per block
            assert np.array_equal(_np(rx.want()), tags_of(range(2 * K - 3, 2 * K)))         # repair mode: the three it lacks
            assert np.array_equal(_np(rx.want(extra=2)), tags_of(range(2 * K - 3, 2 * K + 2)))
            feed(K - 3, K + 2)
            nl, nr = rx.counts()
            assert nl.tolist() == [K] * nblk and nr.tolist() == [K + 2] * nblk
            assert rx.want().numel() == 0
            assert np.array_equal(_np(rx.want(extra=4)), tags_of(range(2 * K + 2, 2 * K + 4)))
            st, used = rx.decode()
            s = c.stats()
            print("high loss resident", s, used)
            assert st.tolist() == [1] * nblk and (used >= K).all() and (used <= K + 2).all()
            assert (s["planner"], s["host_planned"], s["plan_wg_threads"], s["plan_scan_lists"], s["out_view"]) == (1, 0, 256, nblk, nblk), s
            c.sync()
            torch.cuda.synchronize()
            assert np.array_equal(rx.source.cpu().numpy(), src[:nblk])
            assert rx.counts()[0].tolist() == [0] * nblk and rx.want(source=True).numel() == 0 and rx.want(extra=4).numel() == 0
        # the object: block 0 gets no source packet, block 1 all but one and three repair packets
        with nanorq_amd.ObjectSender(c, dev(src[:nblk].reshape(-1)), T, Z=nblk) as tx:
            assert tx.blocks == [(K, nanorq_amd.params(K)["Kp"])] * nblk
            tx.encode()
            t_o = torch.zeros(tx.count_all(K + 2), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            sent = tx.emit_all(K + 2, interleave=True, inline=True, tags_out=t_o)
            c.sync()
            tags, oti = _np(t_o), tx.oti
            sbn, esi = tags >> 24, tags & 0xFFFFFF
            got = np.where(sbn == 0, esi >= K, (esi != 5) & (esi < K + 3))
            pk = sent[dev(np.flatnonzero(got))].contiguous()
            torch.cuda.synchronize()
        with nanorq_amd.ObjectReceiver(c, *oti, rep_cap=cap) as orx:
            orx.add(pk, inline=True)
            nl, nr = orx.counts()
            assert nl.tolist() == [K, 1] and nr.tolist() == [K + 2, 3]
            assert np.array_equal(_np(orx.want(source=True)), np.array([R.tag(0, e) for e in range(K)] + [R.tag(1, 5)], np.uint32))
            assert orx.want().numel() == 0
            assert np.array_equal(_np(orx.want(extra=3)), np.array([R.tag(0, 2 * K + 2), R.tag(1, K + 3)], np.uint32))
            st, used = orx.decode()
            s = c.stats()
            print("high loss object", s, used)
            assert st.tolist() == [1, 1]
            assert (s["planner"], s["host_planned"], s["plan_wg_threads"], s["plan_scan_lists"]) == (1, 0, 256, 1), s
            obj, left = orx.write()
            c.sync()
            torch.cuda.synchronize()
            assert left == 0 and np.array_equal(obj.cpu().numpy(), src[:nblk].reshape(-1))
            assert orx.counts()[0].tolist() == [0, 0] and orx.want(source=True).numel() == 0
    except nanorq_amd.NrqError:
        _BROKEN.append("the resident layer")
        raise
