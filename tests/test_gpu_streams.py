"""-m gpu tier: the library on a caller's SIDE stream, and two contexts at once.

Every other GPU test runs the library on the legacy null stream, where torch's kernels, the library's kernels and anything the
library puts on stream 0 by mistake are ordered by accident.  Here the context lives on a torch.cuda.Stream() of its own
(gpu_support.ctx("side")) and every case is DELAY-FENCED: a bounded stretch of ordinary torch work (passes over a 256 MB tensor)
goes on the stream first, then a torch op on that stream writes the real inputs over poison, then the library call, then a
torch op that copies the outputs (pre-filled with a second poison) aside -- one host wait at the end, then the copies are
compared with the CPU oracle byte for byte.  A library read that ran ahead of the fence computes from poison; a library write
that ran on another stream is not in the copy.  A case asserts right after its library call that the event recorded behind the
fence has NOT completed: a fence that was too short fails the case, it never lets it pass quietly.  (Calls that wait for the
context's stream by contract -- decode of a reception, counts, want, attach -- come after that assertion.)

The fence is calibrated once per module (fixture F): 20 times the measured host time of the slowest enqueue-only call of the
file (warmed), at least 30 ms, and the calibration fails above 50 ms.  docs/LAB_NOTES.md has the measured numbers.

Kernel families each case runs on the side stream (no variant is new; tests/variant_ledger.py lists them all):
  test_codec_on_the_side_stream      solve (64-, 256-, 768-thread workgroups), gen (repair rows of an encode), planner
                                     (device: plan / wt kernels on the context's planner streams; host plan upload: ctl_copy)
  test_gen_symbols / test_row_movers gen; scatter, move_rows, the copy engine (nrq_dev_copy)
  test_sender_receiver_relay         solve, tx emit (range and list), ingest (first/done/hist/scan/classify/copy/fold), lists,
                                     mark, planner
  test_want_emit_add                 ingest, want count/fill, tx hist/scan/place + emit, lists, solve
  test_packets_of_several_symbols    emit syms (range), ingest syms, solve
  test_object_round_trip             obj layout, emit (three segments), orx ingest + foreign, solve, layout back (write)
  test_sets                          txs hist/scan/place + set emit, ings ingest, set lists / counts / want / mark, solve
  test_set_table_is_not_replaced...  ings ingest against the member table (the blocking table upload on stream 0)
  test_set_stream_moves_the_context  solve, planner on both streams
  test_binding_owned_*               want/held (+ runs), emit, emit syms, layout (write), set listings
  test_two_contexts_*                solve, planner (1024-thread, segmented encode-plan build), emit, ingest
"""
import concurrent.futures as cf
import ctypes as C
import functools
import time

import numpy as np
import pytest

import nanorq_amd
from rx_support import ModelRx
from syms_support import range_list
from util import loss_pattern, payload
from want_support import model_books, model_want

pytestmark = pytest.mark.gpu

P_IN, P_OUT = 0x5A, 0xC3      # inputs before the torch op that writes them; outputs before the library writes them
STEP_TIMEOUT = 120            # seconds a step of the two-context cases may take before the case fails
FENCE_MIN_MS, FENCE_MAX_MS = 30.0, 50.0
WARM = 4                      # unfenced runs of a case before the fenced one (see `twice`)
NOTES = {}                    # what the calibration measured (printed by the last test: pytest -s shows it)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available()
    return t


@pytest.fixture(scope="module")
def side(torch):
    """(context, its torch stream)"""
    import gpu_support as G
    return G.ctx("side"), G.side_stream()


@pytest.fixture(autouse=True)
def stop_on_a_device_error(torch):
    """a device error ends the session: nothing more is started on a GPU that has reported one"""
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:   # noqa: BLE001 (whatever the runtime raises)
        pytest.exit("the device reported an error behind this test: %s" % e, returncode=3)


# ----------------------------------------------------------------------------------------------------- references ----
_REF = {}


def ref(orc, K, T, nblk, seed=1, loss=0.1, oh=2, decode=True):
    """One reference per shape, computed once and never changed: the source blocks, the oracle's intermediate and repair symbols
    (ESIs K .. K + nrep - 1), a reception per block (lost source ESIs, the first len(lost) + oh repair symbols) and the oracle's
    verdict and bytes on exactly that reception (decode=False: an encode-only reference)."""
    key = (K, T, nblk, seed, loss, oh, decode)
    if key in _REF:
        return _REF[key]
    src = np.stack([payload(K * T, seed=seed, block=b).reshape(K, T) for b in range(nblk)])
    lost = [loss_pattern(K, loss, seed=seed + 1, block=b) for b in range(nblk)]
    use = [len(x) + oh for x in lost]
    nrep = max(use)
    esis = np.arange(K, K + nrep, dtype=np.uint32)
    rep, inter = [], []
    for b in range(nblk):
        r, i, _ = orc.encode_block(src[b], K, T, esis, want_inter=True)
        rep.append(r), inter.append(i)
    work = src.copy()
    ok, out = [], []
    for b in range(nblk if decode else 0):
        work[b][lost[b]] = 0x3C
        keep = np.setdiff1d(np.arange(K, dtype=np.uint32), lost[b])
        o, r_out, _ = orc.decode_block(np.concatenate([keep, esis[:use[b]]]), np.concatenate([src[b][keep], rep[b][:use[b]]]), K, T)
        ok.append(bool(o)), out.append(r_out if o else work[b])
    r = dict(K=K, T=T, nblk=nblk, src=src, lost=lost, use=use, nrep=nrep, esis=esis, rep=np.stack(rep), inter=np.stack(inter), work=work,
             ok=np.array(ok), out=np.stack(out) if decode else None, L=nanorq_amd.params(K)["L"])
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _REF[key] = r
    return r


def dev(torch, a):
    """a numpy array as a device tensor (uint32 as int32), on torch's current stream; the host has waited for the copy"""
    a = np.ascontiguousarray(a)
    a = a if a.flags.writeable else a.copy()
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def host(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


def poison(torch, shape, value, dtype=None):
    return torch.full(tuple(int(x) for x in np.atleast_1d(shape)), value, dtype=dtype or torch.uint8, device="cuda")


# ---------------------------------------------------------------------------------------------------------- fence ----
class Fence:
    """passes over a 256 MB tensor on one stream; put() returns the event recorded behind them"""

    on = True     # False: put() enqueues nothing (the unfenced first run of a case, see `twice`)

    def __init__(self, torch, side, orc):
        self.torch = torch
        c, s = side
        self.buf = torch.zeros(64 << 20, dtype=torch.int32, device="cuda")
        with torch.cuda.stream(s):
            for _ in range(3):
                self.buf.add_(1)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            for _ in range(20):
                self.buf.add_(1)
            b.record(s)
        s.synchronize()
        self.pass_ms = a.elapsed_time(b) / 20
        slow, name = _slowest_enqueue_ms(torch, c, s, orc)
        self.ms = max(20.0 * slow, FENCE_MIN_MS)
        assert self.ms <= FENCE_MAX_MS, "the slowest enqueue-only call (%s) took %.2f ms on the host: a fence of 20 times that passes %g ms" % (
            name, slow, FENCE_MAX_MS)
        self.passes = int(np.ceil(self.ms / self.pass_ms))
        NOTES.update(pass_ms=self.pass_ms, slowest_enqueue_ms=slow, slowest_enqueue=name, fence_ms=self.ms, passes=self.passes)

    def put(self, stream):
        if not self.on:
            return None
        with self.torch.cuda.stream(stream):
            for _ in range(self.passes):
                self.buf.add_(1)
            ev = self.torch.cuda.Event()
            ev.record(stream)
        return ev

    @staticmethod
    def pending(ev, what):
        assert ev is None or not ev.query(), "the fence had passed when %s returned: the case proved nothing" % what


def _slowest_enqueue_ms(torch, c, s, orc):
    """host time of the file's enqueue-only calls at their largest shapes, each run once before it is timed"""
    times = {}

    def timed(name, fn):
        fn()
        c.sync()
        t0 = time.perf_counter()
        fn()
        times[name] = (time.perf_counter() - t0) * 1e3
        c.sync()

    with torch.cuda.stream(s):
        for K, T, nblk in SHAPES:
            r = ref(orc, K, T, nblk)
            src, rep, inter = dev(torch, r["src"]), poison(torch, (nblk, r["nrep"], T), P_OUT), poison(torch, (nblk, r["L"], T), P_OUT)
            timed("encode_blocks K=%d" % K, lambda: c.encode_blocks(K, T, nblk, src.data_ptr(), K * T, rep.data_ptr(), r["nrep"] * T, r["esis"],
                                                                    inter.data_ptr(), r["L"] * T))
            timed("gen_symbols K=%d" % K, lambda: c.gen_symbols(K, T, nblk, inter.data_ptr(), r["L"] * T, r["esis"], rep.data_ptr(), r["nrep"] * T))
        K, T, nblk = 100, 64, 3
        r = ref(orc, K, T, nblk)
        src = dev(torch, r["src"])
        with nanorq_amd.Sender(c, K, T, nblk, src) as tx, nanorq_amd.Receiver(c, K, T, nblk, rep_cap=32) as rx:
            timed("Sender.encode", tx.encode)
            pk = poison(torch, ((K + 20) * nblk, T), P_OUT)
            tg = poison(torch, (K + 20) * nblk, 0, torch.int32)
            timed("Sender.emit_range", lambda: tx.emit_range(0, K + 20, out=pk, tags_out=tg))
            timed("Sender.emit", lambda: tx.emit(tg, out=pk))
            timed("Receiver.add", lambda: rx.add(pk, tags=tg))
    name = max(times, key=times.get)
    NOTES["enqueue_ms"] = {k: round(v, 3) for k, v in times.items()}
    return times[name], name


@pytest.fixture(scope="module")
def F(torch, side, orc):
    return Fence(torch, side, orc)


def twice(case):
    """Every fenced case runs first without the fence, so that what a FIRST use costs is paid -- buffers of the context grow (a
    hipFree waits for the whole device), pools fill, code objects load -- then behind the fence.  WARM unfenced runs: a context
    rotates through two, three and four sets of its staging buffers and arenas, and each set grows on its own first use.  Every
    run compares its results."""
    @functools.wraps(case)
    def run(*a, **k):
        fence = k["F"]
        try:
            fence.on = False
            for _ in range(WARM):
                case(*a, **k)
        finally:
            fence.on = True
        return case(*a, **k)
    return run


# ------------------------------------------------------------------------------- 1. encode / decode vs the oracle ----
# (K, T, nblk) -> the solve workgroup (threads, waves per SIMD) a context with no option set gives it, as observed on an MI355X on
# a default context on the null stream.  (100, 64, 8) takes the 256-thread workgroup there, not the single-wave one: a context
# with no option set keeps that for launches of several hundred strips, so the ledger's default single-wave shape (100, 1024, 64)
# stands beside it; (100, 64, 1) is the small call the host planner takes.
SHAPES = [(100, 64, 8), (1000, 64, 4), (2600, 16, 2), (100, 1024, 64)]
WG = {(100, 64, 8): (256, 4), (1000, 64, 4): (256, 4), (2600, 16, 2): (768, 1), (100, 1024, 64): (64, 3), (100, 64, 1): None}


def fenced_codec(torch, F, c, s, r, what=""):
    """encode, then decode of the reference's reception (twice), each behind a fence of its own on s -> (encode stats, the plain
    decode's stats)"""
    K, T, nblk, L, nrep = r["K"], r["T"], r["nblk"], r["L"], r["nrep"]
    lost_cap = max(1, max(len(x) for x in r["lost"]))
    la = np.zeros((nblk, lost_cap), np.uint32)
    for b in range(nblk):
        la[b, :len(r["lost"][b])] = r["lost"][b]
    nl = np.array([len(x) for x in r["lost"]], np.uint32)
    re, nr = np.tile(r["esis"], (nblk, 1)), np.array(r["use"], np.uint32)
    with torch.cuda.stream(s):
        real_src, real_work, real_rep = dev(torch, r["src"]), dev(torch, r["work"]), dev(torch, r["rep"])
        d_src, d_work, d_rrows = poison(torch, (nblk, K, T), P_IN), poison(torch, (nblk, K, T), P_IN), poison(torch, (nblk, nrep, T), P_IN)
        d_rep, d_int = poison(torch, (nblk, nrep, T), P_OUT), poison(torch, (nblk, L, T), P_OUT)
        ev = F.put(s)
        d_src.copy_(real_src)
        c.encode_blocks(K, T, nblk, d_src.data_ptr(), K * T, d_rep.data_ptr(), nrep * T, r["esis"], d_int.data_ptr(), L * T)
        F.pending(ev, "encode_blocks" + what)
        est = c.stats()
        rep_c, int_c = d_rep.clone(), d_int.clone()
        # decode_blocks waits for its planner run, which a device planner makes on a stream of the context's own: where that stream
        # shares a hardware queue with s the run sits behind the fence, and the call returns when the fence has passed.  So the
        # fenced decode is the one whose planner run was issued AHEAD of the fence (nrq_decode_plan_ahead: the call then only waits
        # for a run that is over, and enqueues the solve) ...
        dargs = (K, T, nblk, d_work.data_ptr(), K * T, la, nl, re, nr)
        c.decode_plan_ahead(*dargs, None, d_rrows.data_ptr(), nrep * T)
        ev = F.put(s)
        d_work.copy_(real_work)
        d_rrows.copy_(real_rep)
        st = c.decode_blocks(*dargs, d_rrows.data_ptr(), nrep * T)
        F.pending(ev, "decode_blocks" + what)
        dst = c.stats()
        out_c = d_work.clone()
        # ... and the plain call follows behind a fence that is only known to be pending when the call is made
        d_work.fill_(P_IN), d_rrows.fill_(P_IN)
        ev = F.put(s)
        d_work.copy_(real_work)
        d_rrows.copy_(real_rep)
        F.pending(ev, "decode_blocks was called" + what)
        st2 = c.decode_blocks(*dargs, d_rrows.data_ptr(), nrep * T)
        dst2 = c.stats()
        if dst2["planner"] == 0:     # (planned on the host: the call waits for nothing on the device)
            F.pending(ev, "decode_blocks (host planner)" + what)
        out2_c = d_work.clone()
    s.synchronize()
    assert np.array_equal(host(int_c), r["inter"]), "intermediate symbols" + what
    assert np.array_equal(host(rep_c), r["rep"]), "repair symbols" + what
    for st_, out_, w in ((st, out_c, " (planner run issued ahead)"), (st2, out2_c, "")):
        assert np.array_equal(st_.astype(bool), r["ok"]), "verdicts" + what + w
        assert np.array_equal(host(out_), r["out"]), "decoded blocks" + what + w
    assert dst["plan_ahead"] == dst["planner"] and dst2["plan_ahead"] == 0, (dst, dst2)
    assert all(dst[k] == dst2[k] for k in ("strip_bytes", "wg_threads", "wg_waves_per_simd", "movers_aligned", "grid")), (dst, dst2)
    return est, dst2     # (the plain call's: the planner a context with no option set picks for it)


@pytest.mark.parametrize("shape", SHAPES + [(100, 64, 1)], ids=lambda x: "-".join(map(str, x)))
@twice
def test_codec_on_the_side_stream(torch, side, F, orc, shape):
    c, s = side
    est, dst = fenced_codec(torch, F, c, s, ref(orc, *shape))
    if WG[shape] is None:   # one small block: the host planner
        assert (dst["planner"], dst["plan_wg_threads"]) == (0, 0), dst
    else:
        for st in (est, dst):
            assert (st["strip_bytes"], st["wg_threads"], st["wg_waves_per_simd"], st["movers_aligned"]) == (16,) + WG[shape] + (1,), st
        assert (dst["planner"], dst["plan_wg_threads"], dst["host_planned"]) == (1, 1024, 0), dst


@twice
def test_gen_symbols(torch, side, F, orc):
    """nrq_gen_symbols (host ESI list, staged by the library) and its device-list form: source and repair ESIs from the
    intermediate symbols a torch op has only just written"""
    c, s = side
    K, T, nblk = 100, 64, 8
    r = ref(orc, K, T, nblk)
    Kp = nanorq_amd.params(K)["Kp"]
    esis = np.array([0, 7, K - 1] + [int(e) for e in r["esis"][:5]], np.uint32)
    isis = np.where(esis < K, esis, esis + (Kp - K)).astype(np.uint32)        # (the call takes ISIs: a repair ESI lies K' - K higher)
    want = np.stack([np.concatenate([r["src"][b][[0, 7, K - 1]], r["rep"][b][:5]]) for b in range(nblk)])
    L_ = c._L
    L_.nrq_gen_symbols_dev.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_uint32,
                                       C.c_void_p, C.c_void_p, C.c_size_t]
    n = len(isis)
    with torch.cuda.stream(s):
        real, real_isi = dev(torch, r["inter"]), dev(torch, isis)
        d_int, d_isi = poison(torch, (nblk, r["L"], T), P_IN), poison(torch, n, 0x5A5A5A5A, torch.int32)
        out1, out2 = poison(torch, (nblk, n, T), P_OUT), poison(torch, (nblk, n, T), P_OUT)
        ev = F.put(s)
        d_int.copy_(real)
        d_isi.copy_(real_isi)
        c.gen_symbols(K, T, nblk, d_int.data_ptr(), r["L"] * T, isis, out1.data_ptr(), n * T)
        F.pending(ev, "gen_symbols")
        assert L_.nrq_gen_symbols_dev(c._h, K, 0, T, nblk, C.c_void_p(d_int.data_ptr()), r["L"] * T, n, C.c_void_p(d_isi.data_ptr()),
                                      C.c_void_p(out2.data_ptr()), n * T) == 0
        F.pending(ev, "gen_symbols_dev")
        c1, c2 = out1.clone(), out2.clone()
    s.synchronize()
    assert np.array_equal(host(c1), want), "nrq_gen_symbols"
    assert np.array_equal(host(c2), want), "nrq_gen_symbols_dev"


@twice
def test_row_movers(torch, side, F):
    """nrq_scatter_symbols_dev, nrq_move_rows_dev and nrq_dev_copy (stream selector 0: the context's stream): rows and address lists
    that a torch op has only just written"""
    c, s = side
    L_ = c._L
    L_.nrq_scatter_symbols_dev.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    L_.nrq_move_rows_dev.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32]
    L_.nrq_dev_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    n, T = 301, 72
    rng = np.random.default_rng(5)
    rows = rng.integers(0, 256, (n, T), dtype=np.uint8)
    perm = rng.permutation(n)
    with torch.cuda.stream(s):
        real = dev(torch, rows)
        blob, scat, moved, copied = (poison(torch, (n, T), P_IN), poison(torch, (n, T), P_OUT), poison(torch, (n, T), P_OUT),
                                     poison(torch, (n, T), P_OUT))
        # row k -> row perm[k] of scat (row 3 skipped: address 0); pairs: row k of scat -> row k of moved, in reverse order
        dst = scat.data_ptr() + perm.astype(np.int64) * T
        dst[3] = 0
        pairs = np.stack([scat.data_ptr() + np.arange(n, dtype=np.int64)[::-1] * T, moved.data_ptr() + np.arange(n, dtype=np.int64)[::-1] * T], 1)
        real_dst, real_pairs = dev(torch, dst), dev(torch, pairs)
        d_dst, d_pairs = torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros((n, 2), dtype=torch.int64, device="cuda")
        ev = F.put(s)
        blob.copy_(real)
        d_dst.copy_(real_dst)
        d_pairs.copy_(real_pairs)
        assert L_.nrq_scatter_symbols_dev(c._h, 0, C.c_void_p(blob.data_ptr()), n, T, C.c_void_p(d_dst.data_ptr())) == 0
        assert L_.nrq_move_rows_dev(c._h, 0, C.c_void_p(d_pairs.data_ptr()), n, T) == 0
        assert L_.nrq_dev_copy(c._h, C.c_void_p(copied.data_ptr()), C.c_void_p(moved.data_ptr()), n * T) == 0
        F.pending(ev, "scatter / move_rows / dev_copy")
        got = [t.clone() for t in (scat, moved, copied)]
    s.synchronize()
    want = np.full((n, T), P_OUT, np.uint8)
    for k in range(n):
        if k != 3:
            want[perm[k]] = rows[k]
    for name, g in zip(("scatter", "move_rows", "dev_copy"), got):
        assert np.array_equal(host(g), want), name


# ----------------------------------------------------------------------------------------------- 2. resident layer ----
RK, RT, RNB, RR = 100, 64, 3, 24       # K, T, blocks, repair symbols emitted per block


def _expected_packets(r, tags):
    """the payload of every tag from the reference (source row, or the oracle's repair symbol)"""
    K = r["K"]
    out = np.zeros((len(tags), r["T"]), np.uint8)
    for k, t in enumerate(np.asarray(tags, np.uint32)):
        b, e = int(t) >> 24, int(t) & 0xFFFFFF
        out[k] = r["src"][b][e] if e < K else r["rep"][b][e - K]
    return out


def _rref(orc):
    r = ref(orc, RK, RT, RNB, seed=7, loss=0.08, oh=RR)      # (repair symbols K .. K + nrep - 1 with nrep >= RR)
    assert r["nrep"] >= RR
    return r


@twice
def test_sender_receiver_relay(torch, side, F, orc):
    """Sender.encode -> emit_range -> (loss, by torch on s) -> Receiver.add -> decode -> relay.emit, tags built by torch on s
    immediately before each call"""
    c, s = side
    K, T, nblk = RK, RT, RNB
    r = _rref(orc)
    n = K + RR
    all_tags = ((np.arange(n * nblk) % nblk) << 24 | (np.arange(n * nblk) // nblk)).astype(np.uint32)   # interleaved
    esi = all_tags & 0xFFFFFF
    keep = np.flatnonzero(~((esi % 9 == 2) & (esi < K)) & (esi < K + 14))      # every block loses 11 source symbols, gets 14 repair
    fresh = np.array([(b << 24) | (K + RR + i) for b in range(nblk) for i in range(4)], np.uint32)
    r2 = ref(orc, RK, RT, RNB, seed=7, loss=0.08, oh=RR + 4)
    with torch.cuda.stream(s):
        real = dev(torch, r["src"])
        d_src = poison(torch, (nblk, K, T), P_IN)
        pk, tg = poison(torch, (n * nblk, T), P_OUT), poison(torch, n * nblk, 0x43434343, torch.int32)
        res = poison(torch, len(keep), 77, torch.int32)
        d_keep, d_fresh_base = dev(torch, keep.astype(np.int64)), dev(torch, fresh - (K + RR))
        tx = nanorq_amd.Sender(c, K, T, nblk, d_src)
        rx = nanorq_amd.Receiver(c, K, T, nblk, rep_cap=RR)
        relay = rx.relay()
        s.synchronize()
        ev = F.put(s)
        d_src.copy_(real)
        tx.encode()
        tx.emit_range(0, n, interleave=True, out=pk, tags_out=tg)
        F.pending(ev, "Sender.emit_range")
        pk_c, tg_c = pk.clone(), tg.clone()
        rx_pk, rx_tg = pk.index_select(0, d_keep), tg.index_select(0, d_keep)       # torch, on s, immediately before the call
        rx.add(rx_pk, tags=rx_tg, results=res)
        F.pending(ev, "Receiver.add")
        res_c = res.clone()
        st, used = rx.decode()                                                      # (waits for the stream: the lists come down)
        more = d_fresh_base + (K + RR)                                              # torch, on s, immediately before the call
        out2 = relay.emit(more)
        src_c, out2_c = rx.source.clone(), out2.clone()
    s.synchronize()
    assert np.array_equal(host(tg_c), all_tags)
    assert np.array_equal(host(pk_c), _expected_packets(r, all_tags)), "emit_range"
    assert (host(res_c) == 0).all(), "every kept packet is ADDED"
    assert st.all() and np.array_equal(host(src_c), r["src"]), "decode"
    assert np.array_equal(host(out2_c), _expected_packets(r2, fresh)), "relay.emit"
    relay.close(), rx.close(), tx.close()


@twice
def test_want_emit_add(torch, side, F, orc):
    """a reception that lacks symbols lists what it wants, the sender emits that list, the reception ingests it: want -> emit ->
    add with no host-built list, the first ingest behind a fence"""
    c, s = side
    K, T, nblk = RK, RT, RNB
    r = _rref(orc)
    mod = ModelRx(K, T, nblk, RR, Kp=nanorq_amd.params(K)["Kp"])
    first = np.array([(b << 24) | e for b in range(nblk) for e in range(K) if e % 7 != b], np.uint32)
    pay = _expected_packets(r, first)
    mod.add(pay, first)
    with torch.cuda.stream(s):
        d_src = dev(torch, r["src"])
        real_pay, real_tags = dev(torch, pay), dev(torch, first)
        d_pay, d_tags = poison(torch, pay.shape, P_IN), poison(torch, len(first), 0x7F7F7F7F, torch.int32)
        tx = nanorq_amd.Sender(c, K, T, nblk, d_src)
        rx = nanorq_amd.Receiver(c, K, T, nblk, rep_cap=RR)
        tx.encode()
        s.synchronize()
        ev = F.put(s)
        d_pay.copy_(real_pay)
        d_tags.copy_(real_tags)
        rx.add(d_pay, tags=d_tags)
        F.pending(ev, "Receiver.add")
        w = rx.want(extra=1)                     # (waits)
        pk = tx.emit(w)
        rx.add(pk, tags=w)
        st, _ = rx.decode()
        w_c, pk_c, src_c = w.clone(), pk.clone(), rx.source.clone()
    s.synchronize()
    want = model_want(mod, extra=1)
    assert len(want) and np.array_equal(host(w_c), want), "want"
    assert np.array_equal(host(pk_c), _expected_packets(r, want)), "emit of the want list"
    assert st.all() and np.array_equal(host(src_c), r["src"])
    rx.close(), tx.close()


@twice
def test_packets_of_several_symbols(torch, side, F, orc):
    """emit_range_syms -> add_syms at G = 16, every third packet lost"""
    c, s = side
    K, T, nblk, G = RK, RT, RNB, 16
    r = _rref(orc)
    n = K + RR
    tags, cnt = range_list([K] * nblk, 0, 0, [n] * nblk, G, True)
    keep = np.flatnonzero((np.arange(len(tags)) % 7 != 1) | ((tags & 0xFFFFFF) >= K))     # source packets lost, all repair kept
    gone = np.setdiff1d(np.arange(len(tags)), keep)
    for b in range(nblk):     # every block loses a packet, and no more symbols than it has repair symbols
        assert 0 < sum(int(cnt[k]) for k in gone if (tags[k] >> 24) == b) <= RR, b
    with torch.cuda.stream(s):
        real = dev(torch, r["src"])
        d_src = poison(torch, (nblk, K, T), P_IN)
        d_keep = dev(torch, keep.astype(np.int64))
        tx = nanorq_amd.Sender(c, K, T, nblk, d_src)
        rx = nanorq_amd.Receiver(c, K, T, nblk, rep_cap=RR)
        s.synchronize()
        ev = F.put(s)
        d_src.copy_(real)
        tx.encode()
        out, tg, ns = tx.emit_range_syms(0, n, G, interleave=True)
        F.pending(ev, "Sender.emit_range_syms")
        rx.add_syms(out.index_select(0, d_keep), G, tags=tg.index_select(0, d_keep), nsym=ns.index_select(0, d_keep))
        F.pending(ev, "Receiver.add_syms")
        st, _ = rx.decode()
        out_c, tg_c, ns_c, src_c = out.clone(), tg.clone(), ns.clone(), rx.source.clone()
    s.synchronize()
    assert np.array_equal(host(tg_c), tags) and np.array_equal(host(ns_c), cnt), "first tags and counts"
    got = host(out_c)
    for k in range(len(tags)):
        one = (int(tags[k]) + np.arange(int(cnt[k]))).astype(np.uint32)
        assert np.array_equal(got[k, :int(cnt[k]) * T].reshape(-1, T), _expected_packets(r, one)), k
    assert st.all() and np.array_equal(host(src_c), r["src"])
    rx.close(), tx.close()


@twice
def test_object_round_trip(torch, side, F):
    """ObjectSender.emit_all -> ObjectReceiver.add -> decode -> write on an object of two block classes in two sub-blocks; every
    block loses its first four source packets"""
    from nanorq_amd import EXT_SUBBLOCKS
    c, s = side
    case = (100 * 64 - 5, 64, 0, 3, 2, 8, EXT_SUBBLOCKS)
    nrep = 8
    data = np.random.default_rng(3).integers(0, 256, case[0], dtype=np.uint8)
    with torch.cuda.stream(s):
        real = dev(torch, data)
        obj = poison(torch, case[0], P_IN)
        p = nanorq_amd.obj_params_enc(case[0], *case[1:])
        assert (p.ZL, p.ZS, p.N) == (1, 2, 2) and p.KL != p.KS, p.as_dict()
        blocks = [(p.KL, p.KpL)] * p.ZL + [(p.KS, p.KpS)] * p.ZS
        npk = sum(k + nrep for k, _ in blocks)
        tg = poison(torch, npk, 0x43434343, torch.int32)
        pk = poison(torch, (npk, (case[1] + 4 + 15) // 16 * 16), P_OUT)
        # block-major: block b's packets are ESI 0 .. K_b + nrep - 1
        keep = np.concatenate([sum(k + nrep for k, _ in blocks[:b]) + np.arange(4, k + nrep) for b, (k, _) in enumerate(blocks)])
        d_keep = dev(torch, keep.astype(np.int64))
        final = poison(torch, case[0] + 16, P_OUT)
        s.synchronize()
        ev = F.put(s)
        obj.copy_(real)
        tx = nanorq_amd.ObjectSender(c, obj, *case[1:])      # (the constructor lays the object out into rows: it reads it)
        assert tx.blocks == blocks and tx.count_all(nrep) == npk and tx.stride(True) == pk.shape[1]
        tx.encode()
        tx.emit_all(nrep, interleave=False, inline=True, out=pk, tags_out=tg)
        F.pending(ev, "ObjectSender.emit_all")
        rx = nanorq_amd.ObjectReceiver(c, *tx.oti, flags=case[6], rep_cap=nrep)
        rx.add(pk.index_select(0, d_keep), inline=True)
        F.pending(ev, "ObjectReceiver.add")
        st, _ = rx.decode()
        out, left = rx.write()
        _, left2 = rx.write(final)
        out_c, final_c, tg_c = out.clone(), final.clone(), tg.clone()
    s.synchronize()
    want_tags = np.concatenate([(b << 24) | np.arange(k + nrep) for b, (k, _) in enumerate(blocks)]).astype(np.uint32)
    assert np.array_equal(host(tg_c), want_tags)
    assert st.all() and left == 0 and left2 == 0
    assert np.array_equal(host(out_c), data), "write() into a tensor of the binding's own"
    f = host(final_c)
    assert np.array_equal(f[:case[0]], data) and (f[case[0]:] == P_OUT).all(), "write(out)"
    rx.close(), tx.close()


SET_KEYS = (9, 5)      # attached in this order; the set's block order is by key


def _set_members(torch, c, r, srcs):
    txs = [nanorq_amd.Sender(c, RK, RT, RNB, srcs[i]) for i in range(2)]
    rxs = [nanorq_amd.Receiver(c, RK, RT, RNB, rep_cap=RR) for _ in range(2)]
    sset, rset = nanorq_amd.SenderSet(c, RT), nanorq_amd.ReceiverSet(c, RT)
    for i, key in enumerate(SET_KEYS):
        sset.attach(key, txs[i])
        rset.attach(key, rxs[i])
    return txs, rxs, sset, rset


@twice
def test_sets(torch, side, F, orc):
    """SenderSet.emit -> ReceiverSet.add -> want -> emit -> add -> decode with two members; keys and tags built by torch on s"""
    c, s = side
    K, T, nblk = RK, RT, RNB
    refs = [_rref(orc), ref(orc, RK, RT, RNB, seed=11, loss=0.08, oh=RR)]
    mods = [ModelRx(K, T, nblk, RR, Kp=nanorq_amd.params(K)["Kp"]) for _ in range(2)]
    one = np.array([(b << 24) | e for b in range(nblk) for e in range(K) if e % 6 != b + 1], np.uint32)
    tags = np.concatenate([one, one])
    keys = np.repeat(np.array(SET_KEYS, np.uint32), len(one))
    order = np.random.default_rng(2).permutation(len(tags))
    tags, keys = tags[order], keys[order]
    expect = np.zeros((len(tags), T), np.uint8)
    for i, key in enumerate(SET_KEYS):
        m = keys == key
        expect[m] = _expected_packets(refs[i], tags[m])
        mods[i].add(expect[m], tags[m])
    with torch.cuda.stream(s):
        real = [dev(torch, x["src"]) for x in refs]
        srcs = [poison(torch, (nblk, K, T), P_IN) for _ in range(2)]
        txs, rxs, sset, rset = _set_members(torch, c, refs, srcs)
        real_tags, real_keys = dev(torch, tags), dev(torch, keys)
        d_tags, d_keys = poison(torch, len(tags), 0x7F7F7F7F, torch.int32), poison(torch, len(tags), 0x7F7F7F7F, torch.int32)
        pk = poison(torch, (len(tags), T), P_OUT)
        s.synchronize()
        ev = F.put(s)
        for i in range(2):
            srcs[i].copy_(real[i])
            txs[i].encode()
        d_tags.copy_(real_tags)
        d_keys.copy_(real_keys)
        sset.emit(d_keys, d_tags, out=pk)
        F.pending(ev, "SenderSet.emit")
        pk_c = pk.clone()
        rset.add(pk, keys=d_keys, tags=d_tags)
        F.pending(ev, "ReceiverSet.add")
        nl, nr = rset.counts()                   # (waits)
        wk, wt = rset.want(extra=1)
        pk2 = sset.emit(wk, wt)
        rset.add(pk2, keys=wk, tags=wt)
        st, _ = rset.decode()
        wk_c, wt_c, pk2_c = wk.clone(), wt.clone(), pk2.clone()
        src_c = [x.source.clone() for x in rxs]
    s.synchronize()
    assert np.array_equal(host(pk_c), expect), "SenderSet.emit"
    by_key = sorted(range(2), key=lambda i: SET_KEYS[i])
    assert np.array_equal(nl, np.concatenate([[len(m) for m in mods[i].missing] for i in by_key])), "counts"
    assert not nr.any()
    want_t = np.concatenate([model_want(mods[i], extra=1) for i in by_key])
    want_k = np.concatenate([np.full(len(model_want(mods[i], extra=1)), SET_KEYS[i], np.uint32) for i in by_key])
    assert len(want_t) and np.array_equal(host(wt_c), want_t) and np.array_equal(host(wk_c), want_k), "ReceiverSet.want"
    exp2 = np.zeros((len(want_t), T), np.uint8)
    for i in range(2):
        m = want_k == SET_KEYS[i]
        exp2[m] = _expected_packets(refs[i], want_t[m])
    assert np.array_equal(host(pk2_c), exp2), "SenderSet.emit of the want list"
    assert st.all()
    for i in range(2):
        assert np.array_equal(host(src_c[i]), refs[i]["src"]), i
    for h in (sset, rset, *txs, *rxs):
        h.close()


@twice
def test_set_table_is_not_replaced_under_a_pending_ingest(torch, side, F, orc):
    """attach() replaces the set's member table in device memory with a blocking copy on stream 0; an ingest enqueued before it
    on the context's stream still reads the old table.  The ingest waits behind the fence, then a second member is attached: its
    packets in that ingest belong to no member (their results entries untouched, its rows never written)."""
    c, s = side
    K, T, nblk = RK, RT, RNB
    r = _rref(orc)
    one = np.array([(b << 24) | e for b in range(nblk) for e in range(0, K, 3)], np.uint32)
    tags = np.concatenate([one, one])
    keys = np.repeat(np.array([9, 5], np.uint32), len(one))       # key 5 sorts in front of key 9: the table's rows shift
    pay = _expected_packets(r, tags)
    with torch.cuda.stream(s):
        rx9, rx5 = (nanorq_amd.Receiver(c, K, T, nblk, rep_cap=RR) for _ in range(2))
        rset = nanorq_amd.ReceiverSet(c, T)
        rset.attach(9, rx9)
        real_pay, real_tags, real_keys = dev(torch, pay), dev(torch, tags), dev(torch, keys)
        d_pay, d_tags, d_keys = poison(torch, pay.shape, P_IN), poison(torch, len(tags), 0x7F7F7F7F, torch.int32), poison(torch, len(tags), 0x7F7F7F7F, torch.int32)
        res = poison(torch, len(tags), 77, torch.int32)
        s.synchronize()
        ev = F.put(s)
        d_pay.copy_(real_pay), d_tags.copy_(real_tags), d_keys.copy_(real_keys)
        rset.add(d_pay, keys=d_keys, tags=d_tags, results=res)
        F.pending(ev, "ReceiverSet.add")
        rset.attach(5, rx5)                      # (waits for the context's stream, then uploads)
        res_c = res.clone()
    s.synchronize()
    got = host(res_c).view(np.int32)
    assert (got[keys == 9] == 0).all(), "the first member's packets are ADDED"
    assert (got[keys == 5] == 77).all(), "packets of a key attached AFTER the ingest was enqueued were ingested"
    nl5, nr5 = rx5.counts()
    assert (nl5 == K).all() and not nr5.any()
    nl9, _ = rx9.counts()
    assert (nl9 == K - len(one) // nblk).all()
    for h in (rset, rx9, rx5):
        h.close()


# ------------------------------------------------------------------------------------------------- 3. set_stream ----
def test_set_stream_moves_the_context(torch, F, orc):
    """a context created on the null stream is moved to a side stream, runs a fenced encode / decode there, is moved back and
    runs another one on the null stream (the fence and the torch ops on torch's default stream, which is the null stream)"""
    s = torch.cuda.Stream()
    c = nanorq_amd.Context(0)
    try:
        r = ref(orc, 1000, 64, 4)
        for F.on in (False,) * WARM + (True,):      # (as `twice`: the context's first calls grow its buffers)
            c.set_stream(s.cuda_stream)
            fenced_codec(torch, F, c, s, r, " (moved to the side stream)")
            c.set_stream(0)
            fenced_codec(torch, F, c, torch.cuda.default_stream(), r, " (moved back to the null stream)")
    finally:
        F.on = True
        c.close()


# ---------------------------------------------------------------------------------- 4. tensors of the binding's own ----
# The context on the side stream, torch's CURRENT stream the default one, the fence on the DEFAULT stream: whatever the binding
# allocates or fills itself must be ordered on the context's stream, and no call may wait for the whole device (the fence would
# have passed).  Inputs are complete before the fence; results are read on the side stream.
def _read(torch, c, s, *ts):
    """the tensors on the host, read on s once BOTH streams are through: a fill the binding left on torch's current stream, behind
    the fence, has landed by then"""
    c.sync()
    torch.cuda.default_stream().synchronize()
    with torch.cuda.stream(s):
        out = [host(t) for t in ts]
    return out if len(out) > 1 else out[0]


@twice
def test_binding_owned_receiver_tensors(torch, side, F, orc):
    """Receiver(...) with source rows of its own; want / held and their packet forms"""
    from held_support import host_held
    from runs_support import packetise
    c, s = side
    K, T, nblk, G = RK, RT, RNB, 16
    r = _rref(orc)
    mod = ModelRx(K, T, nblk, RR, Kp=nanorq_amd.params(K)["Kp"])
    tags = np.array([(b << 24) | e for b in range(nblk) for e in list(range(0, K, 2)) + [K + 3, K + 1]], np.uint32)
    pay = _expected_packets(r, tags)
    mod.add(pay, tags)
    d0 = torch.cuda.default_stream()
    with torch.cuda.stream(s):
        d_pay, d_tags = dev(torch, pay), dev(torch, tags)
    s.synchronize()
    ev = F.put(d0)
    rx = nanorq_amd.Receiver(c, K, T, nblk, rep_cap=RR)        # (its source rows: a tensor of the binding's own)
    rx.add(d_pay, tags=d_tags)
    w, ws = rx.want(extra=2), rx.want(source=True)
    h = rx.held()
    wt, wn = rx.want_syms(G, source=True)
    ht, hn = rx.held_syms(G)
    F.pending(ev, "Receiver / want / held / want_syms / held_syms")
    w, ws, h, wt, wn, ht, hn, rows = _read(torch, c, s, w, ws, h, wt, wn, ht, hn, rx.source)
    d0.synchronize()
    seen, _, _ = model_books(mod)
    held = host_held(0, K, [seen[b, :K] for b in range(nblk)], mod.reps)
    assert np.array_equal(w, model_want(mod, extra=2)) and np.array_equal(ws, model_want(mod, source=True)), "want"
    assert np.array_equal(h, held), "held"
    for got, lst in (((wt, wn), model_want(mod, source=True)), ((ht, hn), held)):
        et, en = packetise(lst, G, lambda sbn: K)
        assert np.array_equal(got[0], et) and np.array_equal(got[1], en), "the listing in packets"
    for b in range(nblk):
        assert np.array_equal(rows[b][::2], r["src"][b][::2]), "the reception's own source rows"
    rx.close()


@twice
def test_binding_owned_emitter_tensors(torch, side, F, orc):
    """emit / emit_syms / emit_range_syms with out=None, ObjectSender.emit_all_syms, ObjectReceiver.write() with out=None"""
    from nanorq_amd import EXT_SUBBLOCKS
    c, s = side
    K, T, nblk, G = RK, RT, RNB, 16
    r = _rref(orc)
    d0 = torch.cuda.default_stream()
    tags = np.array([(b << 24) | e for b in range(nblk) for e in (0, 5, K - 1, K, K + 7)], np.uint32)
    ftags = np.array([(b << 24) | e for b in range(nblk) for e in (0, 32, K)], np.uint32)        # first tags of packets of G symbols
    case = (100 * 64 - 5, 64, 0, 3, 2, 8, EXT_SUBBLOCKS)
    data = np.random.default_rng(3).integers(0, 256, case[0], dtype=np.uint8)
    with torch.cuda.stream(s):
        d_src, d_tags, d_ftags, obj = dev(torch, r["src"]), dev(torch, tags), dev(torch, ftags), dev(torch, data)
        tx = nanorq_amd.Sender(c, K, T, nblk, d_src)
        otx = nanorq_amd.ObjectSender(c, obj, *case[1:])
        tx.encode(), otx.encode()
    s.synchronize()
    ev = F.put(d0)
    p1 = tx.emit(d_tags)                                           # _out
    p2 = tx.emit_syms(d_ftags, G)                                  # _out_syms
    p3, t3, n3 = tx.emit_range_syms(0, K + RR, G)                  # _range_syms
    p4, t4, n4 = otx.emit_all_syms(4, G, interleave=False, inline=True)
    F.pending(ev, "emit / emit_syms / emit_range_syms / emit_all_syms with tensors of the binding's own")
    p1, p2, p3, t3, n3, t4, n4, p4 = _read(torch, c, s, p1, p2, p3, t3, n3, t4, n4, p4)
    assert np.array_equal(p1, _expected_packets(r, tags)), "emit"
    for k, t in enumerate(ftags):
        cnt = min(G, K - (int(t) & 0xFFFFFF)) if (int(t) & 0xFFFFFF) < K else G
        assert np.array_equal(p2[k, :cnt * T].reshape(-1, T), _expected_packets(r, (int(t) + np.arange(cnt)).astype(np.uint32))), "emit_syms"
    et, en = range_list([K] * nblk, 0, 0, [K + RR] * nblk, G, True)
    assert np.array_equal(t3, et) and np.array_equal(n3, en), "emit_range_syms: first tags and counts"
    for k in range(len(et)):
        one = (int(et[k]) + np.arange(int(en[k]))).astype(np.uint32)
        assert np.array_equal(p3[k, :int(en[k]) * T].reshape(-1, T), _expected_packets(r, one)), k
    blocks = otx.blocks
    et4 = np.concatenate([range_list([k], b, 0, [k + 4], G, False)[0] for b, (k, _) in enumerate(blocks)])
    en4 = np.concatenate([range_list([k], b, 0, [k + 4], G, False)[1] for b, (k, _) in enumerate(blocks)])
    assert np.array_equal(t4, et4) and np.array_equal(n4, en4), "emit_all_syms: first tags and counts"
    for h in (otx, tx):
        h.close()


@twice
def test_binding_owned_write(torch, side, F):
    """ObjectReceiver.write() with out=None: the binding zeroes a tensor of its own and the library writes the complete blocks into
    it -- here every block but the last, whose bytes must stay zero; and the call waits for the context's stream only"""
    from nanorq_amd import EXT_SUBBLOCKS
    c, s = side
    case = (100 * 64 - 5, 64, 0, 3, 2, 8, EXT_SUBBLOCKS)
    data = np.random.default_rng(3).integers(0, 256, case[0], dtype=np.uint8)
    d0 = torch.cuda.default_stream()
    with torch.cuda.stream(s):
        obj = dev(torch, data)
        otx = nanorq_amd.ObjectSender(c, obj, *case[1:])
        blocks = otx.blocks
        orx = nanorq_amd.ObjectReceiver(c, *otx.oti, flags=case[6], rep_cap=8)
        otx.encode()
        tags = np.concatenate([(b << 24) | np.arange(k) for b, (k, _) in enumerate(blocks[:-1])]).astype(np.uint32)
        d_tags = dev(torch, tags)
        orx.add(otx.emit(d_tags), tags=d_tags)       # every source symbol of every block but the last
        nl, _ = orx.counts()
    s.synchronize()
    assert list(nl) == [0] * (len(blocks) - 1) + [blocks[-1][0]]
    ev = F.put(d0)
    whole, left = orx.write()
    F.pending(ev, "ObjectReceiver.write")
    whole = _read(torch, c, s, whole)
    cut = sum(k for k, _ in blocks[:-1]) * case[1]
    assert left == 1 and np.array_equal(whole[:cut], data[:cut]), "the complete blocks"
    assert not whole[cut:].any(), "the incomplete block's bytes are the binding's zeroes"
    for h in (orx, otx):
        h.close()


@twice
def test_binding_owned_set_tensors(torch, side, F, orc):
    """ReceiverSet.want / held / want_syms / held_syms and SenderSet.emit / emit_syms with out=None"""
    from held_support import host_held
    from runs_support import packetise
    c, s = side
    K, T, nblk, G = RK, RT, RNB, 16
    refs = [_rref(orc), ref(orc, RK, RT, RNB, seed=11, loss=0.08, oh=RR)]
    mods = [ModelRx(K, T, nblk, RR, Kp=nanorq_amd.params(K)["Kp"]) for _ in range(2)]
    one = np.array([(b << 24) | e for b in range(nblk) for e in list(range(1, K, 2)) + [K + 2]], np.uint32)
    tags, keys = np.concatenate([one, one]), np.repeat(np.array(SET_KEYS, np.uint32), len(one))
    expect = np.zeros((len(tags), T), np.uint8)
    for i, key in enumerate(SET_KEYS):
        m = keys == key
        expect[m] = _expected_packets(refs[i], tags[m])
        mods[i].add(expect[m], tags[m])
    d0 = torch.cuda.default_stream()
    with torch.cuda.stream(s):
        srcs = [dev(torch, x["src"]) for x in refs]
        txs, rxs, sset, rset = _set_members(torch, c, refs, srcs)
        for t in txs:
            t.encode()
        d_tags, d_keys = dev(torch, tags), dev(torch, keys)
    s.synchronize()
    ev = F.put(d0)
    pk = sset.emit(d_keys, d_tags)
    rset.add(pk, keys=d_keys, tags=d_tags)
    wk, wt = rset.want(source=True)
    hk, ht = rset.held()
    sk, st_, sn = rset.want_syms(G, source=True)
    gk, gt, gn = rset.held_syms(G)
    pk2 = sset.emit_syms(sk, st_, G, nsym=sn)
    F.pending(ev, "the sets' listings and emits with tensors of the binding's own")
    pk, wk, wt, hk, ht, sk, st_, sn, gk, gt, gn, pk2 = _read(torch, c, s, pk, wk, wt, hk, ht, sk, st_, sn, gk, gt, gn, pk2)
    d0.synchronize()
    assert np.array_equal(pk, expect), "SenderSet.emit"
    by_key = sorted(range(2), key=lambda i: SET_KEYS[i])
    wants = [model_want(mods[i], source=True) for i in by_key]
    helds = [host_held(0, K, [model_books(mods[i])[0][b, :K] for b in range(nblk)], mods[i].reps) for i in by_key]
    kk = [SET_KEYS[i] for i in by_key]
    for (gk_, gt_), lists, name in (((wk, wt), wants, "want"), ((hk, ht), helds, "held")):
        assert np.array_equal(gt_, np.concatenate(lists)), name
        assert np.array_equal(gk_, np.concatenate([np.full(len(x), k, np.uint32) for x, k in zip(lists, kk)])), name + " keys"
    for (gk_, gt_, gn_), lists, name in (((sk, st_, sn), wants, "want_syms"), ((gk, gt, gn), helds, "held_syms")):
        pks = [packetise(x, G, lambda sbn: K) for x in lists]
        assert np.array_equal(gt_, np.concatenate([p[0] for p in pks])) and np.array_equal(gn_, np.concatenate([p[1] for p in pks])), name
        assert np.array_equal(gk_, np.concatenate([np.full(len(p[0]), k, np.uint32) for p, k in zip(pks, kk)])), name + " keys"
    row = 0
    for i, p in zip(by_key, [packetise(x, G, lambda sbn: K) for x in wants]):
        for t, n in zip(*p):
            one_ = (int(t) + np.arange(int(n))).astype(np.uint32)
            assert np.array_equal(pk2[row, :int(n) * T].reshape(-1, T), _expected_packets(refs[i], one_)), "SenderSet.emit_syms"
            row += 1
    for h in (sset, rset, *txs, *rxs):
        h.close()


# ------------------------------------------------------------------------------------------ 5. two contexts at once ----
@pytest.fixture(scope="module")
def pair(torch):
    import gpu_support as G
    a, b = G.new_side(), G.new_side()
    yield a, b
    a[0].close(), b[0].close()


SHAPE_KEYS = ("strip_bytes", "wg_threads", "wg_waves_per_simd", "movers_aligned", "grid", "planner", "plan_wg_threads", "host_planned",
              "encplan_device", "plan_segmented")


def _shape_of(st):
    return {k: st[k] for k in SHAPE_KEYS}


def _encode_on(c, r):
    """encode through the C ABI with numpy in / out on context c -> stats; the outputs against the oracle"""
    import gpu_support as G
    rep, inter = G.gpu_encode(r["src"], r["K"], r["T"], r["esis"], want_inter=True, kind=c)
    st = c.stats()
    assert np.array_equal(inter, r["inter"]) and np.array_equal(rep, r["rep"]), ("encode", r["K"])
    return _shape_of(st)


def _decode_on(c, r):
    import gpu_support as G
    nblk = r["nblk"]
    st_, out, _ = G.gpu_decode(r["work"], r["K"], r["T"], r["lost"], [r["esis"][:n] for n in r["use"]],
                               [r["rep"][b][:r["use"][b]] for b in range(nblk)], kind=c)
    st = c.stats()
    assert np.array_equal(st_.astype(bool), r["ok"]) and np.array_equal(out, r["out"]), ("decode", r["K"])
    return _shape_of(st)


def _both(pool, fa, fb):
    """fa and fb at the same time on two host threads, each under the file's timeout -> their results"""
    a, b = pool.submit(fa), pool.submit(fb)
    return a.result(timeout=STEP_TIMEOUT), b.result(timeout=STEP_TIMEOUT)


def test_two_contexts_at_once(pair, orc):
    """Two side-stream contexts driven from two host threads, four rounds: A encodes (1000, 64, 4) while B decodes (2600, 16, 2)
    and the other way round; both decode K = 1000 with different receptions; A builds a device encode plan (K = 15000) while B
    decodes 64 blocks of K = 100.  Every output against the oracle, and stats() of each context describes ITS call: the launch
    shape the same call gave when it ran alone."""
    (A, _), (B, _) = pair
    r1, r2 = ref(orc, 1000, 64, 4), ref(orc, 2600, 16, 2)
    r1b = ref(orc, 1000, 64, 4, seed=5, loss=0.3)
    r3, r4 = ref(orc, 15000, 16, 1, loss=0.02, decode=False), ref(orc, 100, 64, 64)
    alone = {}
    for c in (A, B):      # each call alone, on each context: what its stats look like
        alone[c] = dict(e1=_encode_on(c, r1), d1=_decode_on(c, r1), d1b=_decode_on(c, r1b), e2=_encode_on(c, r2), d2=_decode_on(c, r2),
                        d4=_decode_on(c, r4))
    A.clear_plan_cache()
    alone[A]["e3"] = _encode_on(A, r3)
    assert alone[A]["e3"]["encplan_device"] == 1 and alone[A]["e1"] != alone[A]["d2"] and alone[A]["d1"] != alone[A]["d4"]
    with cf.ThreadPoolExecutor(2) as pool:
        for rnd in range(4):
            sa, sb = _both(pool, lambda: _encode_on(A, r1), lambda: _decode_on(B, r2))
            assert (sa, sb) == (alone[A]["e1"], alone[B]["d2"]), rnd
            sa, sb = _both(pool, lambda: _decode_on(A, r2), lambda: _encode_on(B, r1))
            assert (sa, sb) == (alone[A]["d2"], alone[B]["e1"]), rnd
            sa, sb = _both(pool, lambda: _decode_on(A, r1), lambda: _decode_on(B, r1b))
            assert (sa, sb) == (alone[A]["d1"], alone[B]["d1b"]), rnd
            A.clear_plan_cache()
            sa, sb = _both(pool, lambda: _encode_on(A, r3), lambda: _decode_on(B, r4))
            assert (sa, sb) == (alone[A]["e3"], alone[B]["d4"]), rnd


@twice
def test_hand_over_between_contexts(torch, pair, F, orc):
    """Sender on A emits; stream B waits for stream A's event (the caller's ordering); Receiver on B ingests and decodes: the
    one-context result.  The fence is on A's stream, so B's ingest is enqueued long before A's packets exist."""
    (A, sa), (B, sb) = pair
    K, T, nblk = RK, RT, RNB
    r = _rref(orc)
    n = K + RR
    all_tags = ((np.arange(n * nblk) % nblk) << 24 | (np.arange(n * nblk) // nblk)).astype(np.uint32)
    esi = all_tags & 0xFFFFFF
    keep = np.flatnonzero(~((esi % 9 == 2) & (esi < K)) & (esi < K + 14))
    with torch.cuda.stream(sa):
        real = dev(torch, r["src"])
        d_src = poison(torch, (nblk, K, T), P_IN)
        pk, tg = poison(torch, (n * nblk, T), P_OUT), poison(torch, n * nblk, 0x43434343, torch.int32)
        d_keep = dev(torch, keep.astype(np.int64))
        tx = nanorq_amd.Sender(A, K, T, nblk, d_src)
    with torch.cuda.stream(sb):
        rx = nanorq_amd.Receiver(B, K, T, nblk, rep_cap=RR)
        res = poison(torch, len(keep), 77, torch.int32)
    sa.synchronize(), sb.synchronize()
    with torch.cuda.stream(sa):
        ev = F.put(sa)
        d_src.copy_(real)
        tx.encode()
        tx.emit_range(0, n, interleave=True, out=pk, tags_out=tg)
        done = torch.cuda.Event()
        done.record(sa)
    with torch.cuda.stream(sb):
        sb.wait_event(done)
        rx.add(pk.index_select(0, d_keep), tags=tg.index_select(0, d_keep), results=res)
        F.pending(ev, "Receiver.add on the other context")
        st, _ = rx.decode()
        src_c, res_c = rx.source.clone(), res.clone()
    sb.synchronize(), sa.synchronize()
    assert (host(res_c).view(np.int32) == 0).all()
    assert st.all() and np.array_equal(host(src_c), r["src"])
    rx.close(), tx.close()


def test_the_side_streams_do_not_share_the_null_stream_s_hardware_queue(side, pair):
    """The runtime multiplexes the process's streams over a few hardware queues, and two streams on one queue take turns: a kernel
    the library put on stream 0 by mistake would then still run behind the fence, and every case above would pass by accident
    (seen on an MI355X with four queues: both mutants of docs/LAB_NOTES.md passed on such a stream).  gpu_support picks side
    streams that were seen not to wait for the null stream; if it found none, the file has proved nothing and says so here."""
    import gpu_support as G
    assert G.side_independent(side[0]), "no stream of this process runs beside the null stream"
    NOTES["streams_turned_down"] = len(G._REJECTED)


def test_zz_calibration_on_record(F):
    """the numbers of the fence (pytest -s prints them; docs/LAB_NOTES.md quotes a run)"""
    print("\nSTREAMS CALIBRATION", NOTES)
    assert F.passes >= 1 and FENCE_MIN_MS <= NOTES["fence_ms"] <= FENCE_MAX_MS
    assert NOTES["fence_ms"] >= 20.0 * NOTES["slowest_enqueue_ms"]
