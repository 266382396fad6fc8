"""Worker of tests/test_host_model.py: one group of scenarios of the library's HOST layer over the model HIP runtime
(tests/emu/hip_model.h), in a process of its own whose library is tests/emu/libnanorq_model.so.  Kernels do not run there; what is
checked is the order and the lifetimes the host layer gives its runtime calls.  Prints one JSON object: per scenario what it saw.

    python host_model_worker.py GROUP        (GROUPS below)
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

os.environ["NANORQ_HIP_LIB"] = os.path.join(ROOT, "tests", "emu", "libnanorq_model.so")
os.environ["NANORQ_HIP_FAULT_INJECT"] = "1"
os.environ["NRQ_HOST_PLANNER"] = "1"

import numpy as np  # noqa: E402

import nanorq_amd  # noqa: E402
from util import loss_pattern, payload  # noqa: E402

H2D, D2H, D2D = 1, 2, 3
POISON = 0xDB
vp, sz = C.c_void_p, C.c_size_t


class HmArg(C.Structure):
    _fields_ = [("p", vp), ("n", sz), ("kind", C.c_int)]


ARG_PTR, ARG_CONST_PTR, ARG_BYTES = 0, 1, 2


def model():
    """the model's own interface and the runtime functions it stands in for, typed for ctypes"""
    L = nanorq_amd.lib()
    if getattr(L, "_hm_typed", False):
        return L
    L.hm_hazards_json.restype = sz
    L.hm_hazards_json.argtypes = [C.c_char_p, sz]
    L.hm_hazard_count.restype = C.c_uint64
    L.hm_counters.argtypes = [C.POINTER(C.c_uint64)]
    L.hm_block_of.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
    L.hm_pending_on.argtypes = [vp]
    L.hm_launch_named.argtypes = [C.c_char_p, vp, C.POINTER(HmArg), C.c_int]
    L.hm_launch_named.restype = None
    L.hipMalloc.argtypes = [C.POINTER(vp), sz]
    L.hipFree.argtypes = [vp]
    L.hipHostMalloc.argtypes = [C.POINTER(vp), sz, C.c_uint]
    L.hipHostFree.argtypes = [vp]
    L.hipHostRegister.argtypes = [vp, sz, C.c_uint]
    L.hipHostUnregister.argtypes = [vp]
    L.hipMemcpyAsync.argtypes = [vp, vp, sz, C.c_int, vp]
    L.hipMemcpy.argtypes = [vp, vp, sz, C.c_int]
    L.hipMemsetAsync.argtypes = [vp, C.c_int, sz, vp]
    L.hipStreamCreateWithFlags.argtypes = [C.POINTER(vp), C.c_uint]
    L.hipStreamDestroy.argtypes = [vp]
    L.hipStreamSynchronize.argtypes = [vp]
    L.hipStreamWaitEvent.argtypes = [vp, vp, C.c_uint]
    L.hipEventCreate.argtypes = [C.POINTER(vp)]
    L.hipEventDestroy.argtypes = [vp]
    L.hipEventRecord.argtypes = [vp, vp]
    L.hipEventSynchronize.argtypes = [vp]
    L.nrq_dev_pool_books.argtypes = [vp, C.POINTER(sz)]
    L.nrq_dev_trim.argtypes = [vp]
    L._hm_typed = True
    return L


def hazards(clear=True):
    L = model()
    n = L.hm_hazards_json(None, 0)
    buf = C.create_string_buffer(n + 16)
    L.hm_hazards_json(buf, n + 16)
    out = json.loads(buf.value.decode())
    if clear:
        L.hm_hazards_clear()
    return out


def brief(hz):
    """hazards as short strings, for the report"""
    def op(o):
        return "-" if o is None else "%s [stream %d #%d, %s]" % (o["what"], o["stream"], o["n"], o["site"])
    return ["%s: %s | %s | %s | allocation of %d bytes (kind %d)" % (h["kind"], h["detail"], op(h["first"]), op(h["second"]),
                                                                     h["allocation"]["size"], h["allocation"]["kind"]) for h in hz]


def counters():
    c = (C.c_uint64 * 8)()
    model().hm_counters(c)
    return dict(zip(("ops", "launches", "copies", "unrecorded_waits", "live", "stale_words", "deferred", "unnamed_launches"), map(int, c)))


def block_of(p):
    base, size, kind = C.c_uint64(), C.c_uint64(), C.c_int()
    if not model().hm_block_of(vp(p), C.byref(base), C.byref(size), C.byref(kind)):
        return None
    return base.value, size.value, kind.value


# ------------------------------------------------------------------------------------------------ a. the detector ----
class Rt:
    """the runtime calls of a hand-built scenario, every one checked for hipSuccess"""

    def __init__(self):
        self.L = model()

    def ok(self, rc):
        assert rc == 0, rc

    def malloc(self, n):
        p = vp()
        self.ok(self.L.hipMalloc(C.byref(p), n))
        return p.value

    def pinned(self, n):
        p = vp()
        self.ok(self.L.hipHostMalloc(C.byref(p), n, 0))
        return p.value, np.ctypeslib.as_array((C.c_uint8 * n).from_address(p.value))

    def stream(self):
        s = vp()
        self.ok(self.L.hipStreamCreateWithFlags(C.byref(s), 1))
        return s.value

    def event(self):
        e = vp()
        self.ok(self.L.hipEventCreate(C.byref(e)))
        return e.value

    def memset(self, d, v, n, s):
        self.ok(self.L.hipMemsetAsync(vp(d), v, n, vp(s)))

    def copy(self, dst, src, n, kind, s):
        self.ok(self.L.hipMemcpyAsync(vp(dst), vp(src), n, kind, vp(s)))

    def record(self, e, s):
        self.ok(self.L.hipEventRecord(vp(e), vp(s)))

    def wait(self, s, e):
        self.ok(self.L.hipStreamWaitEvent(vp(s), vp(e), 0))

    def sync(self, s):
        self.ok(self.L.hipStreamSynchronize(vp(s)))

    def launch(self, name, s, *args):
        """args: ("ptr" | "cptr", address) or ("bytes", ctypes object)"""
        a = (HmArg * len(args))()
        keep = []
        for i, (k, v) in enumerate(args):
            if k == "bytes":
                keep.append(v)
                a[i] = HmArg(C.addressof(v), C.sizeof(v), ARG_BYTES)
            else:
                a[i] = HmArg(v, 0, ARG_PTR if k == "ptr" else ARG_CONST_PTR)
        self.L.hm_launch_named(name.encode(), vp(s), a, len(args))


def group_detector():
    r = Rt()
    L = r.L
    out = {}
    hazards()

    def done(name, **extra):
        out[name] = dict(kinds=[h["kind"] for h in hazards(clear=False)], text=brief(hazards()), **extra)

    s1, s2 = r.stream(), r.stream()
    # unordered write / write on two streams
    d = r.malloc(8192)
    r.memset(d, 1, 8192, s1)
    r.memset(d, 2, 8192, s2)
    done("ww_unordered")
    r.sync(s1), r.sync(s2)
    # ... two disjoint halves of one allocation: no conflict
    r.memset(d, 1, 4096, s1)
    r.memset(d + 4096, 2, 4096, s2)
    done("ww_disjoint")
    r.sync(s1), r.sync(s2)
    # ... ordered by record / wait
    e = r.event()
    r.memset(d, 1, 8192, s1)
    r.record(e, s1)
    r.wait(s2, e)
    r.memset(d, 2, 8192, s2)
    done("ww_record_wait")
    r.sync(s1), r.sync(s2)
    # ... ordered by the host: it waited for the first stream before it enqueued on the second
    r.memset(d, 1, 8192, s1)
    r.sync(s1)
    r.memset(d, 2, 8192, s2)
    done("ww_host_sync")
    r.sync(s2)
    # ... the event recorded BEFORE the write it should have covered
    r.record(e, s1)
    r.memset(d, 1, 8192, s1)
    r.wait(s2, e)
    r.memset(d, 2, 8192, s2)
    done("ww_recorded_too_early")
    r.sync(s1), r.sync(s2)
    # a wait for an event nobody recorded orders nothing
    e2 = r.event()
    before = counters()["unrecorded_waits"]
    r.memset(d, 1, 8192, s1)
    r.wait(s2, e2)
    r.memset(d, 2, 8192, s2)
    done("wait_never_recorded", unrecorded=counters()["unrecorded_waits"] - before)
    r.sync(s1), r.sync(s2)
    # read / read needs no order; read / write does
    d2 = r.malloc(8192)
    r.copy(d2, d, 4096, D2D, s1)
    r.copy(d2 + 4096, d, 4096, D2D, s2)
    done("rr_unordered")
    r.memset(d, 3, 8192, s2)
    done("rw_unordered")
    r.sync(s1), r.sync(s2)
    # a page-locked source rewritten before the host synchronised behind its copy
    p, pv = r.pinned(4096)
    pv[:] = 7
    r.copy(d, p, 4096, H2D, s1)
    pv[100] = 8
    r.sync(s1)
    done("pinned_source_rewritten_early")
    pv[:] = 7
    r.copy(d, p, 4096, H2D, s1)
    r.sync(s1)
    pv[100] = 8
    done("pinned_source_rewritten_after_sync")
    # a download read before the synchronisation shows poison, after it the bytes
    r.memset(d, 0x11, 4096, s1)
    r.copy(p, d, 4096, D2H, s1)
    early = int(pv[0]), int(pv[4095])
    r.sync(s1)
    done("download_read_early", early=early, late=(int(pv[0]), int(pv[4095])))
    # ... into pageable memory the copy returns with the bytes
    host = np.zeros(4096, np.uint8)
    r.copy(host.ctypes.data, d, 4096, D2H, s1)
    done("download_pageable", got=(int(host[0]), int(host[4095])), pending=L.hm_pending_on(vp(d)))
    # a copy / memset one byte past its block
    blk = r.malloc(4096)
    r.memset(blk, 0, 4097, s1)
    done("memset_one_past")
    src = np.zeros(4097, np.uint8)
    r.copy(blk, src.ctypes.data, 4097, H2D, s1)
    done("copy_one_past")
    r.copy(blk + 1, src.ctypes.data, 4095, H2D, s1)
    done("copy_to_the_last_byte")
    r.sync(s1)
    # use after hipFree
    r.ok(L.hipFree(vp(blk)))
    r.memset(blk, 0, 16, s1)
    done("use_after_free")
    # hipHostFree under a pending copy
    p2, pv2 = r.pinned(4096)
    r.copy(d, p2, 4096, H2D, s1)
    r.ok(L.hipHostFree(vp(p2)))
    r.sync(s1)
    done("host_free_under_pending_copy")
    p3, _ = r.pinned(4096)
    r.copy(d, p3, 4096, H2D, s1)
    r.sync(s1)
    r.ok(L.hipHostFree(vp(p3)))
    done("host_free_after_sync")
    # hipHostUnregister under a pending download
    reg = np.zeros(8192, np.uint8)
    r.ok(L.hipHostRegister(vp(reg.ctypes.data), 8192, 0))
    r.copy(reg.ctypes.data, d, 4096, D2H, s1)
    r.ok(L.hipHostUnregister(vp(reg.ctypes.data)))
    r.sync(s1)
    done("unregister_under_pending_download", untouched=bool((reg[:4096] == POISON).all()))
    # launches: a pointer argument, a pointer inside a struct, a pointer inside a record a pointer argument names
    r.memset(d, 1, 8192, s1)
    r.launch("k_direct", s2, ("ptr", d))
    done("launch_pointer_unordered")
    r.sync(s1), r.sync(s2)
    r.copy(d2, d, 4096, D2D, s1)
    r.launch("k_reads", s2, ("cptr", d))
    done("launch_const_pointer_beside_a_read")
    r.sync(s1), r.sync(s2)
    st = (C.c_uint64 * 4)(5, d, 0, 9)
    r.memset(d, 1, 8192, s1)
    r.launch("k_struct", s2, ("bytes", st))
    done("launch_struct_word_unordered")
    r.sync(s1), r.sync(s2)
    jobs = r.malloc(4096)
    rec = np.zeros(64, np.uint64)
    rec[3] = d
    r.copy(jobs, rec.ctypes.data, 512, H2D, s2)
    r.memset(d, 1, 8192, s1)
    r.launch("k_jobs", s2, ("cptr", jobs))
    done("launch_record_word_unordered")
    r.sync(s1), r.sync(s2)
    r.memset(d, 1, 8192, s1)
    r.record(e, s1)
    r.wait(s2, e)
    r.launch("k_jobs", s2, ("cptr", jobs))
    done("launch_record_word_ordered")
    r.sync(s1), r.sync(s2)
    r.launch("k_host", s1, ("cptr", host.ctypes.data))
    done("launch_reads_pageable_memory")
    r.launch("k_pinned", s1, ("cptr", p))
    done("launch_reads_page_locked_memory")
    r.sync(s1)
    out["pending_at_end"] = L.hm_pending_total()
    return out


# ---------------------------------------------------------------------------------------------------- b. the pool ----
def books(c):
    b = (sz * 3)()
    assert model().nrq_dev_pool_books(c._h, b) == 0
    return tuple(int(x) for x in b)


def device_blocks():
    return counters()["live"]


def group_pool():
    model()
    out = {}
    hazards()
    c = nanorq_amd.Context(0)
    base_live = device_blocks()
    # reuse only within the 1.25 x + 64 KiB rule (sizes round up to 4 KiB)
    S = 1 << 20
    a = c.alloc(S)
    c.free(a)
    rule = []
    for req in (S, S - 4096, 1, (S - 65536) * 4 // 5, (S - 65536) * 4 // 5 - 8192, S + 1):
        want = max(req, 16) + 4095 & ~4095
        expect = want <= S <= want + want // 4 + 65536
        b = c.alloc(req)
        blk = block_of(b)
        rule.append(dict(req=req, expect_reuse=expect, reused=b == a, block_bytes=blk[1], books=books(c)))
        c.free(b)
        if b != a:           # (leave only the first block cached for the next request)
            keep = c.alloc(S)
            assert keep == a
            model().nrq_dev_trim(c._h)
            c.free(keep)
    out["rule"] = rule
    # the books after a trim: nothing cached, the handed-out blocks still owned, the model agrees
    x, y = c.alloc(10000), c.alloc(300000)
    c.free(x)
    before = books(c)
    assert model().nrq_dev_trim(c._h) == 0
    out["trim"] = dict(before=before, after=books(c), live_after=device_blocks() - base_live, y_alive=block_of(y) is not None,
                       x_alive=block_of(x) is not None)
    c.free(y)
    model().nrq_dev_trim(c._h)
    # an injected failure of the allocation: an error, no block, the books as before, the next call succeeds
    inj = []
    for n in (1, 2, 3):  # (the call's first checked runtime call, the allocation itself, and one call too late)
        model().nrq_dev_trim(c._h)
        b0 = books(c)
        c.set_option("fail_after", n)
        try:
            c.free(c.alloc(123456))
            failed = False
        except nanorq_amd.binding.NrqError:
            failed = True
        c.set_option("fail_after", 0)
        b1 = books(c)
        p = c.alloc(123456)
        inj.append(dict(n=n, failed=failed, books_before=b0, books_after=b1, retry_ok=block_of(p) is not None))
        c.free(p)
    out["inject"] = inj
    # a second free of the same block is refused: an error, no second cache entry, the block is handed out once
    p = c.alloc(50000)
    c.free(p)
    b0 = books(c)
    try:
        c.free(p)
        refused, msg = False, ""
    except nanorq_amd.binding.NrqError as e:
        refused, msg = True, str(e)
    b1 = books(c)
    q1, q2 = c.alloc(50000), c.alloc(50000)
    out["double_free"] = dict(refused=refused, msg=msg, books_before=b0, books_after=b1, q1_is_p=q1 == p, q2_is_p=q2 == p)
    try:
        c.free(q1 + 4096)
        inner = False
    except nanorq_amd.binding.NrqError:
        inner = True
    out["free_of_an_inner_address_refused"] = inner
    c.free(q1), c.free(q2)
    # one block never has two live owners: a random walk of allocations and frees
    rng = np.random.default_rng(11)
    live = {}
    overlaps = short = 0
    for step in range(600):
        if live and rng.random() < 0.45:
            k = list(live)[int(rng.integers(len(live)))]
            c.free(k)
            del live[k]
        else:
            n = int(rng.choice([1, 4096, 5000, 70000, 300000, 1 << 20])) + int(rng.integers(0, 9000))
            p = c.alloc(n)
            blk = block_of(p)
            short += blk is None or blk[0] != p or blk[1] < n
            overlaps += any(p < q + m and q < p + n for q, m in live.items())
            live[p] = n
        if step % 97 == 0:
            model().nrq_dev_trim(c._h)
    out["walk"] = dict(overlaps=int(overlaps), short=int(short), books=books(c), live=len(live))
    # destroy with blocks outstanding: everything goes back
    c.close()
    out["destroy"] = dict(live_after=device_blocks() - base_live)
    hz = hazards()
    out["hazards"] = brief(hz)
    return out


# ------------------------------------------------------------------------------------- c. the call that faulted ----
class Checked:
    """gpu_support bound to one context whose downloads are checked against the model's allocation table, and whose buffers
    are checked for pending work behind every sync"""

    def __init__(self, kind):
        import gpu_support
        self.G = gpu_support.bound(kind)
        self.c = self.G.ctx()
        self.bad_downloads = []
        self.pending_after_sync = []
        self.blocks = set()
        self.calls = 0
        c = self.c
        alloc, free, download, sync = c.alloc, c.free, c.download, c.sync

        def alloc_(n):
            p = alloc(n)
            self.blocks.add(p)
            return p

        def free_(p):
            self.blocks.discard(p)
            return free(p)

        def download_(p, n):
            blk = block_of(p)
            if blk is None or blk[2] != 0 or p + n > blk[0] + blk[1]:
                self.bad_downloads.append((p, n, blk))
            return download(p, n)

        def sync_():
            sync()
            self.calls += 1
            for p in self.blocks:
                k = model().hm_pending_on(vp(p))
                if k:
                    self.pending_after_sync.append((self.calls, p, k))

        c.alloc, c.free, c.download, c.sync = alloc_, free_, download_, sync_


def random_shapes(W, seed, trials=30):
    """the calls tests/test_gpu_fuzz.py::_random_shapes makes for `seed` (the same generator draws), without its comparisons:
    kernels do not run here"""
    G, c = W.G, W.c
    rng = np.random.default_rng(4000 + seed)
    host_planned = decodes = 0
    for trial in range(trials):
        K = int(rng.choice([1, 2, 7, 10, 11, 26, 55, 100, 101, 257, 400, 777, 1024, 1500, 2049, 2600, 3100]))
        T = int(rng.choice([1, 2, 3, 5, 8, 15, 16, 17, 31, 40, 64, 100, 128, 129, 200, 272]))
        nblk = int(rng.choice([1, 2, 3, 7, 8, 9, 16, 33]))
        if K * T * nblk > 24 << 20:
            nblk = max(1, (24 << 20) // (K * T))
        p = float(rng.choice([0.02, 0.1, 0.3, 0.6]))
        oh = int(rng.choice([0, 0, 1, 2, 5]))
        src = np.stack([payload(K * T, seed=seed * 100 + trial, block=b).reshape(K, T) for b in range(nblk)])
        lost = [loss_pattern(K, p, seed=seed * 977 + trial, block=b) for b in range(nblk)]
        nrep = max(len(x) for x in lost) + oh
        esis = np.arange(K, K + nrep, dtype=np.uint32)
        rep, inter = G.gpu_encode(src, K, T, esis, want_inter=True)
        rng.integers(nblk)  # (the block the GPU test compares with the oracle: the draw keeps the sequence)
        work = src.copy()
        for b in range(nblk):
            work[b][lost[b]] = 0x77
        use = [len(x) + (oh if len(x) else 0) for x in lost]
        st, out, _ = G.gpu_decode(work, K, T, lost, [esis[:n] for n in use], [rep[b][:use[b]] for b in range(nblk)])
        s = c.stats()
        decodes += 1
        host_planned += s["planner"] == 0
        # what travels by copies alone: a block no kernel touched comes back as it went up
        assert all(np.array_equal(out[b], work[b]) for b in range(nblk) if not len(lost[b])), (K, T, nblk)
    return dict(decodes=decodes, host_planned=int(host_planned))


def fuzz0(kinds=("forced", "default")):
    out = {}
    for kind in kinds:
        W = Checked(kind)
        r = random_shapes(W, 0)
        r.update(bad_downloads=W.bad_downloads, pending_after_sync=W.pending_after_sync[:8], syncs=W.calls)
        out[kind] = r
    return out


def group_fuzz0():
    model()
    hazards()
    out = fuzz0()
    out["hazards"] = brief(hazards())
    out["counters"] = counters()
    return out


# --------------------------------------------------------------------------------- d. what nrq_ctx_sync promises ----
def sync_scenarios(c, device_planner):
    """encode / decode / nrq_precalculate / nrq_decode_plan_ahead + decode on context c: per step, the operations pending on the
    three buffers the caller passed in, before and after nrq_ctx_sync"""
    out = {}
    K, T, nblk = 300, 64, 5
    L_ = nanorq_amd.params(K)["L"]
    src = np.stack([payload(K * T, seed=3, block=b).reshape(K, T) for b in range(nblk)])
    lost = [loss_pattern(K, 0.1, seed=5, block=b) for b in range(nblk)]
    nrep = max(len(x) for x in lost) + 2
    esis = np.arange(K, K + nrep, dtype=np.uint32)
    d_src, d_rep, d_int = c.alloc(nblk * K * T), c.alloc(nblk * nrep * T), c.alloc(nblk * L_ * T)
    bufs = (d_src, d_rep, d_int)

    def pend():
        return [model().hm_pending_on(vp(p)) for p in bufs]

    c.upload(d_src, src)
    # nrq_precalculate, then the encode that uses the plan
    c.precalculate(K)
    c.encode_blocks(K, T, nblk, d_src, K * T, d_rep, nrep * T, esis, d_int, L_ * T)
    mid = pend()
    c.sync()
    out["encode"] = dict(before_sync=mid, after_sync=pend(), planner=c.stats()["planner"])
    la = np.zeros((nblk, max(len(x) for x in lost)), np.uint32)
    for b in range(nblk):
        la[b, :len(lost[b])] = lost[b]
    nl = np.array([len(x) for x in lost], np.uint32)
    re = np.tile(esis, (nblk, 1))
    st = c.decode_blocks(K, T, nblk, d_src, K * T, la, nl, re, nl + 2, d_rep, nrep * T, d_int, L_ * T)
    mid = pend()
    c.sync()
    out["decode"] = dict(before_sync=mid, after_sync=pend(), status=[int(x) for x in st], planner=c.stats()["planner"])
    # nrq_decode_plan_ahead followed by the decode it belongs to, with the stream kept busy and never waited for in between: the
    # planner streams take turns, the arena sets go round (three), a set is written again while its last solve may still run
    ahead = []
    for rnd in range(5):
        c.memset(d_rep, rnd, nblk * nrep * T)
        c.decode_plan_ahead(K, T, nblk, d_src, K * T, la, nl, re, nl, nl + 2, d_rep, nrep * T)
        c.encode_blocks(K, T, nblk, d_src, K * T, d_rep, nrep * T, esis, d_int, L_ * T)   # (beside the planner run)
        st, used = c.decode_blocks_lazy(K, T, nblk, d_src, K * T, la, nl, re, nl, nl + 2, d_rep, nrep * T)
        ahead.append(dict(status=[int(x) for x in st], plan_ahead=c.stats()["plan_ahead"], planner=c.stats()["planner"]))
    mid = pend()
    c.sync()
    out["plan_ahead"] = dict(before_sync=mid, after_sync=pend(), rounds=ahead)
    # two runs issued ahead, consumed in order; then one issued and never consumed
    c.decode_plan_ahead(K, T, nblk, d_src, K * T, la, nl, re, nl, nl + 2, d_rep, nrep * T)
    c.decode_plan_ahead(K, T, nblk, d_src, K * T, la, nl, re, nl, None, d_rep, nrep * T, d_int, L_ * T)
    st1, _ = c.decode_blocks_lazy(K, T, nblk, d_src, K * T, la, nl, re, nl, nl + 2, d_rep, nrep * T)
    st2 = c.decode_blocks(K, T, nblk, d_src, K * T, la, nl, re, nl, d_rep, nrep * T, d_int, L_ * T)
    two = c.stats()["plan_ahead"]
    c.decode_plan_ahead(K, T, nblk, d_src, K * T, la, nl, re, nl, nl + 2, d_rep, nrep * T)
    c.sync()
    out["plan_ahead_two_deep"] = dict(after_sync=pend(), status=[int(x) for x in st1] + [int(x) for x in st2], plan_ahead=two)
    for p in bufs:
        c.free(p)
    return out


def group_sync():
    model()
    hazards()
    out = {}
    for name, dev in (("host_planner", False), ("device_planner", True)):
        c = nanorq_amd.Context(0)
        c.set_planner(dev)
        c.set_option("host_plan_auto", 0)
        out[name] = sync_scenarios(c, dev)
        c.close()
        out[name]["hazards"] = brief(hazards())
    out["counters"] = counters()
    return out


# ------------------------------------------------------------------ d2. a launch that is refused starts nothing ----
def group_refusal():
    """K = 3000 with every column of V forced inactive (the option plan_force_inact: 3135 inactive columns, 98 W words) on 4-byte
    strips: the tables of the split solve's back-substitution would take 196 KiB of LDS.  The decode must come back with the
    library's status for it and NO kernel launched; the context then decodes the same blocks as ever."""
    model()
    hazards()
    K, T, nblk = 3000, 48, 2
    c = nanorq_amd.Context(0)
    c.set_planner(False)
    c.set_option("max_wb", 4)
    src = np.stack([payload(K * T, seed=9, block=b).reshape(K, T) for b in range(nblk)])
    lost = loss_pattern(K, 0.1, seed=K + 17)
    la, nl = np.tile(lost, (nblk, 1)), np.full(nblk, len(lost), np.uint32)
    re = np.tile(np.arange(K, K + len(lost) + 2, dtype=np.uint32), (nblk, 1))
    d_src, d_rep = c.alloc(nblk * K * T), c.alloc(nblk * re.shape[1] * T)
    c.upload(d_src, src)
    c.sync()
    out = {}
    c.set_option("plan_force_inact", nanorq_amd.params(K)["W"])
    before = counters()["launches"]
    try:
        c.decode_blocks(K, T, nblk, d_src, K * T, la, nl, re, nl + 2, d_rep, re.shape[1] * T)
        out["error"] = None
    except nanorq_amd.NrqError as e:
        out["error"] = str(e)
    out["launches_of_the_refused_call"] = counters()["launches"] - before
    c.sync()
    c.set_option("plan_force_inact", 0)
    st = c.decode_blocks(K, T, nblk, d_src, K * T, la, nl, re, nl + 2, d_rep, re.shape[1] * T)
    s = c.stats()
    out["launches_of_the_next_call"] = counters()["launches"] - before
    out["next"] = dict(status=[int(x) for x in st], strip_bytes=s["strip_bytes"], backsub_strip=s["backsub_strip"], u=s["u"])
    c.sync()
    c.free(d_src); c.free(d_rep)
    c.close()
    out["hazards"] = brief(hazards())
    return out


# ------------------------------------------------------------------- g. a context on a stream of the caller's own ----
def caller_ctx(r, device_planner):
    """a context on a fresh model stream (every other group's contexts live on stream 0, where an operation the library puts on
    stream 0 by mistake IS in stream order)"""
    s = r.stream()
    c = nanorq_amd.Context(0, s)
    c.set_planner(device_planner)
    return c, s


def more_scenarios(c, r):
    """on context c: the device build of an encode plan, nrq_decode_plan_ahead on one block list, a decode whose blocks go out in
    two lists, and the row movers / the control copy on the stream selectors 0 .. 3 over buffers the context's stream has just
    written.  Returns what each step saw."""
    L = r.L
    out = {}
    # the encode plan built on the device (the planner kernel on a stream of the context's own, the encode behind it)
    K, T, nblk = 300, 32, 3
    L_ = nanorq_amd.params(K)["L"]
    src = np.stack([payload(K * T, seed=4, block=b).reshape(K, T) for b in range(nblk)])
    esis = np.arange(K, K + 20, dtype=np.uint32)
    d_src, d_rep, d_int = c.alloc(nblk * K * T), c.alloc(nblk * 20 * T), c.alloc(nblk * L_ * T)
    c.upload(d_src, src)
    c.set_option("encplan_dev_min_l", 1)
    for rnd in range(3):
        c.clear_plan_cache()
        c.memset(d_rep, rnd, nblk * 20 * T)
        c.precalculate(K)
        c.encode_blocks(K, T, nblk, d_src, K * T, d_rep, 20 * T, esis, d_int, L_ * T)
    out["encplan"] = dict(encplan_device=c.stats()["encplan_device"])
    c.set_option("encplan_dev_min_l", 12000)   # (its default)
    c.sync()
    # two lists: receptions that grow heavier over the batch, the LDS bound lowered until some blocks' images no longer fit
    K, T, nblk = 1000, 32, 8
    src = np.stack([payload(K * T, seed=6, block=b).reshape(K, T) for b in range(nblk)])
    lost = [loss_pattern(K, 0.10 + 0.5 * b / nblk, seed=11, block=b) for b in range(nblk)]
    nrep = max(len(x) for x in lost) + 2
    la = np.zeros((nblk, max(len(x) for x in lost)), np.uint32)
    for b in range(nblk):
        la[b, :len(lost[b])] = lost[b]
    nl = np.array([len(x) for x in lost], np.uint32)
    re = np.tile(np.arange(K, K + nrep, dtype=np.uint32), (nblk, 1))
    e_src, e_rep = c.alloc(nblk * K * T), c.alloc(nblk * nrep * T)
    c.upload(e_src, src)
    two = None
    for kb in range(160, 8, -4):
        c.set_option("lds_max", kb * 1024)
        c.memset(e_rep, kb, nblk * nrep * T)
        try:
            st = c.decode_blocks(K, T, nblk, e_src, K * T, la, nl, re, nl + 2, e_rep, nrep * T)
        except nanorq_amd.NrqError:
            break
        s_ = c.stats()
        if 0 < s_["blocks_b"] < nblk:
            two = dict(lds_max=kb * 1024, blocks_b=s_["blocks_b"], strip_bytes=s_["strip_bytes"], strip_bytes_b=s_["strip_bytes_b"],
                       status=[int(x) for x in st])
            # ... and once more with the planner run issued ahead
            c.decode_plan_ahead(K, T, nblk, e_src, K * T, la, nl, re, nl + 2, None, e_rep, nrep * T)
            c.memset(e_rep, 1, nblk * nrep * T)
            c.decode_blocks(K, T, nblk, e_src, K * T, la, nl, re, nl + 2, e_rep, nrep * T)
            two["plan_ahead"] = c.stats()["plan_ahead"]
            break
    c.set_option("lds_max", 0)
    out["two_lists"] = two
    c.sync()
    # rows by address list and the control copy, selectors 0 .. 3: each on buffers the context's stream wrote last, ordered by the
    # caller's event (nrq_event_record on selector 0, nrq_stream_wait on the selector's stream) -- and back
    L.nrq_scatter_symbols.argtypes = [vp, C.c_int, vp, C.c_uint32, C.c_uint32, vp]
    L.nrq_move_rows_dev.argtypes = [vp, C.c_int, vp, C.c_uint32, C.c_uint32]
    L.nrq_ctl_copy.argtypes = [vp, C.c_int, vp, vp, sz]
    L.nrq_event_new.argtypes = [vp, C.POINTER(vp)]
    L.nrq_event_record.argtypes = [vp, vp, C.c_int]
    L.nrq_stream_wait.argtypes = [vp, C.c_int, vp]
    L.nrq_event_free.argtypes = [vp]
    L.nrq_stream_sync.argtypes = [vp, C.c_int]
    n, T = 64, 48
    blob, rows, rows2, pairs = c.alloc(n * T), c.alloc(n * T), c.alloc(n * T), c.alloc(n * 16)
    pin, pv = r.pinned(n * 16)
    ev = vp()
    assert L.nrq_event_new(c._h, C.byref(ev)) == 0
    movers = []
    for sel in range(4):
        dst = (rows + np.arange(n, dtype=np.uint64)[::-1] * T).astype(np.uint64)
        pv.view(np.uint64)[:] = np.stack([rows + np.arange(n, dtype=np.uint64) * T, rows2 + np.arange(n, dtype=np.uint64) * T], 1).reshape(-1)
        c.memset(blob, 0x20 + sel, n * T)          # the context's stream writes the buffers ...
        c.memset(rows, 0, n * T)
        c.memset(rows2, 0, n * T)
        assert L.nrq_event_record(c._h, ev, 0) == 0 and L.nrq_stream_wait(c._h, sel, ev) == 0
        rc = [L.nrq_ctl_copy(c._h, sel, vp(pairs), vp(pin), n * 16),            # ... the selector's stream moves them ...
              L.nrq_scatter_symbols(c._h, sel, vp(blob), n, T, dst.ctypes.data_as(vp)),
              L.nrq_move_rows_dev(c._h, sel, vp(pairs), n, T)]
        assert L.nrq_event_record(c._h, ev, sel) == 0 and L.nrq_stream_wait(c._h, 0, ev) == 0
        got = c.download(rows2, n * T)             # ... and the context's stream reads the result
        movers.append(dict(sel=sel, rc=rc, moved=bool((got == 0x20 + sel).all())))
        assert L.nrq_stream_sync(c._h, sel) == 0   # (the pinned list is rewritten in the next round)
    out["movers"] = movers
    L.nrq_event_free(ev)
    for p in (d_src, d_rep, d_int, e_src, e_rep, blob, rows, rows2, pairs):
        c.free(p)
    return out


def set_stream_scenario(r):
    """nrq_ctx_set_stream to a second model stream between two calls that touch the same buffers, and back to stream 0"""
    c, s1 = caller_ctx(r, False)
    s2 = r.stream()
    K, T, nblk = 300, 64, 4
    L_ = nanorq_amd.params(K)["L"]
    src = np.stack([payload(K * T, seed=3, block=b).reshape(K, T) for b in range(nblk)])
    esis = np.arange(K, K + 30, dtype=np.uint32)
    d_src, d_rep, d_int = c.alloc(nblk * K * T), c.alloc(nblk * 30 * T), c.alloc(nblk * L_ * T)
    c.upload(d_src, src)
    pend = []
    for st in (s2, 0, s1):
        c.encode_blocks(K, T, nblk, d_src, K * T, d_rep, 30 * T, esis, d_int, L_ * T)
        c.memset(d_src, 1, nblk * K * T)
        before = model().hm_pending_on(vp(d_rep))
        c.set_stream(st)
        pend.append((before, model().hm_pending_on(vp(d_rep))))
        c.memset(d_rep, 2, nblk * 30 * T)
        c.encode_blocks(K, T, nblk, d_src, K * T, d_rep, 30 * T, esis, d_int, L_ * T)
    c.sync()
    for p in (d_src, d_rep, d_int):
        c.free(p)
    c.close()
    return dict(pending_before_and_after_set_stream=pend)


def group_callerstream():
    r = Rt()
    hazards()
    out = {}
    for name, dev in (("host_planner", False), ("device_planner", True)):
        c, _ = caller_ctx(r, dev)
        c.set_option("host_plan_auto", 0)
        res = sync_scenarios(c, dev)
        res["more"] = more_scenarios(c, r)
        c.set_option("host_plan_auto", 1)
        W = Checked(c)
        f = random_shapes(W, 0, trials=8)
        f.update(bad_downloads=W.bad_downloads, pending_after_sync=W.pending_after_sync[:8], syncs=W.calls)
        res["fuzz"] = f
        c.close()
        res["hazards"] = brief(hazards())
        out[name] = res
    out["set_stream"] = set_stream_scenario(r)
    out["set_stream"]["hazards"] = brief(hazards())
    # the detector on the library's own pattern: a blocking copy goes to stream 0, whatever stream the context is on
    det = {}

    def done(name):
        det[name] = dict(kinds=[h["kind"] for h in hazards(clear=False)], text=brief(hazards()))

    s1 = r.stream()
    d = r.malloc(4096)
    host = np.zeros(4096, np.uint8)
    r.launch("k_reads_table", s1, ("cptr", d))
    r.ok(r.L.hipMemcpy(vp(d), vp(host.ctypes.data), 4096, H2D))
    done("blocking_copy_beside_a_kernel_on_the_context_stream")
    r.sync(s1)
    r.launch("k_reads_table", s1, ("cptr", d))
    r.sync(s1)
    r.ok(r.L.hipMemcpy(vp(d), vp(host.ctypes.data), 4096, H2D))
    done("blocking_copy_behind_a_stream_synchronisation")
    r.launch("k_reads_table", s1, ("cptr", d))      # (the blocking copy has returned: the host has waited for it)
    done("kernel_behind_a_blocking_copy")
    r.sync(s1)
    out["detector"] = det
    out["counters"] = counters()
    out["pending_at_end"] = model().hm_pending_total()
    return out


GROUPS = {"detector": group_detector, "callerstream": group_callerstream, "pool": group_pool, "fuzz0": group_fuzz0, "sync": group_sync, "refusal": group_refusal}


if __name__ == "__main__":
    import object_model_scenarios as O  # noqa: E402  (groups e and f: the object layer under fault injection)
    GROUPS.update(O.groups(sys.modules[__name__]))
    res = GROUPS[sys.argv[1]]()
    print("RESULT " + json.dumps(res, default=str))
