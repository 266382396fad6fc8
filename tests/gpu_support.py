"""Helpers for the -m gpu tier: run the HIP path through the C ABI with numpy in/out.

Two shared contexts: "forced" (ctx(), the options below pin the device planner and every small workgroup form) and
"default" (default_ctx(), no option set: the launch choices a product caller gets).  gpu_encode / gpu_decode take
kind= to pick one; bound(kind) gives a module-like view with the same three functions bound to it.  A third kind, "side", is a
default context created on a torch.cuda.Stream() of its own (side_stream() is that stream; new_side() makes further ones): the
null stream orders caller and library work by accident, a side stream does not (tests/test_gpu_streams.py)."""
import numpy as np

import nanorq_amd

KINDS = ("forced", "default", "side")
_CTXS = {}
_STREAMS = {}   # context -> its torch stream (kept alive as long as the context)


def _torch_up():
    # Tests that keep blocks in HBM use torch tensors.  torch brings its own copy of the HIP runtime, and it only
    # finds the GPU if it initialises BEFORE the runtime libnanorq_hip.so is linked against opens the device
    # (bench.py has the same order): bring torch up first.
    try:
        import torch
        if torch.cuda.is_available():
            torch.cuda.init()
            torch.empty(1, device="cuda")
    except ImportError:
        pass


def ctx(kind="forced"):
    if isinstance(kind, nanorq_amd.Context):   # (a context of the caller's own: gpu_encode / gpu_decode run on it)
        return kind
    c = _CTXS.get(kind)
    if c is not None:
        return c
    if kind not in KINDS:
        raise ValueError("unknown context kind %r" % kind)
    _torch_up()
    c = new_side()[0] if kind == "side" else nanorq_amd.Context(0)
    if kind == "forced":
        # the parity tests are about the DEVICE planner at every size and block count; a product context gives calls of one or two small
        # blocks to the host planner (nrq_decode_blocks_lazy "host_small"), which test_small_calls_take_the_host_planner covers
        c.set_option("host_plan_auto", 0)
        # ... and about every FORM of it: a product context gives a batch of at most one block per compute unit the 1024-thread planner
        # workgroup; the 256- and 128-thread forms that batches of thousands of small blocks use are exercised here at a few blocks
        c.set_option("plan_pack", 1)
        # ... and the single-wave solve workgroups, which a product context keeps for launches of more than ~500 strips
        c.set_option("tiny_any", 1)
    _CTXS[kind] = c
    return c


_PROBE = []     # the probe's work tensor
_REJECTED = []  # streams the probe turned down, kept alive so that torch hands out others


def shares_a_queue(s, other=None, ms=5.0):
    """Does work on stream s wait for work on `other` (default: the null stream)?  The runtime multiplexes a process's streams
    over a few hardware queues (GPU_MAX_HW_QUEUES); two streams on one queue take turns, so a kernel put on the wrong one of them
    still runs in order -- by accident, exactly what a side-stream test wants to rule out.  The probe: a few ms of passes over a
    tensor on `other`, one tiny kernel on s, wait for s: did the passes end first?"""
    import torch
    other = other or torch.cuda.default_stream()
    if not _PROBE:
        _PROBE.append(torch.zeros(16 << 20, dtype=torch.int32, device="cuda"))
        for _ in range(3):
            _PROBE[0].add_(1)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(50):
            _PROBE[0].add_(1)
        b.record()
        torch.cuda.synchronize()
        _PROBE.append(max(1, int(ms / (a.elapsed_time(b) / 50))))
    torch.cuda.synchronize()
    with torch.cuda.stream(other):
        for _ in range(_PROBE[1]):
            _PROBE[0].add_(1)
        ev = torch.cuda.Event()
        ev.record(other)
    with torch.cuda.stream(s):
        torch.zeros(1, device="cuda")
    s.synchronize()
    shared = ev.query()
    torch.cuda.synchronize()
    return shared


def new_side(tries=12):
    """(context, stream): a fresh context with no option set on a fresh torch.cuda.Stream() (non-blocking: the null stream does
    not wait for it, nor it for the null stream) -- one that does not share its hardware queue with the null stream, if `tries`
    streams yield one (side_independent(c) says whether)."""
    import torch
    _torch_up()
    for k in range(tries):
        s = torch.cuda.Stream()
        shared = shares_a_queue(s)
        if not shared:
            break
        _REJECTED.append(s)
    c = nanorq_amd.Context(0, s.cuda_stream)
    _STREAMS[c] = s
    _INDEPENDENT[c] = not shared
    return c, s


_INDEPENDENT = {}


def side_independent(c=None):
    """the side stream of c (default: of ctx("side")) was seen NOT to wait for work on the null stream"""
    return _INDEPENDENT[c or ctx("side")]


def side_stream(c=None):
    """the torch stream of a side-stream context (default: of ctx("side"))"""
    return _STREAMS[c or ctx("side")]


def default_ctx():
    """A context with no option set: the launch shapes real callers get (lone workgroups, the host planner for small calls,
    the 1024-thread planner for batches of at most one block per CU)."""
    return ctx("default")


class bound:
    """ctx / gpu_encode / gpu_decode on the context of one kind: a test body written against this module runs unchanged on it."""

    def __init__(self, kind):
        self.kind = kind

    def __repr__(self):
        return "bound(%r)" % self.kind

    def ctx(self):
        return ctx(self.kind)

    def gpu_encode(self, *a, **k):
        k.setdefault("kind", self.kind)
        return gpu_encode(*a, **k)

    def gpu_decode(self, *a, **k):
        k.setdefault("kind", self.kind)
        return gpu_decode(*a, **k)


def gpu_encode(src_blocks, K, T, esis, want_inter=False, Kp=0, kind="forced"):
    """src_blocks: [nblk, K, T] uint8 -> (repair [nblk, nrep, T], inter [nblk, L, T] or None)"""
    c = ctx(kind)
    src_blocks = np.ascontiguousarray(src_blocks, np.uint8)
    nblk = src_blocks.shape[0]
    esis = np.ascontiguousarray(esis, np.uint32)
    nrep = len(esis)
    L = nanorq_amd.params(Kp or K)["L"]
    d_src = c.alloc(nblk * K * T)
    d_rep = c.alloc(max(1, nblk * nrep * T))
    d_int = c.alloc(nblk * L * T) if want_inter else 0
    try:
        c.upload(d_src, src_blocks)
        c.memset(d_rep, 0xCD, max(1, nblk * nrep * T))
        c.encode_blocks(K, T, nblk, d_src, K * T, d_rep, nrep * T, esis, d_int, L * T, Kp=Kp)
        c.sync()
        rep = c.download(d_rep, nblk * nrep * T).reshape(nblk, nrep, T) if nrep else np.zeros((nblk, 0, T), np.uint8)
        inter = c.download(d_int, nblk * L * T).reshape(nblk, L, T) if want_inter else None
    finally:
        c.free(d_src); c.free(d_rep)
        if d_int:
            c.free(d_int)
    return rep, inter


def gpu_decode(work_blocks, K, T, lost_lists, rep_esi_lists, rep_syms_lists, want_inter=False, Kp=0, kind="forced"):
    """work_blocks: [nblk, K, T] with received source symbols in place (missing rows arbitrary).
    Returns (status[nblk], recovered blocks [nblk,K,T], inter or None)."""
    c = ctx(kind)
    work_blocks = np.ascontiguousarray(work_blocks, np.uint8)
    nblk = work_blocks.shape[0]
    lost_cap = max(1, max(len(x) for x in lost_lists))
    rep_cap = max(1, max(len(x) for x in rep_esi_lists))
    lost = np.zeros((nblk, lost_cap), np.uint32)
    resi = np.zeros((nblk, rep_cap), np.uint32)
    reps = np.zeros((nblk, rep_cap, T), np.uint8)
    for b in range(nblk):
        lost[b, :len(lost_lists[b])] = lost_lists[b]
        resi[b, :len(rep_esi_lists[b])] = rep_esi_lists[b]
        if len(rep_esi_lists[b]):
            reps[b, :len(rep_esi_lists[b])] = rep_syms_lists[b]
    nlost = np.array([len(x) for x in lost_lists], np.uint32)
    nrep = np.array([len(x) for x in rep_esi_lists], np.uint32)
    L = nanorq_amd.params(Kp or K)["L"]
    d_src = c.alloc(nblk * K * T)
    d_rep = c.alloc(nblk * rep_cap * T)
    d_int = c.alloc(nblk * L * T) if want_inter else 0
    try:
        c.upload(d_src, work_blocks)
        c.upload(d_rep, reps)
        st = c.decode_blocks(K, T, nblk, d_src, K * T, lost, nlost, resi, nrep, d_rep, rep_cap * T, d_int, L * T, Kp=Kp)
        c.sync()
        out = c.download(d_src, nblk * K * T).reshape(nblk, K, T)
        inter = c.download(d_int, nblk * L * T).reshape(nblk, L, T) if want_inter else None
    finally:
        c.free(d_src); c.free(d_rep)
        if d_int:
            c.free(d_int)
    return st, out, inter
