"""Test support: one encode / decode call as the host would launch it, run by tests/emu/launch_emu.cpp on fenced memory.

Every array the solve launch reads or writes gets an anonymous mapping of its own between two pages nobody may touch, at exactly
the size the host gives it (out_slots[]: the formula of the host site the case mirrors).  A case runs twice: every array ending in
front of its upper page (side 0), and every array beginning right behind its lower page (side 1; `mis` bytes behind it for the
cases whose rows are to be unaligned).  The launch record comes from solve_lists / solve_shape on the call's real plan headers.
Results are compared with the oracle byte for byte; rows the call must not write keep their prefill."""
import ctypes as C

import numpy as np

import nanorq_amd
from emu_support import ROW_ZERO, Job, decode_setup, pemu
from nanorq_amd import build as nbuild
from util import loss_pattern, payload, received_set, undecodable

NCU = 256  # compute units of the MI355X: what the context hands solve_shape
PREFILL = 0xCD


class LaunchRec(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("err two_lists wb NT WV G AL lds_bytes split by_block nstrips spl grid lsub nslots stage_stride "
                                          "ostage_stride res_elems backsub_strip backsub_nsb nchunks pad").split()] + \
               [("ybuf_stride", C.c_uint64), ("stage_bytes", C.c_uint64)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_ if n != "pad"}


_L = None


def lemu():
    global _L
    if _L is None:
        L = C.CDLL(nbuild.build_launch_emu())
        L.lemu_fenced.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_size_t]
        L.lemu_fenced.restype = C.c_void_p
        L.lemu_check_margins.restype = C.c_char_p
        L.lemu_set_case.argtypes = [C.c_char_p]
        L.lemu_tuning_new.restype = C.c_void_p
        L.lemu_tuning_free.argtypes = [C.c_void_p]
        L.lemu_tuning_set.argtypes = [C.c_void_p, C.c_char_p, C.c_longlong]
        L.lemu_shape.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int,
                                 C.POINTER(LaunchRec)]
        L.lemu_store_slack.restype = C.c_uint32
        L.lemu_run.argtypes = [C.POINTER(LaunchRec), C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        _L = L
    return _L


FORCED = {"tiny_any": 1}  # what gpu_support.ctx("forced") sets that solve_shape reads (host_plan_auto / plan_pack: the planner's)
DEFAULT = {}


def r16(x):
    return (x + 15) & ~15


class Arena:
    """the fenced arrays of one run: place(name, bytes-like or size) -> numpy view on the mapping"""

    def __init__(self, side, mis=0):
        self.side, self.mis = side, mis

    def place(self, name, data, fill=None, mis=None):
        L = lemu()
        if isinstance(data, (int, np.integer)):
            n, src = int(data), None
        else:
            src = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
            n = src.size
        p = L.lemu_fenced(name.encode(), n, self.side, self.mis if mis is None else mis)
        assert p, "no memory for " + name
        a = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(max(n, 1),))[:n]
        if src is not None:
            a[:] = src
        elif fill is not None:
            a[:] = fill
        return a, p


_KC, _ENCPLAN = {}, {}


def kconst(K):
    if K not in _KC:
        _KC[K] = nanorq_amd.host_kconst(K)
    return _KC[K]


def encode_plan(K, extra_inact=0):
    """the host's encode plan; extra_inact: with that many columns more inactive from the start (the option plan_force_inact)"""
    if (K, extra_inact) not in _ENCPLAN:
        Kp = nanorq_amd.params(K)["Kp"]
        _ENCPLAN[(K, extra_inact)] = nanorq_amd.host_plan(K, np.arange(Kp, dtype=np.uint32), kconst(K), extra_inact=extra_inact)
    return _ENCPLAN[(K, extra_inact)]


def out_lists(orc, K, isis, plan):
    """build_out_lists (nrq_device.hip): cptr u32[n + 1], cols u16[] through the plan's colslot[]"""
    hdr = nanorq_amd.plan_header(plan)
    colslot = np.frombuffer(plan, np.uint16, count=hdr["L"], offset=hdr["off_colslot"])
    cptr, cols = [0], []
    for x in isis:
        cols += [int(colslot[c]) for c in orc.lt_columns(K, int(x))]
        cptr.append(len(cols))
    return np.array(cptr, np.uint32), np.array(cols, np.uint16)


def tuning(opts):
    L = lemu()
    t = L.lemu_tuning_new()
    for k, v in opts.items():
        assert L.lemu_tuning_set(t, k.encode(), v) == 0, k
    return t


def shape(opts, plan_ptrs, can_split, nblk, T, max_out, io_aligned):
    L = lemu()
    t = tuning(opts)
    rec = LaunchRec()
    arr = (C.c_uint64 * len(plan_ptrs))(*plan_ptrs)
    L.lemu_shape(t, arr, len(plan_ptrs), int(can_split), nblk, T, max_out, int(io_aligned), NCU, C.byref(rec))
    L.lemu_tuning_free(t)
    return rec


def launch(rec, A, jobs, nblk, T, kc_ptr):
    L = lemu()
    stage, stage_p = A.place("staging area", int(rec.stage_bytes), fill=0x5A, mis=0)
    ybuf_p = None
    if rec.split:
        _, ybuf_p = A.place("work buffers (ybuf)", nblk * int(rec.ybuf_stride), fill=0x77, mis=0)
    jb, jobs_p = A.place("job records", bytes(jobs), mis=0)
    r = L.lemu_run(C.byref(rec), jobs_p, nblk, T, kc_ptr, stage_p, ybuf_p, A.side)
    assert r == 1, ("the launch emulation refused", r, rec.as_dict())
    bad = L.lemu_check_margins()
    assert bad is None, "bytes next to the array '%s' were written" % bad.decode()


def run_encode(orc, K, T, nblk, nrep, opts, want_inter=True, side=0, mis=0, expect=None, seed=1, lists=None, extra_inact=0):
    """One nrq_encode_blocks call (host site: encode_blocks, out_slots[] of r16(cols * 2 + NRQ_STORE_SLACK) bytes).
    extra_inact: the plan of a context with the option plan_force_inact.  Returns the launch record as a dict."""
    L = lemu()
    p = nanorq_amd.params(K)
    Lsym, Kp = p["L"], p["Kp"]
    plan = encode_plan(K, extra_inact)
    hdr = nanorq_amd.plan_header(plan)
    assert hdr["status"] == 0 and hdr["M"] == Lsym
    A = Arena(side, mis)
    esis = np.arange(K, K + nrep, dtype=np.uint32)
    if lists is None:
        cptr, cols = out_lists(orc, K, esis + (Kp - K), plan)
    else:  # made-up generated symbols: symbol q is the sum of the intermediate symbols lists[q] names (lengths no ESI has)
        assert len(lists) == nrep
        colslot = np.frombuffer(plan, np.uint16, count=Lsym, offset=hdr["off_colslot"])
        cptr = np.cumsum([0] + [len(x) for x in lists]).astype(np.uint32)
        cols = np.array([colslot[c] for x in lists for c in x], np.uint16)
    _, plan_p = A.place("plan arena", plan[:max(hdr["total_bytes"], 256)], mis=0)
    rowsrc = np.full(Lsym, ROW_ZERO, np.uint32)
    rowsrc[p["S"] + p["H"]:p["S"] + p["H"] + K] = np.arange(K, dtype=np.uint32)
    _, rowsrc_p = A.place("rowsrc", rowsrc, mis=0)
    _, cptr_p = A.place("out_cptr", cptr, mis=0)
    _, orow_p = A.place("out_row", np.arange(nrep, dtype=np.uint32), mis=0)
    slots = np.zeros(r16(cols.size * 2 + L.lemu_store_slack()), np.uint8)  # encode_blocks: total - off_cols
    slots[:cols.size * 2] = cols.view(np.uint8)
    slots[cols.size * 2:] = 0xEE  # (what the staging buffer held before: nothing may depend on it)
    _, slots_p = A.place("out_slots", slots, mis=0)
    _, kc_p = A.place("kconst", np.frombuffer(kconst(K), np.uint8), mis=0)
    src, srcs, reps, ints = [], [], [], []
    jobs = (Job * nblk)()
    bits = T
    for b in range(nblk):
        s = payload(K * T, seed=seed, block=b)
        src.append(s.reshape(K, T))
        a, sp = A.place("src[%d]" % b, s)
        srcs.append(a)
        ra, rp = A.place("rep[%d]" % b, nrep * T, fill=PREFILL) if nrep else (None, 0)
        ia, ip = A.place("inter[%d]" % b, Lsym * T, fill=PREFILL) if want_inter else (None, 0)
        reps.append(ra)
        ints.append(ia)
        bits |= sp | (rp or 0) | (ip or 0)
        j = jobs[b]
        j.plan, j.rowsrc, j.src, j.rep, j.inter, j.out = plan_p, rowsrc_p, sp, 0, ip or 0, rp or 0
        j.out_cptr, j.out_slots, j.out_row, j.nout = cptr_p, slots_p, orow_p, nrep
    io_aligned = (bits & 15) == 0  # Rows::aligned: every row of the call on a 16-byte boundary, T a multiple of 16
    rec = shape(opts, [plan_p], False, nblk, T, (Lsym if want_inter else 0) + nrep, io_aligned)
    assert rec.err == 0 and not rec.two_lists, rec.as_dict()
    if expect:
        for k, v in expect.items():
            assert getattr(rec, k) == v, (k, v, rec.as_dict())
    try:
        launch(rec, A, jobs, nblk, T, kc_p)
        for b in range(nblk):
            assert np.array_equal(srcs[b].reshape(K, T), src[b]), ("source rows of block %d were written" % b)
            r_rep, r_int, _ = orc.encode_block(src[b], K, T, esis, want_inter=want_inter or lists is not None)
            if lists is not None:
                r_rep = np.stack([np.bitwise_xor.reduce(r_int[x], axis=0) for x in lists])
            if nrep:
                assert np.array_equal(reps[b].reshape(nrep, T), r_rep), ("repair symbols", b)
            if want_inter:
                assert np.array_equal(ints[b].reshape(Lsym, T), r_int), ("intermediate symbols", b)
    finally:
        L.lemu_release_all()
    d = rec.as_dict()
    d["io_aligned"] = io_aligned
    d["u"] = hdr["u"]
    return d


def device_plan(K, lost, rep_esis, no_out_view=False):
    """the emulated device planner's arena (cut at total_bytes) and where the job's arrays lie in it (pl_final_b); no_out_view: the
    plan of a context with the option plan_no_out_view -- the arena ends behind the needed-pivot view's W rows"""
    P = pemu()
    kc = kconst(K)
    kcb = (C.c_uint8 * len(kc)).from_buffer_copy(kc)
    lost = np.ascontiguousarray(lost, np.uint32)
    rep_esis = np.ascontiguousarray(rep_esis, np.uint32)
    cap = P.emu_plan_arena_bound(K, C.addressof(kcb), max(0, len(rep_esis) - len(lost)) + 24, len(lost) + 8)
    arena = np.zeros(cap, np.uint8)
    job = Job()
    P.emu_plan_set_caps(0, 0)
    P.emu_plan_set_mode(0x800 if no_out_view else 0)
    try:
        rc = P.emu_plan(K, 0, C.addressof(kcb), lost.ctypes.data_as(C.POINTER(C.c_uint32)), len(lost),
                        rep_esis.ctypes.data_as(C.POINTER(C.c_uint32)), len(rep_esis), len(rep_esis), arena.ctypes.data, cap, 140 * 1024,
                        C.byref(job))
    finally:
        P.emu_plan_set_mode(0)
    assert rc == 0
    hdr = nanorq_amd.plan_header(arena.tobytes()[:256])
    base = arena.ctypes.data
    total = max(hdr["total_bytes"], 256)
    if hdr["status"]:
        return arena[:total].copy(), hdr, None, 0
    offs = {k: getattr(job, k) - base for k in ("rowsrc", "out_cptr", "out_slots", "out_row")}
    assert all(0 < o < total for o in offs.values()), (offs, total)
    return arena[:total].copy(), hdr, offs, int(job.nout)


def run_decode(orc, K, T, nblk, loss, overhead, opts, want_inter=False, side=0, mis=0, site="host", bad_block=None, expect=None, seed=2,
               extra_inact=0, lost_all=None, no_out_view=False):
    """One nrq_decode_blocks call.  site "host": decode_host's arrays (out_slots[] of r16(cols * 2 + NRQ_STORE_SLACK) bytes per block);
    "device": the planner's arena, cut at total_bytes, with rowsrc / out_cptr / out_row / out_slots inside it (pl_final_b).
    bad_block: that block's reception is rank deficient -- the launch must skip it and leave its rows alone.
    extra_inact (site "host"): the plans of a context with the option plan_force_inact; lost_all: every block misses these symbols
    (the option is the context's: blocks with one reception have one plan, and so one number of inactive columns).
    no_out_view (site "device", no intermediate symbols): the plans of a context with the option plan_no_out_view -- the arena's last
    part is the needed-pivot view (needslot[nneed], wneed at stride need_pad with room for every pivot), which the back-substitution
    then walks."""
    L = lemu()
    p = nanorq_amd.params(K)
    Lsym = p["L"]
    A = Arena(side, mis)
    kc = kconst(K)
    _, kc_p = A.place("kconst", np.frombuffer(kc, np.uint8), mis=0)
    dummy = np.zeros(64, np.uint32)  # decode_host's shared header of the blocks that need no work: status = 1
    dummy[1] = 1
    _, dummy_p = A.place("dummy plan header", dummy, mis=0)
    jobs = (Job * nblk)()
    blocks, plan_ptrs, max_out, bits = [], [], 0, T
    for b in range(nblk):
        src = payload(K * T, seed=seed, block=b).reshape(K, T)
        lost = undecodable(orc, K, b) if b == bad_block else lost_all if lost_all is not None else loss_pattern(K, loss, seed=seed * 31 + 5, block=b)
        oh = 0 if b == bad_block else (overhead if len(lost) else 0)
        esis = np.arange(K, K + len(lost) + oh, dtype=np.uint32)
        rep, r_int, _ = orc.encode_block(src, K, T, esis, want_inter=True)
        work = src.copy()
        work[lost] = 0x77
        wa, wp = A.place("src[%d]" % b, work)
        ra, rp = A.place("rep[%d]" % b, rep) if len(esis) else (None, 0)
        ia, ip = A.place("inter[%d]" % b, Lsym * T, fill=PREFILL) if want_inter else (None, 0)
        bits |= wp | (rp or 0) | (ip or 0)
        rx = received_set(K, lost, oh)
        syms = np.concatenate([src[rx[rx < K]], rep]) if len(esis) else src[rx[rx < K]]
        ok, _, _ = orc.decode_block(rx, syms, K, T)
        blk = dict(src=src, work=work, wa=wa, ia=ia, lost=lost, ok=ok, inter=r_int, solved=False)
        blocks.append(blk)
        j = jobs[b]
        j.plan = dummy_p
        if not len(lost):
            continue
        if site == "host":
            isis, rowsrc = decode_setup(orc, K, lost, esis)
            plan = nanorq_amd.host_plan(K, isis, kc, extra_inact=extra_inact)
            hdr = nanorq_amd.plan_header(plan)
            assert (hdr["status"] == 0) == ok, ("verdict", b, hdr["status"], ok)
            if hdr["status"]:
                continue
            _, plan_p = A.place("plan arena[%d]" % b, plan[:max(hdr["total_bytes"], 256)], mis=0)
            cptr, cols = out_lists(orc, K, lost, plan)
            _, j.rowsrc = A.place("rowsrc[%d]" % b, rowsrc, mis=0)
            _, j.out_cptr = A.place("out_cptr[%d]" % b, cptr, mis=0)
            _, j.out_row = A.place("out_row[%d]" % b, lost.astype(np.uint32), mis=0)
            slots = np.full(r16(cols.size * 2 + L.lemu_store_slack()), 0xEE, np.uint8)  # decode_host: off of the next array - off_cols
            slots[:cols.size * 2] = cols.view(np.uint8)
            _, j.out_slots = A.place("out_slots[%d]" % b, slots, mis=0)
            j.nout = len(lost)
        else:
            arena, hdr, offs, nout = device_plan(K, lost, esis, no_out_view)
            assert (hdr["status"] == 0) == ok, ("verdict", b, hdr["status"], ok)
            if hdr["status"]:
                continue
            assert nout == len(lost)
            if no_out_view:  # (the view ends the arena: the page behind it is the fence)
                assert not want_inter and hdr["off_wout"] == 0 and hdr["off_needslot"] != 0 and 0 < hdr["nneed"] <= hdr["need_pad"], hdr
                assert len(arena) == hdr["total_bytes"] == r16(hdr["off_wneed"] + 4 * hdr["wpr"] * hdr["npiv_pad"]), hdr  # (room for every pivot)
            _, plan_p = A.place("plan arena[%d] (rowsrc, out lists inside)" % b, arena, mis=0)
            j.rowsrc, j.out_cptr, j.out_row, j.out_slots = (plan_p + offs[k] for k in ("rowsrc", "out_cptr", "out_row", "out_slots"))
            j.nout = nout
        j.plan, j.src, j.rep, j.inter, j.out = plan_p, wp, rp or 0, ip or 0, wp
        plan_ptrs.append(plan_p)
        max_out = max(max_out, len(lost))
        blk["solved"], blk["u"] = True, hdr["u"]
    io_aligned = (bits & 15) == 0
    rec = shape(opts, plan_ptrs, True, nblk, T, (Lsym if want_inter else 0) + max_out, io_aligned)
    assert rec.err == 0 and not rec.two_lists, rec.as_dict()
    if expect:
        for k, v in expect.items():
            assert getattr(rec, k) == v, (k, v, rec.as_dict())
    try:
        launch(rec, A, jobs, nblk, T, kc_p)
        for b, blk in enumerate(blocks):
            got = blk["wa"].reshape(K, T)
            if not blk["solved"]:
                assert np.array_equal(got, blk["work"]), ("a block the launch must skip was written", b)
                assert blk["ia"] is None or (blk["ia"] == PREFILL).all(), ("intermediate symbols of a skipped block", b)
                continue
            keep = np.setdiff1d(np.arange(K), blk["lost"])
            assert np.array_equal(got[keep], blk["work"][keep]), ("received rows were written", b)
            assert np.array_equal(got[blk["lost"]], blk["src"][blk["lost"]]), ("recovered rows", b)
            if want_inter:
                assert np.array_equal(blk["ia"].reshape(Lsym, T), blk["inter"]), ("intermediate symbols", b)
    finally:
        L.lemu_release_all()
    d = rec.as_dict()
    d["io_aligned"] = io_aligned
    d["solved"] = sum(1 for x in blocks if x["solved"])
    d["u"] = max([x["u"] for x in blocks if x["solved"]] or [0])  # (inactive columns of the plans that ran)
    return d
