"""Test support: host plans at a chosen number of inactive columns (nanorq_amd.host_plan(..., extra_inact=n), the context option
"plan_force_inact"), and the table of GPU cases built on them.

The solve kernel's back-substitution picks its code by wpr = ceil(u / 32), u the inactive columns of the plan (solve_body.h
ph_backsub: unrolled classes NW = 4 / 8 / 12 / 24 and a plain loop beyond).  Receptions do not move u; inactivating n columns more
before peeling does, and changes nothing else: same rank, same solution, same verdict.  The host planner is deterministic, so a
pair (reception, n) is a fixed plan: GPU_CASES names, per form of the kernel, the n that gives each target u -- found by find_n on
the CPU, asserted again wherever a case is used (tests/test_forced_inact_emu.py on the CPU, tests/test_gpu_backsub_forms.py on the
GPU)."""
import ctypes as C

import numpy as np

import nanorq_amd
from emu_support import ROW_REP, ROW_ZERO, decode_setup
from util import loss_pattern, payload

NRQ_LDS_MAX = 163840   # launch_shape.h
WPRS = (1, 4, 5, 8, 9, 12, 13, 24, 25, 40)   # every class of ph_backsub at both of its edges, and the device planner's 40 words


def wpr_of(u):
    return max(1, (u + 31) // 32)


def nw_class(wpr):
    """the instance of backsub_fixed that ph_backsub takes (0: the plain loop)"""
    for nw in (4, 8, 12, 24):
        if wpr <= nw:
            return nw
    return 0


_KC = {}


def kconst(K):
    if K not in _KC:
        _KC[K] = nanorq_amd.host_kconst(K)
    return _KC[K]


def encode_isis(K):
    return np.arange(nanorq_amd.params(K)["Kp"], dtype=np.uint32)


def reception(orc, K, loss=0.1, overhead=2, seed=None):
    """(lost, repair ESIs, isis, rowsrc) of one decode: Bernoulli losses, repair ESIs K, K + 1, ..."""
    lost = loss_pattern(K, loss, seed=K + 17 if seed is None else seed)
    if not len(lost):
        lost = np.array([K // 2], np.uint32)
    esis = np.arange(K, K + len(lost) + overhead, dtype=np.uint32)
    isis, rowsrc = decode_setup(orc, K, lost, esis)
    return lost, esis, isis, rowsrc


def plan(K, isis, n=0):
    return nanorq_amd.host_plan(K, isis, kconst(K), extra_inact=n)


def header(K, isis, n=0):
    return nanorq_amd.plan_header(plan(K, isis, n))


def find_n(K, isis, target_u):
    """the smallest n found with header u == target_u, or None.  u(n) >= P + n and u grows with n nearly everywhere: bisect for the
    first n at or above the target, then look at its neighbours."""
    P, W = nanorq_amd.params(K)["P"], nanorq_amd.params(K)["W"]
    seen = {}

    def u(n):
        if n not in seen:
            seen[n] = header(K, isis, n)["u"]
        return seen[n]

    if u(0) == target_u:
        return 0
    if u(0) > target_u or target_u > P + W:
        return None
    lo, hi = 0, min(W, target_u - P)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if u(mid) >= target_u:
            hi = mid
        else:
            lo = mid
    for d in range(0, 48):
        for n in (hi + d, hi - d):
            if 0 <= n <= W and u(n) == target_u:
                return n
    return None


def exec_rows(plan_bytes, rowsrc, src, rep, T):
    """the M x T input of oracle.plan_exec: every row of the system with its symbol (rowsrc[]: a source row, a repair row, zero)"""
    M = nanorq_amd.plan_header(plan_bytes)["M"]
    assert len(rowsrc) == M
    din = np.zeros((M, T), np.uint8)
    for r, v in enumerate(rowsrc):
        v = int(v)
        if v == ROW_ZERO:
            continue
        din[r] = rep[v & ~ROW_REP] if v & ROW_REP else src[v]
    return din


def source_from_inter(orc, K, inter, esis):
    """symbols `esis` (source ESIs: ISI = ESI) as sums of intermediate symbols"""
    return np.stack([np.bitwise_xor.reduce(inter[orc.lt_columns(K, int(e))], axis=0) for e in esis])


# ---- the launch decisions on plan headers (launch_emu_support.shape over solve_lists / solve_shape) ----

def launch_record(plans, opts, nblk, T, max_out, io_aligned, can_split):
    """the record solve_lists / solve_shape give for these plans (one shared plan: encode; one per block: decode)"""
    import launch_emu_support as S
    bufs = [(C.c_uint8 * len(p)).from_buffer_copy(p) for p in plans]
    rec = S.shape(opts, [C.addressof(b) for b in bufs], can_split, nblk, T, max_out, io_aligned)
    return rec.as_dict()


def form_of(rec):
    """what nrq_call_stats reports of a launch record: (strip_bytes, wg_threads, backsub_strip)"""
    return (rec["wb"] * rec["G"], rec["NT"], rec["backsub_strip"])


# ---- the GPU cases ----
def _edge(b):
    """the u around the boundary between b and b + 1 W words: u % 32 = 31, 0 (b words) and 1 (b + 1 words); 31 and 1: u % 4 != 0"""
    return [32 * b - 1, 32 * b, 32 * b + 1]


# A form: K, the context options on top of the forced context of gpu_support (tiny_any, plan_pack, host_plan_auto = 0), the targets
# of u.  What solve_shape picks for a target (strip bytes, threads, the split's strip) is NOT the form's to say: it moves with u --
# the image grows -- and GPU_CASES records it per case.
FORMS = {
    "w16_big": dict(K=5200, opts={}, us=_edge(8) + _edge(12) + _edge(24)),
    "w16_k1000": dict(K=1000, opts={}, us=_edge(4) + _edge(8) + _edge(12) + _edge(24) + [1071]),   # 1071 = L: every column inactive
    "w16_k3000": dict(K=3000, opts={}, us=_edge(4) + _edge(8) + _edge(12) + _edge(24) + _edge(40)),
    "w16_k100": dict(K=100, opts={}, us=_edge(1) + _edge(2) + _edge(3) + [127, 128]),           # npiv = 128 - u: 97 .. 63, 64, 65 .. 1, 0
    "w12_k10000": dict(K=10000, opts={"max_wb": 12}, us=_edge(8) + _edge(12)),
    "w12_k5200": dict(K=5200, opts={"max_wb": 12}, us=_edge(24)),
    "w8_k15000": dict(K=15000, opts={"max_wb": 8}, us=_edge(12) + _edge(24) + [1280, 1281]),
    "w8_k10000": dict(K=10000, opts={"max_wb": 8}, us=_edge(8)),
    "w8_k1000": dict(K=1000, opts={"max_wb": 8}, us=_edge(4) + _edge(8) + _edge(12) + _edge(24) + [1071]),
    "w4_k3000": dict(K=3000, opts={"max_wb": 4}, us=_edge(20) + _edge(40)),
    "w2_k3000": dict(K=3000, opts={"max_wb": 2}, us=_edge(20) + _edge(40)),
}
TS = (48, 40)      # three whole 16-byte strips; a partial last strip
NBLK = 2
NREP = 4
GPU_FORCED = {"tiny_any": 1}   # what the forced context sets that solve_shape reads


def gpu_reception(orc, K):
    """the one reception all blocks of a GPU decode case share (the option is the context's: one n for every block of a call)"""
    return reception(orc, K, 0.1, 2)


def gpu_source(K, T, nblk=NBLK):
    """block b of a case at symbol size T: the first T byte columns of its 48-byte rows (one oracle run serves both sizes: the
    code works on every byte column alike)"""
    return np.stack([payload(K * 48, seed=K + 3, block=b).reshape(K, 48)[:, :T] for b in range(nblk)])


def calls_of(index):
    """the three calls of GPU case number `index`: (kind, T, want_inter) -- both symbol sizes and both decode forms in every case,
    dealt the other way round in every second one"""
    a, b = TS if index % 2 == 0 else TS[::-1]
    return (("encode", a, True), ("decode", b, False), ("decode", a, True))


def case_record(orc, form, n_enc, n_dec, kind, T, want_inter):
    """(strip_bytes, wg_threads, backsub_strip, lds_bytes) solve_shape picks for one call of a case"""
    f = FORMS[form]
    K, opts = f["K"], dict(GPU_FORCED, **f["opts"])
    L = nanorq_amd.params(K)["L"]
    if kind == "encode":
        rec = launch_record([plan(K, encode_isis(K), n_enc)], opts, NBLK, T, L + NREP, T % 16 == 0, False)
    else:
        lost, _, isis, _ = gpu_reception(orc, K)
        rec = launch_record([plan(K, isis, n_dec)] * NBLK, opts, NBLK, T, (L if want_inter else 0) + len(lost), T % 16 == 0, True)
    assert rec["err"] == 0 and not rec["two_lists"], rec
    return form_of(rec) + (rec["lds_bytes"],)


# (form, u, n for the encode plan, n for the decode plan of gpu_reception, then what the call stats must say: strip_bytes, wg_threads,
# backsub_strip).  Printed by search_cases; test_forced_inact_emu.py holds every row against host_plan and solve_shape again.
# Where the image of a form outgrows its width or its workgroup the launch moves on, and the row says where to: K = 1000 and 3000
# leave the 256-thread workgroup once the 16-byte image passes half of the LDS (u = 767 / 383), K = 3000 at 40 words leaves the
# 16-byte strip for the 12-byte one, K = 15000 at 40 words the 8-byte strip for the split solve on full-size workgroups.
GPU_CASES = [
    ('w16_big', 255, 139, 133, 16, 768, 0),
    ('w16_big', 256, 140, 134, 16, 768, 0),
    ('w16_big', 257, 141, 143, 16, 768, 0),
    ('w16_big', 383, 269, 269, 16, 768, 0),
    ('w16_big', 384, 270, 270, 16, 768, 0),
    ('w16_big', 385, 271, 271, 16, 768, 0),
    ('w16_big', 767, 653, 653, 16, 768, 0),
    ('w16_big', 768, 654, 654, 16, 768, 0),
    ('w16_big', 769, 655, 655, 16, 768, 0),
    ('w16_k1000', 127, 77, 77, 16, 256, 0),
    ('w16_k1000', 128, 78, 78, 16, 256, 0),
    ('w16_k1000', 129, 79, 79, 16, 256, 0),
    ('w16_k1000', 255, 205, 205, 16, 256, 0),
    ('w16_k1000', 256, 206, 206, 16, 256, 0),
    ('w16_k1000', 257, 207, 207, 16, 256, 0),
    ('w16_k1000', 383, 333, 333, 16, 256, 0),
    ('w16_k1000', 384, 334, 334, 16, 256, 0),
    ('w16_k1000', 385, 335, 335, 16, 256, 0),
    ('w16_k1000', 767, 717, 717, 16, 768, 0),
    ('w16_k1000', 768, 718, 718, 16, 768, 0),
    ('w16_k1000', 769, 719, 719, 16, 768, 0),
    ('w16_k1000', 1071, 1021, 1021, 16, 768, 0),
    ('w16_k3000', 127, 27, 1, 16, 256, 0),
    ('w16_k3000', 128, 28, 2, 16, 256, 0),
    ('w16_k3000', 129, 29, 3, 16, 256, 0),
    ('w16_k3000', 255, 169, 169, 16, 256, 0),
    ('w16_k3000', 256, 170, 170, 16, 256, 0),
    ('w16_k3000', 257, 171, 171, 16, 256, 0),
    ('w16_k3000', 383, 297, 297, 16, 768, 0),
    ('w16_k3000', 384, 298, 298, 16, 768, 0),
    ('w16_k3000', 385, 299, 299, 16, 768, 0),
    ('w16_k3000', 767, 681, 681, 16, 768, 0),
    ('w16_k3000', 768, 682, 682, 16, 768, 0),
    ('w16_k3000', 769, 683, 683, 16, 768, 0),
    ('w16_k3000', 1279, 1193, 1193, 12, 768, 0),
    ('w16_k3000', 1280, 1194, 1194, 12, 768, 0),
    ('w16_k3000', 1281, 1195, 1195, 12, 768, 0),
    ('w16_k100', 31, 5, 0, 16, 64, 0),
    ('w16_k100', 32, 6, 1, 16, 64, 0),
    ('w16_k100', 33, 7, 2, 16, 64, 0),
    ('w16_k100', 63, 48, 48, 16, 64, 0),
    ('w16_k100', 64, 49, 49, 16, 64, 0),
    ('w16_k100', 65, 50, 50, 16, 64, 0),
    ('w16_k100', 95, 80, 80, 16, 64, 0),
    ('w16_k100', 96, 81, 81, 16, 64, 0),
    ('w16_k100', 97, 82, 82, 16, 64, 0),
    ('w16_k100', 127, 112, 112, 16, 64, 0),
    ('w16_k100', 128, 113, 113, 16, 64, 0),
    ('w12_k10000', 255, 83, 49, 12, 768, 0),
    ('w12_k10000', 256, 84, 50, 12, 768, 0),
    ('w12_k10000', 257, 85, 51, 12, 768, 0),
    ('w12_k10000', 383, 224, 209, 12, 768, 0),
    ('w12_k10000', 384, 225, 210, 12, 768, 0),
    ('w12_k10000', 385, 226, 211, 12, 768, 0),
    ('w12_k5200', 767, 653, 653, 12, 768, 0),
    ('w12_k5200', 768, 654, 654, 12, 768, 0),
    ('w12_k5200', 769, 655, 655, 12, 768, 0),
    ('w8_k15000', 383, 173, 118, 8, 768, 0),
    ('w8_k15000', 384, 174, 119, 8, 768, 0),
    ('w8_k15000', 385, 175, 120, 8, 768, 0),
    ('w8_k15000', 767, 574, 558, 8, 768, 0),
    ('w8_k15000', 768, 575, 559, 8, 768, 0),
    ('w8_k15000', 769, 576, 560, 8, 768, 0),
    ('w8_k15000', 1280, 1087, 1087, 4, 768, 16),
    ('w8_k15000', 1281, 1088, 1088, 4, 768, 16),
    ('w8_k10000', 255, 83, 49, 8, 768, 0),
    ('w8_k10000', 256, 84, 50, 8, 768, 0),
    ('w8_k10000', 257, 85, 51, 8, 768, 0),
    ('w8_k1000', 127, 77, 77, 8, 64, 0),
    ('w8_k1000', 128, 78, 78, 8, 64, 0),
    ('w8_k1000', 129, 79, 79, 8, 64, 0),
    ('w8_k1000', 255, 205, 205, 8, 64, 0),
    ('w8_k1000', 256, 206, 206, 8, 64, 0),
    ('w8_k1000', 257, 207, 207, 8, 64, 0),
    ('w8_k1000', 383, 333, 333, 8, 256, 0),
    ('w8_k1000', 384, 334, 334, 8, 256, 0),
    ('w8_k1000', 385, 335, 335, 8, 256, 0),
    ('w8_k1000', 767, 717, 717, 8, 256, 0),
    ('w8_k1000', 768, 718, 718, 8, 256, 0),
    ('w8_k1000', 769, 719, 719, 8, 256, 0),
    ('w8_k1000', 1071, 1021, 1021, 8, 256, 0),
    ('w4_k3000', 639, 553, 553, 4, 256, 32),
    ('w4_k3000', 640, 554, 554, 4, 256, 32),
    ('w4_k3000', 641, 555, 555, 4, 256, 16),
    ('w4_k3000', 1279, 1193, 1193, 4, 256, 16),
    ('w4_k3000', 1280, 1194, 1194, 4, 256, 16),
    ('w4_k3000', 1281, 1195, 1195, 4, 256, 16),
    ('w2_k3000', 639, 553, 553, 2, 64, 32),
    ('w2_k3000', 640, 554, 554, 2, 64, 32),
    ('w2_k3000', 641, 555, 555, 2, 64, 16),
    ('w2_k3000', 1279, 1193, 1193, 2, 64, 16),
    ('w2_k3000', 1280, 1194, 1194, 2, 64, 16),
    ('w2_k3000', 1281, 1195, 1195, 2, 64, 16),
]


def search_cases(orc):
    """the rows of GPU_CASES, searched: python tests/forced_inact_support.py prints them"""
    rows = []
    for form, f in FORMS.items():
        K = f["K"]
        isis = gpu_reception(orc, K)[2]
        for u in f["us"]:
            n_enc, n_dec = find_n(K, encode_isis(K), u), find_n(K, isis, u)
            if n_enc is None or n_dec is None:
                print("#", form, u, "not reached:", n_enc, n_dec)
                continue
            recs = {case_record(orc, form, n_enc, n_dec, *c)[:3] for c in calls_of(len(rows))}
            assert len(recs) == 1, (form, u, recs)   # (every call of a case runs one form)
            rows.append((form, u, n_enc, n_dec) + recs.pop())
    return rows


if __name__ == "__main__":
    import oracle   # (with the repository root on PYTHONPATH)
    for row in search_cases(oracle):
        print("    %r," % (row,))
