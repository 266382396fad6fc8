"""Test support for the row pipelines of solve_body.h (fwd_rows and its half / third forms, rev_rows, fwd_rows_wide): op streams
in the layout of plan.h, the two rules a stream obeys, a plain replay as the reference, models of the pipelined orders, the
case table of tests/test_gpu_rows.py and the binding of tests/gpu/librows_probe.so.

A stream here is two arrays dst[nrows, 64] and src[nrows, 64] of image indices (slot + NRQ_SCRATCH); a padding op of lane l has
dst = src = l.  pack() lays it out as the pipelines fetch it.

The rules (plan.h: "a row may only read slots last written NRQ_PIPE or more rows earlier"), for the real ops of a stream:
  R1  within a row, no index is both a source and a target;
  R2  an index that is a target in row q is not a source in rows q+1 .. q+NRQ_PIPE-1.
Repeated targets in a row and repeated sources are legal.  On such streams the pipelined orders of the device (forward: apply
row q-NRQ_PIPE, then read row q; wide: read row q, then apply row q-1; reverse: the same depth from the last row down, fields
swapped) compute what the plain replay computes: tests/test_rows_support.py holds the models to it on every case of the table.
"""
import ctypes as C
import functools
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "nanorq_amd", "csrc")
LDS_MAX = 163840  # dynamic LDS of every probe launch: the MI355X workgroup's 160 KiB


def read_defines(path, names):
    """the values of `#define NAME <integer expression of earlier names>` lines of a C source (first definition of each)"""
    text = open(path).read()
    env = {}
    for name, body in re.findall(r"^\s*#define (\w+) ([^\n/]+?)\s*(?:/\*.*)?$", text, re.M):
        if name in env:
            continue
        expr = re.sub(r"\b(\d+)u\b", r"\1", body)
        if not re.fullmatch(r"[\w\s()+*\-]+", expr):
            continue
        try:
            env[name] = int(eval(expr, {"__builtins__": {}}, dict(env)))
        except Exception:
            continue
    return {n: env[n] for n in names}


_P = read_defines(os.path.join(CSRC, "plan.h"), ("NRQ_ROW", "NRQ_PIPE", "NRQ_RING_MULT", "NRQ_RING", "NRQ_RING_MAX", "NRQ_PAD_ROWS", "NRQ_SCRATCH"))
ROW, PIPE, RING, RING_MAX, PAD_ROWS, SCRATCH = (_P[k] for k in ("NRQ_ROW", "NRQ_PIPE", "NRQ_RING", "NRQ_RING_MAX", "NRQ_PAD_ROWS", "NRQ_SCRATCH"))
assert ROW == 64 and SCRATCH == ROW, "a padding op of lane l names scratch slot l"


def op_index(row, lane):
    """NRQ_OP_INDEX: the stream is stored quad-interleaved"""
    return ((row >> 2) * ROW + lane) * 4 + (row & 3)


def stream_words(nrows):
    """words of memory a stream of nrows rows has: NRQ_STREAM_ROWS(nrows + NRQ_PAD_ROWS) rows"""
    return ((nrows + PAD_ROWS + 3) & ~3) * ROW


def pack(dst, src):
    """op words dst | src << 16 at NRQ_OP_INDEX(row, lane); every row behind the stream is NRQ_NOP_AT(lane)"""
    nrows = dst.shape[0]
    lanes = np.arange(ROW, dtype=np.uint32)
    rows = np.arange(stream_words(nrows) // ROW, dtype=np.int64)
    words = np.empty(stream_words(nrows), np.uint32)
    idx = op_index(rows[:, None], lanes[None, :].astype(np.int64))
    words[idx] = (lanes * 0x10001)[None, :]
    if nrows:
        words[idx[:nrows]] = dst.astype(np.uint32) | (src.astype(np.uint32) << 16)
    return words


def unpack(words, nrows):
    idx = op_index(np.arange(nrows, dtype=np.int64)[:, None], np.arange(ROW, dtype=np.int64)[None, :])
    w = words[idx] if nrows else np.zeros((0, ROW), np.uint32)
    return (w & 0xFFFF).astype(np.int64), (w >> 16).astype(np.int64)


def check_stream(words, nrows, nslots, rules=(1, 2)):
    """What a stream must be before the device sees it (AssertionError otherwise): its memory as large as the pipelines read ahead,
    padding behind row nrows, every op either the lane's padding op or a real one with both indices in [NRQ_SCRATCH, nslots),
    and the rules R1 and R2 on the real ops."""
    assert words.dtype == np.uint32 and words.shape == (stream_words(nrows),)
    assert SCRATCH < nslots <= 65536
    all_rows = words.size // ROW
    dst, src = unpack(words, all_rows)
    lanes = np.arange(ROW)
    nop = (dst == lanes) & (src == lanes)
    assert nop[nrows:].all(), "rows behind the stream must be padding"
    real = ~nop[:nrows]
    d, s = dst[:nrows], src[:nrows]
    assert ((d[real] >= SCRATCH) & (d[real] < nslots) & (s[real] >= SCRATCH) & (s[real] < nslots)).all(), "index outside the image"
    for q in range(nrows):
        t = set(d[q][real[q]].tolist())
        if 1 in rules:
            assert not t & set(s[q][real[q]].tolist()), "R1: row %d reads what it writes" % q
        if 2 in rules:
            for k in range(q + 1, min(q + PIPE, nrows)):
                assert not t & set(s[k][real[k]].tolist()), "R2: row %d reads a target of row %d" % (k, q)
    return dst[:nrows], src[:nrows]


def obeys(words, nrows, nslots, rules):
    try:
        check_stream(words, nrows, nslots, rules)
        return True
    except AssertionError:
        return False


# ---- the generator ----------------------------------------------------------------------------------------------------------------

KINDS = ("a", "b", "c", "d")        # random fill, full rows, chains at the minimum distance, one target
KINDS_W2 = ("d2", "d3")             # 2-byte slots: pairs on the halfwords of a dword, odd and even slots mixed
SMALL = (66, 70, 200, 1000)         # image indices of kinds a-d: collisions and reuse are dense


def gen_stream(seed, nrows, pool, kind, hazard=True, group=ROW, pad_every=0):
    """dst, src of a stream on the indices `pool`.  hazard=False switches R2 off (R1 stays).  group: lanes of an instruction of the
    wide form (kind f).  pad_every: every pad_every-th row is all padding (the rows a planner puts between level groups)."""
    rng = np.random.default_rng(seed)
    pool = np.unique(np.asarray(list(pool), np.int64))
    assert pool.size and pool[0] >= SCRATCH and pool[-1] < 65536
    lanes = np.arange(ROW, dtype=np.int64)
    dst, src = np.tile(lanes, (nrows, 1)), np.tile(lanes, (nrows, 1))
    none = np.zeros(0, np.int64)
    targets = []  # per row: its targets
    mark = np.zeros(65536, bool)

    def without(a, *gone):
        """the indices of a that are in none of the arrays `gone`"""
        mark[:] = False
        for g in gone:
            mark[g] = True
        return a[~mark[a]]

    pairs = np.intersect1d(pool[pool % 2 == 0], pool - 1)  # even indices whose odd neighbour is in the pool too
    for q in range(nrows):
        targets.append(none)
        if pad_every and q % pad_every == pad_every - 1:
            continue
        allowed = without(pool, *targets[max(0, q - PIPE + 1):q]) if hazard else pool
        if allowed.size == 0 or pool.size < 2:
            continue
        # which lanes hold real ops
        if kind == "a":
            act = rng.permutation(ROW)[:rng.integers(0, ROW + 1)]
        elif kind == "f":
            act = (np.array([0]), np.array([0, 1]), np.array([ROW - group + rng.integers(0, group)]), lanes)[q % 4]
        else:
            act = lanes
        if act.size == 0:
            continue
        # the row's sources S and targets T: disjoint (R1), S outside the targets of the rows just before (R2)
        if kind in ("d", "d2", "d3"):
            if kind == "d":  # (a target that leaves a source: the pool may be two slots)
                T = rng.choice(pool if allowed.size > 1 else without(pool, allowed), 1)
            else:
                e = rng.choice(pairs, 1 if kind == "d2" else min(2, pairs.size), replace=False)
                T = np.concatenate([e, e + 1])
            S = without(allowed, T)
            if S.size == 0:
                continue
            S = rng.permutation(S)[:rng.integers(1, min(S.size, ROW) + 1)]
            if kind == "d2":
                dst[q, act] = T[act % 2]  # neighbouring lanes on the two halfwords of one dword
            else:
                dst[q, act] = rng.choice(T, act.size)
            src[q, act] = rng.choice(S, act.size)
            targets[q] = np.unique(dst[q, act])
            continue
        S = None
        if kind == "c" and q >= PIPE and targets[q - PIPE].size:
            chain = without(targets[q - PIPE], without(pool, allowed))
            if chain.size:
                S = chain[:pool.size - 1]
        if S is None:
            S = rng.permutation(allowed)[:rng.integers(1, min(allowed.size, ROW, pool.size - 1) + 1)]
        T = without(pool, S)
        T = rng.permutation(T)[:rng.integers(1, min(T.size, ROW) + 1)]
        dst[q, act] = rng.choice(T, act.size)
        src[q, act] = rng.choice(S, act.size)
        targets[q] = np.unique(dst[q, act])
    return dst, src


# ---- the reference: a plain replay, no pipeline in it -------------------------------------------------------------------------------

def replay_forward(img, dst, src):
    """img: uint8[nslots, width], changed in place.  Row by row: every op's target ^= its source as it was before the row."""
    for q in range(dst.shape[0]):
        v = img[src[q]]
        np.bitwise_xor.at(img, dst[q], v)
    return img


def replay_reverse(img, dst, src):
    """rev_rows: the rows from the last to the first, every op transposed (its source ^= its target)"""
    for q in range(dst.shape[0] - 1, -1, -1):
        v = img[dst[q]]
        np.bitwise_xor.at(img, src[q], v)
    return img


# ---- the orders the device runs (CPU tier: equal to the replay on legal streams) -----------------------------------------------------

def model_forward(img, dst, src, depth=None):
    """fwd_rows / emu_forward: step q applies row q - P, then reads row q"""
    P = PIPE if depth is None else depth
    n = dst.shape[0]
    held = {}
    for q in range(n + P):
        if q >= P:
            np.bitwise_xor.at(img, dst[q - P], held.pop(q - P))
        if q < n:
            held[q] = img[src[q]]
    return img


def model_wide(img, dst, src):
    """fwd_rows_wide: step q reads row q, then applies row q - 1"""
    n = dst.shape[0]
    prev = None
    for q in range(n + 1):
        cur = img[src[q]] if q < n else None
        if prev is not None:
            np.bitwise_xor.at(img, dst[q - 1], prev)
        prev = cur
    return img


def model_reverse(img, dst, src):
    """rev_rows: from the last row down, step k applies row k + P (read P steps ago), then reads row k; the last P pending rows are
    applied oldest first"""
    n = dst.shape[0]
    held = {}
    for k in range(n - 1, -1, -1):
        if k + PIPE in held:
            np.bitwise_xor.at(img, src[k + PIPE], held.pop(k + PIPE))
        held[k] = img[dst[k]]
    for k in sorted(held, reverse=True):
        np.bitwise_xor.at(img, src[k], held[k])
    return img


# ---- the case table -----------------------------------------------------------------------------------------------------------------

def fwd_nrows(U):
    """every edge of fwd_rows_impl's loop: the primed ring is U - 4 rows, whole trips of U run while base < nrows + NRQ_PIPE"""
    return sorted(set([0, 1, 2, 3, 4, 5] + list(range(U - 5, U + 6)) + list(range(2 * U - 2, 2 * U + 2)) + [3 * U + 7]))


REV_NROWS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49)  # chunks of 16 rows, the first may start in the padding


def wide_nrows(G):
    n = 32 // G  # rows of the 32-instruction ring
    return sorted(set([0, 1, 2, n - 1, n, n + 1, 2 * n - 1, 2 * n + 1, 3 * n + 1]))


# full images: the largest the LDS holds
FULL = {2: 65536, 4: 40960, 8: 20480, 12: 13653, 16: 10240}


def extreme_pool(nslots, rng):
    """the first real slot, the last index, the indices either side of 0x8000 (bit 15 of a field) where the image reaches them"""
    pool = [SCRATCH, SCRATCH + 1, SCRATCH + 2, nslots - 3, nslots - 2, nslots - 1]
    if nslots >= 0x8000 + 8:
        pool += list(range(0x8000 - 8, 0x8000 + 8))
    pool += [int(i) for i in rng.integers(SCRATCH, nslots, 12)]
    return pool


class Case:
    """one workgroup of a probe launch"""
    def __init__(self, name, nrows, nslots, dst, src, seed):
        self.name, self.nrows, self.nslots, self.dst, self.src, self.seed = name, nrows, nslots, dst, src, seed
        self.words = pack(dst, src)
        self.words.setflags(write=False)
        self._legal = False

    def check(self):
        """check_stream on the packed words, once (the cases are shared between the instances of a ring; the words are read-only)"""
        if not self._legal:
            d, s = check_stream(self.words, self.nrows, self.nslots)
            assert np.array_equal(d, self.dst) and np.array_equal(s, self.src)
            self._legal = True

    def image(self, width):
        """the seeded start image, uint8[nslots, width]: the scratch slots zero (as ph_clear leaves them), every other slot random.
        Narrower widths are the leading bytes of the 16-byte image, so that a reference is shared between them."""
        rng = np.random.default_rng(self.seed ^ 0x5EED)
        img = rng.integers(0, 256, (self.nslots, max(width, 16)), dtype=np.uint8)[:, :width].copy()
        img[:SCRATCH] = 0
        return img


def _seed(*parts):
    h = 0x9E3779B9
    for p in parts:
        for ch in str(p):
            h = (h * 1000003 ^ ord(ch)) & 0x7FFFFFFF
    return h


@functools.lru_cache(maxsize=None)
def small_cases(family, ring, w2=False):
    """kinds a-d (and, w2, the two kinds of 2-byte slots) on the small images, for every nrows of the family: "fwd" with ring U,
    "rev", or "wide" with ring = G (then also kind f: thin rows)"""
    nrows_list = fwd_nrows(ring) if family == "fwd" else REV_NROWS if family == "rev" else wide_nrows(ring)
    group = ROW // ring if family == "wide" else ROW
    kinds = KINDS + (KINDS_W2 if w2 else ()) + (("f",) if family == "wide" else ())
    out = []
    for n in nrows_list:
        for kind in kinds:
            if w2 and kind in KINDS:
                continue  # (the w2 table holds only what it adds)
            for si, nslots in enumerate(SMALL):
                if kind in KINDS_W2 and nslots == 66:
                    continue  # (two real slots: no source left beside a pair of targets)
                seed = _seed(family, ring, n, kind, nslots)
                pad_every = (2, 0, 2, 3)[si] if kind == "c" else 0
                dst, src = gen_stream(seed, n, range(SCRATCH, nslots), kind, group=group, pad_every=pad_every)
                out.append(Case("%s-n%d-%s-%d" % (family, n, kind, nslots), n, nslots, dst, src, seed))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def extreme_cases(family, ring, nslots):
    """kind e: full rows on a full image that name its first real slot, its last index and the indices round 0x8000"""
    nrows_list = fwd_nrows(ring) if family == "fwd" else REV_NROWS if family == "rev" else wide_nrows(ring)
    out = []
    for n in nrows_list:
        seed = _seed(family, ring, n, "e", nslots)
        pool = extreme_pool(nslots, np.random.default_rng(seed))
        dst, src = gen_stream(seed, n, pool, "b")
        out.append(Case("%s-n%d-e-%d" % (family, n, nslots), n, nslots, dst, src, seed))
    return tuple(out)


# the probe's instances (tests/gpu/rows_probe.hip g_inst): name -> (family, ring U or G, slot bytes)
INSTANCES = {}
for _wb in (16, 8, 4, 2):
    for _u in (24, 36, 60):
        INSTANCES["fwd_rows<%d,%d>" % (_wb, _u)] = ("fwd", _u, _wb)
for _wb in (4, 2):
    INSTANCES["fwd_rows<%d,120>" % _wb] = ("fwd", 120, _wb)
INSTANCES["fwd_rows_half<16,120>"] = ("fwd", 120, 16)
INSTANCES["fwd_rows_half<8,120>"] = ("fwd", 120, 8)
INSTANCES["fwd_rows_third<120>"] = ("fwd", 120, 12)
INSTANCES["fwd_rows_two_thirds<120>"] = ("fwd", 120, 12)
for _wb in (16, 8, 4):
    INSTANCES["rev_rows<%d>" % _wb] = ("rev", 0, _wb)
for _g in (2, 4, 8):
    INSTANCES["fwd_rows_wide<%d>" % _g] = ("wide", _g, 16 * _g)


def instance_cases(name):
    """every case of an instance's launch: the small images shared by the widths of a ring, then the instance's full image"""
    family, ring, width = INSTANCES[name]
    cases = small_cases(family, ring)
    if width == 2:
        cases += small_cases(family, ring, True)
    return cases + extreme_cases(family, ring, FULL[16] // ring if family == "wide" else FULL[width])


_REPLAY = {"fwd": replay_forward, "wide": replay_forward, "rev": replay_reverse}
_REF16 = {}


def reference(name, case):
    """the image after the stream, by the plain replay.  Of the small images the 16-byte reference is computed once and its leading
    bytes serve the narrower widths (the replay treats every byte column alike)."""
    family, ring, width = INSTANCES[name]
    if family == "wide" or case.nslots > max(SMALL):
        return _REPLAY[family](case.image(width), case.dst, case.src)
    key = (family, ring, case.name)
    if key not in _REF16:
        ref = _REPLAY[family](case.image(16), case.dst, case.src)
        ref.setflags(write=False)
        _REF16[key] = ref
    return _REF16[key][:, :width]


def lds_pattern(nbytes=LDS_MAX):
    """what the LDS holds behind an image before the run -- and must still hold after it"""
    return ((np.arange(nbytes, dtype=np.uint32) * 7 + 3) % 251).astype(np.uint8)


# ---- the probe ------------------------------------------------------------------------------------------------------------------------

class ProbeCase(C.Structure):
    _fields_ = [("ops", C.c_void_p), ("ops_words", C.c_uint64), ("image_in", C.c_void_p), ("image_out", C.c_void_p),
                ("nrows", C.c_uint32), ("pad", C.c_uint32)]


_LIB = None


def probe(path=None):
    """the probe library, loaded once.  path: another build of it, given before anything else loads the regular one (a scratch build
    with a defect seeded in the copy of solve_body.h it sees: docs/LAB_NOTES.md)"""
    global _LIB
    if _LIB is None:
        if path is None:
            from nanorq_amd import build as nbuild
            path = nbuild.build_rows_probe()
        L = C.CDLL(path)
        L.rows_probe_ninstances.restype = C.c_uint32
        L.rows_probe_name.argtypes = [C.c_uint32]
        L.rows_probe_name.restype = C.c_char_p
        L.rows_probe_slot_bytes.argtypes = [C.c_uint32]
        L.rows_probe_slot_bytes.restype = C.c_uint32
        L.rows_probe_run.argtypes = [C.c_uint32, C.POINTER(ProbeCase), C.c_uint32, C.c_uint32]
        L.rows_probe_addr.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        _LIB = L
    return _LIB


def probe_instances():
    """name -> (index, slot bytes) of the library's instance table"""
    L = probe()
    return {L.rows_probe_name(i).decode(): (i, L.rows_probe_slot_bytes(i)) for i in range(L.rows_probe_ninstances())}


def run_instance(name, cases, lds_bytes=LDS_MAX):
    """One launch: every case's stream on its image (the rest of the LDS filled with lds_pattern).  Every stream is checked against
    R1, R2 and its image's bounds first.  Returns (status, lds_in, lds_out): uint8[ncases, lds_bytes] each."""
    family, ring, width = INSTANCES[name]
    index, slot_bytes = probe_instances()[name]
    assert slot_bytes == width
    n = len(cases)
    lds_in = np.tile(lds_pattern(lds_bytes), (n, 1))
    lds_out = np.zeros((n, lds_bytes), np.uint8)
    recs = (ProbeCase * n)()
    for k, c in enumerate(cases):
        c.check()
        assert c.nslots * width <= lds_bytes
        lds_in[k, :c.nslots * width] = c.image(width).ravel()
        recs[k].ops, recs[k].ops_words, recs[k].nrows = c.words.ctypes.data, c.words.size, c.nrows
        recs[k].image_in, recs[k].image_out = lds_in[k].ctypes.data, lds_out[k].ctypes.data
    status = probe().rows_probe_run(index, recs, n, lds_bytes)
    return status, lds_in, lds_out
