"""The known-answer cases of oracle/ref_kat.c: the case table, the runner, the record parser and the one hashing helper that the
generator (tools/gen_ref_kat.py) and the tests (test_ref_kat.py, test_gpu_ref_kat.py) share.  Plain data and subprocess.

A case is a dict: id, family, kind (params / encode / decode), obj = (len, T, K, Z, Al, ex), and `lines`, the driver lines it
stands for (one, except the verdict groups: one line per reception).  tests/golden/ref_kat.json holds summarise() of what the
REFERENCE's build of the driver answered to every case, and summarise(host=True) of what it answered under --host."""
import hashlib
import json
import os
import signal
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_kat.json")
REF_TREE = "/root/reference"
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "ref_kat")
HIP_BIN = os.path.join(ROOT, "oracle", "_ref", "ref_kat_hip")
FILL = 0x3C                      # the driver's fill of the output buffer and of a symbol buffer nanorq_encode leaves alone
VERDICT_SEED = 4                 # searched (tools/gen_ref_kat.py --search-seed) until the reference refuses >= 3 receptions
FAMILIES = ("params", "encode", "decode_orders", "decode_verdicts", "decode_scattered")
# cases that were chosen first and got no answer from the reference: [{"id", "family", "reason", "replaced_by"}]
DROPPED = []
# where this library deliberately does not do what the reference does: {case id: {"reason": one line, "ours": the summary this library
# must give instead of the reference's}}.  INTEGRATION.md documents each; the tests assert `ours`.
DEVIATIONS = {}
DROP_CAP = 0.05                  # at most this share of a family may be replaced for want of an answer (params exempt)


# ------------------------------------------------------------------------------------------------ helpers

def sha(data):
    """THE hashing helper: SHA-256 of bytes (or of a str's UTF-8), as hex."""
    if isinstance(data, str):
        data = data.encode()
    return hashlib.sha256(bytes(data)).hexdigest()


def canonical(obj):
    return json.dumps(obj, sort_keys=True, separators=(",", ":"))


def kat_bytes(n):
    """byte i = ((uint32) i * 2654435761) >> 24: the payload of every case (as in survey_kat.json)."""
    i = np.arange(n, dtype=np.uint64)
    return (((i * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(24)).astype(np.uint8)


_KP = None


def kprime(K):
    """Table 2's row for K (the smallest K' >= K), from the committed table."""
    global _KP
    if _KP is None:
        with open(os.path.join(ROOT, "tests", "golden", "rfc6330_tables.json")) as f:
            _KP = [r[0] for r in json.load(f)["table2_rows"]]
    return next(k for k in _KP if k >= K)


class Rng:
    """splitmix64: the receptions must not depend on a library's generator."""

    def __init__(self, seed):
        self.s = seed & 0xFFFFFFFFFFFFFFFF

    def next(self):
        self.s = (self.s + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
        return z ^ (z >> 31)

    def below(self, n):
        return self.next() % n

    def shuffle(self, xs):
        for i in range(len(xs) - 1, 0, -1):
            j = self.below(i + 1)
            xs[i], xs[j] = xs[j], xs[i]

    def sample(self, lo, hi, n):
        """n distinct integers of [lo, hi], in the order drawn"""
        got, seen = [], set()
        while len(got) < n:
            x = lo + self.below(hi - lo + 1)
            if x not in seen:
                seen.add(x)
                got.append(x)
        return got


def effective_T(T, Al):
    """what nanorq_encoder_new_ex makes of (T, Al) before it looks at the length"""
    al = max([a for a in (1, 2, 4, 8) if Al >= a] or [1])
    return al if T < al else T - T % al


# ------------------------------------------------------------------------------------------------ the case table

def _obj_words(obj):
    return " ".join(str(int(x)) for x in obj)


def _tok(sbn, lo, hi=None):
    return "%d:%d" % (sbn, lo) if hi is None or hi == lo else "%d:%d-%d" % (sbn, lo, hi)


def _runs(sbn, esis):
    """ascending ESIs as range tokens"""
    out, i = [], 0
    while i < len(esis):
        j = i
        while j + 1 < len(esis) and esis[j + 1] == esis[j] + 1:
            j += 1
        out.append((sbn, esis[i], esis[j]))
        i = j + 1
    return out


def _params_cases():
    cases = []

    def add(name, obj):
        c = dict(id="p_" + name, family="params", kind="params", obj=tuple(obj))
        c["lines"] = ["params %s %s" % (c["id"], _obj_words(obj))]
        cases.append(c)

    for T in (3, 8, 13, 52):
        for Al in (1, 2, 4, 8):
            Te = effective_T(T, Al)        # T < Al (3 under 4 and 8), T no multiple of Al (13, 52 under 8, 3 under 2) are in here
            for n in (10, 103):
                for d in (0, 1, -1):
                    F = n * Te + d
                    add("T%d_A%d_n%d%+d_auto" % (T, Al, n, d), (F, T, 0, 0, Al, 0))
                    add("T%d_A%d_n%d%+d_K25" % (T, Al, n, d), (F, T, 25, 0, Al, 1))
                    add("T%d_A%d_n%d%+d_Z5" % (T, Al, n, d), (F, T, 0, 5, Al, 1))   # both partition classes non-empty at n=103
    KM, ZM = 56403, 256
    add("al0", (1000, 16, 0, 0, 0, 0))
    add("al3", (1000, 16, 0, 0, 3, 0))
    add("al16", (1000, 16, 0, 0, 16, 0))
    add("one_byte", (1, 8, 0, 0, 8, 0))
    add("len0", (0, 8, 0, 0, 8, 0))                                   # the reference divides by zero
    add("len0_K10", (0, 8, 10, 0, 8, 1))
    add("Kmax_one_block", (KM * 8, 8, KM, 0, 8, 1))
    add("Kmax_plus1_one_block", ((KM + 1) * 8, 8, 0, 1, 8, 1))        # more than K_max symbols in the block
    add("Kmax_plus1_K", ((KM + 1) * 8, 8, KM, 0, 8, 1))
    add("K_and_Z", (1000 * 8, 8, 100, 5, 8, 1))
    add("Z256", (5000 * 8, 8, 0, 256, 8, 1))
    add("Z257", (5000 * 8, 8, 0, 257, 8, 1))
    add("Z300_small", (100 * 8, 8, 0, 300, 8, 1))
    add("K1", (300 * 8, 8, 1, 0, 8, 1))                               # more than 256 blocks
    add("K1_256", (256 * 8, 8, 1, 0, 8, 1))
    add("full_8", (ZM * KM * 8, 8, 0, 0, 8, 0))
    add("full_8_plus1", (ZM * KM * 8 + 1, 8, 0, 0, 8, 0))             # T grows by Al
    add("full_4_plus1", (ZM * KM * 4 + 1, 4, 0, 0, 4, 0))
    add("full_1_plus1", (ZM * KM * 1 + 1, 1, 0, 0, 1, 0))             # T *= 1 for ever in the reference
    add("full_16_al1_plus1", (ZM * KM * 16 + 1, 16, 0, 0, 1, 0))
    add("grow_past_u16", (ZM * KM * 32768, 16384, 0, 0, 8, 0))
    add("max_transfer", (946270874880, 65535, 0, 0, 1, 0))
    add("max_transfer_plus1", (946270874881, 65535, 0, 0, 1, 0))
    add("T65535_al8", (65528 * 20, 65535, 0, 0, 8, 0))
    add("T0", (1000, 0, 0, 0, 8, 0))
    add("T0_al1", (1000, 0, 0, 0, 1, 0))
    return cases


def _encode_case(name, obj, groups, precalc=0):
    """groups: [(name, [(sbn, lo, hi), ...]), ...]"""
    c = dict(id="e_" + name, family="encode", kind="encode", obj=tuple(obj), precalc=precalc,
             groups=[(g, list(t)) for g, t in groups])
    toks = [_tok(*t) for _, ts in groups for t in ts]
    c["lines"] = ["encode %s %s %d %s" % (c["id"], _obj_words(obj), precalc, " ".join(toks))]
    return c


def _block_groups(sbn, K, Kp, near=40):
    far = [K + 1000, 2 * Kp, 65535, 65536, (1 << 24) - 7, (1 << 24) - 1]
    return [("src%d" % sbn, [(sbn, 0, K - 1)]), ("near%d" % sbn, [(sbn, K, K + near)]),
            ("far%d" % sbn, [(sbn, e, e) for e in far])]


ENCODE_KS = (1, 2, 10, 11, 26, 100, 101, 257, 1024, 1500, 3000, 8192, 10000, 15000, 27000, 56403)


def _encode_cases():
    cases = []
    for K in ENCODE_KS:
        cases.append(_encode_case("K%d_T16" % K, (K * 16, 16, K, 0, 8, 1), _block_groups(0, K, kprime(K))))
    for K in (10, 257, 1500):
        for T in (8, 24, 40):
            cases.append(_encode_case("K%d_T%d" % (K, T), (K * T, T, K, 0, 8, 1), _block_groups(0, K, kprime(K))))
    for K in (10, 100):
        cases.append(_encode_case("K%d_T13_al1" % K, (K * 13, 13, K, 0, 1, 1), _block_groups(0, K, kprime(K))))
    for K in (100, 1024):
        cases.append(_encode_case("K%d_T16_precalc" % K, (K * 16, 16, K, 0, 8, 1), _block_groups(0, K, kprime(K)), precalc=1))

    def obj_case(name, obj, ks, near=5):
        groups = []
        for sbn, K in enumerate(ks):
            groups += _block_groups(sbn, K, kprime(ks[0]), near=near)   # (2 K' of block 0's row: the reference's max_esi)
        cases.append(_encode_case(name, obj, groups))

    obj_case("ragged", (103 * 64 - 17, 64, 25, 0, 8, 1), [21, 21, 21, 20, 20])
    obj_case("two_block_102_101", (203 * 48, 48, 102, 0, 8, 1), [102, 101])
    obj_case("z5_two_rows", (132 * 16, 16, 0, 5, 8, 1), [27, 27, 26, 26, 26])      # K' = 30 and 26; all coded on 30
    obj_case("al4_T52", (52 * 40 + 9, 52, 0, 0, 4, 0), [3] * 13 + [2])
    return cases


def _decode_case(family, name, obj, script, max_esi=-1, reception=None):
    """script: [("a", sbn, lo, hi) | ("r", sbn) | ("n", sbn)]"""
    c = dict(id=name, family=family, kind="decode", obj=tuple(obj), max_esi=max_esi, script=list(script))
    if reception:
        c["reception"] = reception
    c["lines"] = [_decode_line(name, obj, max_esi, script)]
    return c


def _decode_line(name, obj, max_esi, script):
    toks = []
    for op in script:
        toks.append("a" + _tok(*op[1:]) if op[0] == "a" else "%s%d" % (op[0], op[1]))
    return "decode %s %s %d %s" % (name, _obj_words(obj), max_esi, " ".join(toks))


def _adds(sbn, esis):
    return [("a", sbn, e, e) for e in esis]


def _orders_cases():
    cases = []
    K, T = 100, 16
    obj = (K * T, T, K, 0, 8, 1)
    lost = [0, 7, 8, 31, 32, 33, 50, 64, 98, 99]
    keep = [e for e in range(K) if e not in lost]
    reps = list(range(K, K + len(lost)))
    src_runs = [("a",) + r for r in _runs(0, keep)]

    def add(name, script, obj=obj, max_esi=-1):
        cases.append(_decode_case("decode_orders", "d_" + name, obj, script, max_esi))

    add("sorted", src_runs + _adds(0, reps))
    mixed = keep + reps
    Rng(11).shuffle(mixed)
    add("shuffled", _adds(0, mixed))
    add("repair_first", _adds(0, reps) + src_runs)
    add("repair_descending", src_runs + _adds(0, reps[::-1]))
    add("duplicates", src_runs + _adds(0, [5, 6]) + _adds(0, reps[:4]) + _adds(0, [reps[1], reps[1], 99]) + _adds(0, reps[4:]) + _adds(0, [98, reps[0]]))
    Kp = kprime(K)
    add("above_max_esi", src_runs + _adds(0, [2 * Kp + 1, 2 * Kp, 65535, (1 << 24) - 1]) + [("n", 0)] + _adds(0, reps[1:]))
    add("set_max_esi_refused", src_runs + _adds(0, [2 * Kp + 1]) + _adds(0, reps), max_esi=Kp - 1)
    add("set_max_esi_at_kprime", src_runs + _adds(0, [Kp, Kp + 1]) + _adds(0, reps), max_esi=Kp)
    add("set_max_esi_2p24", src_runs + _adds(0, reps), max_esi=1 << 24)
    add("set_max_esi_top", src_runs + _adds(0, [(1 << 24) - 1, 70000]) + _adds(0, reps[2:]), max_esi=(1 << 24) - 1)
    add("no_gaps_ign", [("a", 0, 0, K - 1)] + _adds(0, [K, 3, K + 1]) + [("n", 0)])
    add("ign_after_repair", src_runs + _adds(0, reps) + [("r", 0)] + _adds(0, [0, K + 50]) + [("n", 0)])
    add("sbn_beyond_z", src_runs + _adds(1, [0]) + _adds(200, [5, 150]) + [("n", 1), ("n", 200)] + _adds(0, reps))
    add("too_few_then_retry", src_runs + _adds(0, reps[:8]) + [("r", 0), ("n", 0)] + _adds(0, reps[8:]) + [("r", 0), ("n", 0)])
    add("nothing_received", [("n", 0)])
    add("only_repairs", _adds(0, list(range(K, 2 * K + 2))))
    add("overhead_20", src_runs + _adds(0, list(range(K + 30, K + 60))))
    # the 102/101 object: block 1 is coded on block 0's row
    o2 = (203 * 48, 48, 102, 0, 8, 1)
    lost1 = [0, 9, 33, 34, 77, 99, 100]
    add("two_block_second", [("a", 0, 0, 101)] + [("a",) + r for r in _runs(1, [e for e in range(101) if e not in lost1])]
        + _adds(1, list(range(101, 101 + len(lost1)))), obj=o2)
    add("two_block_both", [("a",) + r for r in _runs(0, list(range(3, 102)))] + _adds(0, [102, 200, 228])
        + [("a",) + r for r in _runs(1, list(range(0, 95)))] + _adds(1, list(range(101, 107))), obj=o2)
    # the ragged object, every block short of some symbols, the last symbol of the object among them
    o3 = (103 * 64 - 17, 64, 25, 0, 8, 1)
    s3 = []
    for sbn, Kb in enumerate([21, 21, 21, 20, 20]):
        s3 += [("a", sbn, 1, Kb - 2)] + _adds(sbn, [Kb + 3, Kb, Kb + 9])
    add("ragged_object", s3, obj=o3)
    for K2, seed in ((1500, 5), (3000, 6)):
        r = Rng(seed)
        lost2 = sorted(r.sample(0, K2 - 1, K2 // 10))
        mixed2 = [e for e in range(K2) if e not in set(lost2)] + list(range(K2, K2 + len(lost2) + 1))
        r.shuffle(mixed2)
        add("K%d_shuffled" % K2, _adds(0, mixed2), obj=(K2 * T, T, K2, 0, 8, 1))
    return cases


VERDICT_KS = (10, 26, 100, 257)
VERDICT_COUNTS = {0: 100, 1: 25, 2: 25}          # receptions per K at each overhead: 400 + 100 + 100 in all


def reception(K, rng, overhead, loss=None, esi_hi=None):
    """lost source ESIs (ascending) and the repair ESIs in arrival order"""
    p = loss if loss is not None else 0.10 + 0.50 * (rng.below(1001) / 1000.0)
    nlost = max(1, int(round(K * p)))
    lost = sorted(rng.sample(0, K - 1, nlost))
    reps = rng.sample(K, esi_hi if esi_hi is not None else 2 * K, nlost + overhead)
    return lost, reps


def _verdict_cases(seed=None):
    seed = VERDICT_SEED if seed is None else seed
    cases = []
    T = 16
    for K in VERDICT_KS:
        for oh, n in sorted(VERDICT_COUNTS.items()):
            rng = Rng(seed * 1000003 + K * 101 + oh)
            cid = "v_K%d_oh%d" % (K, oh)
            obj = (K * T, T, K, 0, 8, 1)
            c = dict(id=cid, family="decode_verdicts", kind="decode", obj=obj, max_esi=-1, receptions=[], lines=[])
            for i in range(n):
                lost, reps = reception(K, rng, oh)
                keep = [e for e in range(K) if e not in set(lost)]
                script = [("a",) + r for r in _runs(0, keep)] + _adds(0, reps)
                c["receptions"].append(dict(K=K, T=T, lost=lost, reps=reps))
                c["lines"].append(_decode_line("%s.%d" % (cid, i), obj, -1, script))
            cases.append(c)
    return cases


SCATTERED = [(K, loss, oh) for K in (1000, 3000, 8192) for loss in (0.10, 0.30) for oh in (0, 2)] + [(10000, 0.10, 2)]


def _scattered_cases():
    cases = []
    T = 16
    for K, loss, oh in SCATTERED:
        rng = Rng(K * 7 + int(loss * 100) * 3 + oh)
        lost, reps = reception(K, rng, oh, loss=loss, esi_hi=65535)
        keep = [e for e in range(K) if e not in set(lost)]
        # the repair symbols arrive between the source symbols, in the order drawn
        cuts = sorted(rng.below(len(keep) + 1) for _ in reps)
        script, at = [], 0
        for cut, e in zip(cuts, reps):
            script += [("a",) + r for r in _runs(0, keep[at:cut])] + [("a", 0, e, e)]
            at = cut
        script += [("a",) + r for r in _runs(0, keep[at:])]
        cases.append(_decode_case("decode_scattered", "s_K%d_l%d_oh%d" % (K, int(loss * 100), oh), (K * T, T, K, 0, 8, 1), script,
                                  max_esi=65535, reception=dict(K=K, T=T, lost=lost, reps=reps)))
    return cases


_TABLE = {}


def cases(seed=None):
    """the whole table, in family order"""
    key = VERDICT_SEED if seed is None else seed
    if key not in _TABLE:
        _TABLE[key] = _params_cases() + _encode_cases() + _orders_cases() + _verdict_cases(key) + _scattered_cases()
    return _TABLE[key]


def family(name, seed=None):
    return [c for c in cases(seed) if c["family"] == name]


# ------------------------------------------------------------------------------------------------ running the driver

def signal_name(rc):
    if rc >= 0:
        return "exit %d" % rc
    try:
        return signal.Signals(-rc).name
    except ValueError:
        return "signal %d" % -rc


def run_driver(binary, lines, host=False, timeout=120, env=None):
    """Feed `lines` to the driver in one child process.  Returns (records, trouble): records = {id: [words of a line, ...]} of the
    cases that ended; trouble = None, or (id of the case the process was in or None, "SIGFPE" / "timeout" / "exit 2")."""
    cmd = [binary] + (["--host"] if host else [])
    try:
        p = subprocess.run(cmd, input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True,
                           timeout=timeout, env=env)
        out, why = p.stdout, (None if p.returncode == 0 else signal_name(p.returncode))
    except subprocess.TimeoutExpired as e:
        out = e.stdout or ""
        if isinstance(out, bytes):
            out = out.decode()
        why = "timeout"
    records, cur, rows = {}, None, None
    for ln in out.split("\n"):
        w = ln.split(" ")
        if w[0] == "begin":
            cur, rows = w[1], []
        elif w[0] == "end" and cur is not None:
            records[cur] = rows
            cur = None
        elif cur is not None:
            rows.append(w)
    return records, ((cur, why) if why else None)


def run_cases(binary, table, host=False, timeout=120, case_timeout=20, env=None, go_on=True):
    """Run a list of cases; a case the driver dies or hangs in is run again alone under case_timeout, and if that gives no answer
    either it is recorded as {"no_answer": why} and the rest goes on.  Returns {case id: [records of its lines] or {"no_answer":..}}.
    go_on=False (a driver that uses the GPU): nothing is started again after trouble; RuntimeError names the case and the cause."""
    lines, owner = [], {}
    for c in table:
        if host and c["kind"] == "encode":
            continue
        for ln in c["lines"]:
            owner[ln.split(" ")[1]] = c["id"]
            lines.append(ln)
    got, dead = {}, {}
    todo = lines
    while todo:
        recs, trouble = run_driver(binary, todo, host=host, timeout=timeout, env=env)
        got.update(recs)
        if not trouble:
            break
        at = trouble[0]
        if not go_on:
            raise RuntimeError("driver %s: %s in case %s" % (os.path.basename(binary), trouble[1], at))
        if at is None:                                      # died between cases, or never started: nothing to blame
            raise RuntimeError("driver %s: %s outside a case" % (binary, trouble[1]))
        idx = next(i for i, ln in enumerate(todo) if ln.split(" ")[1] == at)
        if len(todo) > 1 and trouble[1] == "timeout":       # the list as a whole may just have been long: ask that case alone
            r1, t1 = run_driver(binary, [todo[idx]], host=host, timeout=case_timeout, env=env)
            got.update(r1)
            if t1:
                dead[at] = t1[1]
        else:
            dead[at] = trouble[1]
        todo = todo[idx + 1:]
    out = {}
    for c in table:
        if host and c["kind"] == "encode":
            continue
        ids = [ln.split(" ")[1] for ln in c["lines"]]
        bad = [dead[i] for i in ids if i in dead]
        out[c["id"]] = {"no_answer": bad[0]} if bad else [got[i] for i in ids]
    return out


# ------------------------------------------------------------------------------------------------ records -> what the fixture holds

def _rle(xs):
    out = []
    for x in xs:
        if out and out[-1][0] == x:
            out[-1][1] += 1
        else:
            out.append([x, 1])
    return out


def _facts(rows):
    """the 'new' and 'ks' lines"""
    new = next(r for r in rows if r[0] in ("new", "decoder"))
    if new[1] == "null":
        return "null"
    kv = dict(x.split("=") for x in new[2:])
    ks = next(r for r in rows if r[0] == "ks")[1:]
    return [kv["common"], kv["scheme"], int(kv["F"]), int(kv["T"]), int(kv["Z"]), int(kv["maxblocks"]), _rle([int(k) for k in ks])]


def _codes(rows):
    codes = [int(r[3]) for r in rows if r[0] == "add"]
    s = "".join("E" if c < 0 else str(c) for c in codes)
    other = [[i, c] for i, c in enumerate(codes) if c != 0]
    return dict(n=len(codes), sha=sha(s), other=other[:40], n_other=len(other))


def _one(case, rows, host):
    if isinstance(rows, dict):
        return rows
    odd = [" ".join(r) for r in rows if r[0] in ("bad", "short", "skipped") or (r[0] == "gen" and r[-1] != "1")]
    s = {"new": _facts(rows)}
    if odd:
        s["odd"] = odd
    if case["kind"] == "params" or s["new"] == "null":
        return s
    if case["kind"] == "encode":
        pc = [int(r[1]) for r in rows if r[0] == "precalc"]
        if pc:
            s["precalc"] = pc[0]
        syms = [r for r in rows if r[0] == "sym"]
        s["groups"], at = {}, 0
        for name, toks in case["groups"]:
            n = sum(hi - lo + 1 for _, lo, hi in toks)
            part = syms[at:at + n]
            at += n
            written = sorted(set(int(r[3]) for r in part))
            g = dict(n=len(part), written=written, sha=sha(bytes.fromhex("".join(r[4] for r in part))))
            if not name.startswith("src"):
                g["head"] = [part[0][4][:32], part[-1][4][:32]]
            s["groups"][name] = g
        assert at == len(syms), (case["id"], at, len(syms))
        return s
    sm = [int(r[1]) for r in rows if r[0] == "setmax"]
    if sm:
        s["setmax"] = sm[0]
    s["codes"] = _codes(rows)
    s["mid"] = [[r[0]] + [int(x) for x in r[1:]] for r in rows if r[0] in ("num",) + (() if host else ("rep",))]
    fin = [[int(x) for x in r[1:]] for r in rows if r[0] == "final"]
    s["final"] = [f[1:3] for f in fin] if host else [f[1:] for f in fin]
    out = next(r for r in rows if r[0] == "out")[1] if any(r[0] == "out" for r in rows) else ""
    s["out"] = sha(bytes.fromhex(out))
    if not host:
        s["out_head"] = out[:32]
    return s


def summarise(case, recs, host=False):
    """what the fixture keeps of a case's records.  recs: the list run_cases() gives (one entry per line), or {"no_answer": ..}."""
    if isinstance(recs, dict):
        return recs
    if len(case["lines"]) == 1:
        return _one(case, recs[0], host)
    ones = [_one(case, r, host) for r in recs]                 # a verdict group: one bit per reception and one digest of the rest
    s = dict(n=len(ones), sha=sha(canonical(ones)))
    if not host:
        s["verdicts"] = "".join(str(o["final"][0][2]) for o in ones)
    return s


def block_layout(ks, T):
    """byte offset of every block in the object (N = 1: a block's symbols lie one after the other)"""
    offs, at = [], 0
    for K in ks:
        offs.append(at)
        at += K * T
    return offs


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)
