"""CPU tier of the reference known answers (tests/golden/ref_kat.json: what the reference's OWN library answered, through
oracle/ref_kat.c, to the cases of ref_kat_support.py).  The fixture is complete and fresh; the oracle computes what the reference
computed; this library's host layer (oracle/_ref/ref_kat_hip --host: no solver needed) answers what the reference answered; the
stand-in field library the reference was built over is checked against arithmetic done here."""
import importlib.util
import os
import subprocess

import numpy as np
import pytest

import ref_kat_support as S

GOLD = S.load_golden()
CASES = S.cases()
BY_ID = {c["id"]: c for c in CASES}


def expected(cid, host=False):
    """what this library must answer: the reference's answer, or the documented deviation from it"""
    dev = GOLD["deviations"].get(cid)
    if dev:
        return dev["ours_host" if host else "ours"]
    return GOLD["cases"][cid]["host" if host else "ref"]


# ------------------------------------------------------------------------------------------------ 1, 2: the fixture itself

def test_fixture_is_complete():
    assert sorted(GOLD["cases"]) == sorted(BY_ID), "the fixture and the case table list different cases"
    assert GOLD["verdict_seed"] == S.VERDICT_SEED and GOLD["dropped"] == S.DROPPED and GOLD["deviations"] == S.DEVIATIONS
    for fam in S.FAMILIES:
        ids = [c["id"] for c in S.family(fam)]
        silent = [i for i in ids if "no_answer" in GOLD["cases"][i]["ref"]]
        if fam == "params":
            # where the reference refuses to answer is what this family records; the library returns NULL there
            assert 250 <= len(ids) and 0 < len(silent) < 10, (len(ids), silent)
            assert sorted(GOLD["params_no_answer"]) == sorted(silent)
            continue
        assert not silent, "cases without an answer from the reference: %r" % silent
        dropped = [d for d in GOLD["dropped"] if d["family"] == fam]
        assert len(dropped) <= S.DROP_CAP * len(ids), (fam, dropped)
    assert os.path.getsize(S.GOLDEN) < 100 * 1000
    # the design failure rate (0.5-1 %) shows: the reference refuses at least three receptions without overhead, and not above 5 %
    v0 = "".join(GOLD["cases"][c["id"]]["ref"]["verdicts"] for c in S.family("decode_verdicts") if c["id"].endswith("oh0"))
    assert len(v0) >= 400 and 3 <= v0.count("0") <= len(v0) // 20, v0.count("0")
    for oh in (1, 2):
        v = "".join(GOLD["cases"][c["id"]]["ref"]["verdicts"] for c in S.family("decode_verdicts") if c["id"].endswith("oh%d" % oh))
        assert len(v) >= 100


def _generator():
    spec = importlib.util.spec_from_file_location("gen_ref_kat", os.path.join(S.ROOT, "tools", "gen_ref_kat.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixture_is_fresh():
    """Where the reference tree is, its library answers today what the committed file says (everything but the measured wall time)."""
    if not os.path.isdir(os.path.join(S.REF_TREE, "lib")):
        pytest.skip("no reference tree here")
    assert os.path.isfile(S.REF_BIN), "the reference tree is here but oracle/_ref/ref_kat is not built"
    gen = _generator()
    doc = gen.generate()
    doc["provenance"]["wall_seconds"] = GOLD["provenance"]["wall_seconds"]
    assert gen.dump(doc) == gen.dump(GOLD)


# ------------------------------------------------------------------------------------------------ 5: the stand-in, the survey answers

def _gf_mul(a, b):
    """carry-less product modulo x^8+x^4+x^3+x^2+1"""
    r = 0
    while b:
        if b & 1:
            r ^= a
        a <<= 1
        if a & 0x100:
            a ^= 0x11D
        b >>= 1
    return r


def test_stand_in_field_library(orc):
    """The stand-in's tables against the project's own and against arithmetic mod 0x11D; its four row kernels at the lengths
    around the 32-byte row stride, rows i != j, against the same arithmetic; no kernel writes past the row's length."""
    subprocess.run(["make", "-s", "-C", os.path.join(S.ROOT, "oracle"), "_ref/refshim_selftest"], check=True)
    out = subprocess.run([os.path.join(S.ROOT, "oracle", "_ref", "refshim_selftest")], stdout=subprocess.PIPE, check=True,
                         universal_newlines=True, timeout=60).stdout.split("\n")
    rows = [ln.split(" ") for ln in out if ln]
    tab = {r[0]: bytes.fromhex(r[1]) for r in rows if r[0] in ("EXP", "LOG", "INV")}
    e, l, inv = orc.gf_tables()
    assert tab["EXP"] == e.tobytes() and tab["LOG"][1:] == l.tobytes()[1:] and tab["INV"] == inv.tobytes()
    x = 1
    for n in range(510):
        assert tab["EXP"][n] == x
        if n < 255:
            assert tab["LOG"][x] == n
        x = _gf_mul(x, 2)
    assert tab["INV"][0] == 0 and all(_gf_mul(v, tab["INV"][v]) == 1 for v in range(1, 256))
    seen = set()
    for k in (1, 31, 32, 33):
        stride = next(int(r[2]) for r in rows if r[0] == "STRIDE" and int(r[1]) == k)
        assert stride == (k + 31) // 32 * 32
        m = np.zeros((4, stride), np.uint8)
        for r in range(4):
            for c in range(k):
                m[r, c] = (r * 37 + c * 11 + 5) & 255
        bits = [c for c in range(k) if (c * 7 + k) % 3 == 0]

        def step(name):
            got = next(bytes.fromhex(r[2]) for r in rows if r[0] == name and int(r[1]) == k)
            assert got == m.tobytes(), (name, k)
            seen.add((name, k))
        step("INIT")
        m[1, :k] ^= np.array([_gf_mul(int(v), 0x53) for v in m[2, :k]], np.uint8)
        step("AXPY")
        m[3, :k] = [_gf_mul(int(v), 0xCA) for v in m[3, :k]]
        step("SCAL")
        m[[0, 3]] = m[[3, 0]]
        step("SWAP")
        for c in bits:
            m[2, c] ^= 0x8E
        step("AXPYB32")
        m[0, :k] = [1 if c in bits else 0 for c in range(k)]
        step("FILL")
        g = next(r for r in rows if r[0] == "GF2" and int(r[1]) == k)
        assert [int(v) for v in g[2:]] == [(k + 31) // 32, 1, 0, 1 if 0 in bits else 0]
    assert len(seen) == 24


def test_survey_known_answers_are_rederived():
    """The survey's four known answers (survey_kat.json, made once over a stand-in nobody kept) equal what the reference's library
    gives today (ref_kat.json 'survey', regenerated with the rest by test_fixture_is_fresh)."""
    import golden_support as GS
    old, new = GS.load("survey_kat.json"), GOLD["survey"]
    assert new["small"] == old["small"]
    assert new["sha256_of_repair"] == old["sha256_of_repair"] and len(new["sha256_of_repair"]) == 3
    assert new["oti"][0] == old["oti"][0] and new["oti"][1]["common"] == old["oti"][1]["common"]


# ------------------------------------------------------------------------------------------------ 3: the oracle against the reference

def _facts_rows(new):
    common, scheme, F, T, Z, mb, rle = new
    ks = [k for k, n in rle for _ in range(n)]
    return [["new", "ok", "common=" + common, "scheme=" + scheme, "F=%d" % F, "T=%d" % T, "Z=%d" % Z, "maxblocks=%d" % mb],
            ["ks"] + [str(k) for k in ks]], ks, T, F


class OracleObject:
    """the object's blocks as the oracle sees them: source rows (zero padded) and repair symbols on block 0's table row"""

    def __init__(self, orc, F, T, ks):
        self.orc, self.F, self.T, self.ks = orc, F, T, ks
        self.offs = S.block_layout(ks, T)
        self.data = S.kat_bytes(F)
        self.Kp = S.kprime(ks[0])
        self.src = {}

    def block(self, sbn):
        if sbn not in self.src:
            K = self.ks[sbn]
            b = np.zeros(K * self.T, np.uint8)
            part = self.data[self.offs[sbn]:self.offs[sbn] + K * self.T]
            b[:len(part)] = part
            self.src[sbn] = b.reshape(K, self.T)
        return self.src[sbn]

    def symbols(self, sbn, esis):
        """{esi: bytes} as an encoder sends them"""
        K, src = self.ks[sbn], self.block(sbn)
        rep = sorted(set(e for e in esis if e >= K))
        got = {e: src[e].tobytes() for e in esis if e < K}
        if rep:
            r, _, _ = self.orc.encode_block(src, K, self.T, rep, Kp=self.Kp)
            got.update({e: r[i].tobytes() for i, e in enumerate(rep)})
        return got


def _oracle_encode(orc, case, ref):
    rows, ks, T, F = _facts_rows(ref["new"])
    obj = OracleObject(orc, F, T, ks)
    if case["precalc"]:
        rows.append(["precalc", "1"])
    want = {}
    for _, toks in case["groups"]:
        for sbn, lo, hi in toks:
            want.setdefault(sbn, []).extend(range(lo, hi + 1))
    syms = {sbn: obj.symbols(sbn, esis) for sbn, esis in want.items()}
    for _, toks in case["groups"]:
        for sbn, lo, hi in toks:
            for esi in range(lo, hi + 1):
                rows.append(["sym", str(sbn), str(esi), str(T), syms[sbn][esi].hex()])
    return S._one(case, rows, False)


def _oracle_decode(orc, case, ref, script):
    """the reference's add_symbol rules modelled here, the solve by the oracle"""
    rows, ks, T, F = _facts_rows(ref["new"])
    obj = OracleObject(orc, F, T, ks)
    Z, Kp = len(ks), S.kprime(ks[0])
    max_esi = 2 * Kp
    if case["max_esi"] >= 0:
        ok = Kp <= case["max_esi"] < (1 << 24)
        rows.append(["setmax", str(int(ok))])
        if ok:
            max_esi = case["max_esi"]
    out = np.full(F, S.FILL, np.uint8)
    have = {}          # sbn -> dict(K, seen set, order [(esi, bytes)], nrep)

    def blk(sbn):
        if sbn not in have:
            have[sbn] = dict(K=ks[sbn] if sbn < Z else 0, seen=set(), order=[], nrep=0)
        return have[sbn]

    def missing(b):
        return b["K"] - len([e for e in b["seen"] if e < b["K"]])

    def write(sbn, esi, sym):
        at = obj.offs[sbn] + esi * T
        n = max(0, min(T, F - at))
        out[at:at + n] = np.frombuffer(sym, np.uint8)[:n]

    def repair(sbn):
        b = blk(sbn)
        gaps = missing(b)
        if gaps == 0:
            return 1
        if b["nrep"] < gaps:
            return 0
        esis = [e for e, _ in b["order"]]
        ok, rec, _ = orc.decode_block(esis, np.frombuffer(b"".join(s for _, s in b["order"]), np.uint8), b["K"], T, Kp=Kp, max_esi=max_esi)
        if not ok:
            return 0
        for e in range(b["K"]):
            if e not in b["seen"]:
                assert np.array_equal(rec[e], obj.block(sbn)[e]), "the oracle recovered something else than the source"
                write(sbn, e, rec[e].tobytes())
                b["seen"].add(e)
        return 1

    need = {}
    for op in script:
        if op[0] == "a" and op[1] < Z:
            need.setdefault(op[1], []).extend(range(op[2], op[3] + 1))
    syms = {sbn: obj.symbols(sbn, esis) for sbn, esis in need.items()}
    for op in script:
        if op[0] == "n":
            b = blk(op[1])
            rows.append(["num", str(op[1]), str(missing(b)), str(b["nrep"])])
        elif op[0] == "r":
            rows.append(["rep", str(op[1]), str(repair(op[1]))])
        else:
            sbn = op[1]
            for esi in range(op[2], op[3] + 1):
                b = blk(sbn)
                if esi > max_esi:
                    code = -1
                elif missing(b) == 0:
                    code = 1
                elif esi in b["seen"]:
                    code = 2
                else:
                    code = 0
                    sym = syms[sbn][esi]
                    b["seen"].add(esi)
                    b["order"].append((esi, sym))
                    if esi < b["K"]:
                        write(sbn, esi, sym)
                    else:
                        b["nrep"] += 1
                rows.append(["add", str(sbn), str(esi), str(code)])
    for sbn in range(Z):
        b = blk(sbn)
        nm, nr = missing(b), b["nrep"]
        v1 = repair(sbn)
        v2 = repair(sbn)
        rows.append(["final", str(sbn), str(nm), str(nr), str(v1), str(v2), str(missing(b))])
    rows.append(["out", out.tobytes().hex()])
    return S._one(case, rows, False)


def _line_script(line):
    """the script of a decode driver line, back as ops"""
    ops = []
    for w in line.split(" ")[9:]:
        if w[0] in "rn":
            ops.append((w[0], int(w[1:])))
        else:
            sbn, r = w[1:].split(":")
            lo, _, hi = r.partition("-")
            ops.append(("a", int(sbn), int(lo), int(hi or lo)))
    return ops


@pytest.mark.parametrize("cid", [c["id"] for c in S.family("encode")])
def test_oracle_encodes_what_the_reference_encodes(orc, cid):
    case, ref = BY_ID[cid], GOLD["cases"][cid]["ref"]
    got = _oracle_encode(orc, case, ref)
    assert got == ref


@pytest.mark.parametrize("cid", [c["id"] for c in CASES if c["kind"] == "decode"])
def test_oracle_decodes_what_the_reference_decodes(orc, cid):
    case, ref = BY_ID[cid], GOLD["cases"][cid]["ref"]
    if len(case["lines"]) == 1:
        assert _oracle_decode(orc, case, ref, case["script"]) == ref
        return
    K, T = case["obj"][2], case["obj"][1]
    new = ["%016x" % ((K * T << 24) | (T - 1)), "%08x" % 8, K * T, T, 1, 256, [[K, 1]]]      # one block, Al = 8, N = 1
    ones = [_oracle_decode(orc, case, {"new": new}, _line_script(ln)) for ln in case["lines"]]
    assert "".join(str(o["final"][0][2]) for o in ones) == ref["verdicts"]
    assert dict(n=len(ones), sha=S.sha(S.canonical(ones)), verdicts=ref["verdicts"]) == ref


# ------------------------------------------------------------------------------------------------ 4: the host layer against the reference

@pytest.fixture(scope="module")
def host_answers():
    assert os.path.isfile(S.HIP_BIN), "oracle/_ref/ref_kat_hip is not built"
    return S.run_cases(S.HIP_BIN, [c for c in CASES if c["kind"] != "encode"], host=True, timeout=300)


@pytest.mark.parametrize("fam", [f for f in S.FAMILIES if f != "encode"])
def test_host_layer_answers_what_the_reference_answers(host_answers, fam):
    """OTI words, partitioning, add_symbol codes, counts and where source symbols are written through: no solver involved."""
    wrong = []
    for c in S.family(fam):
        got = S.summarise(c, host_answers[c["id"]], host=True)
        want = expected(c["id"], host=c["kind"] != "params")
        if "no_answer" in want:
            want = {"new": "null"}          # where the reference dies or spins this library returns NULL
        if got != want:
            wrong.append((c["id"], got, want))
    assert not wrong, wrong[:3]
