#!/usr/bin/env python3
"""Regenerates tests/golden/ref_kat.json: what the REFERENCE's own library answers to the case table of tests/ref_kat_support.py.

Needs oracle/_ref/ref_kat (oracle/Makefile: the reference's lib sources read in place, over the stand-in field library of
oracle/refshim/), so it runs where the reference tree is, and only there.  The file holds data only: inputs, return codes, counts,
verdicts and SHA-256 digests, with the first bytes of a few symbols so that a mismatch can be read.

Every run of the reference is a child process with a time limit: the reference aborts on paths it does not handle, divides by
zero or spins on parameters it does not reject.  Such a case is kept as {"no_answer": "SIGFPE" | "timeout" | ...}.

    python tools/gen_ref_kat.py                 write tests/golden/ref_kat.json
    python tools/gen_ref_kat.py --out FILE      write elsewhere
    python tools/gen_ref_kat.py --search-seed   print, seed by seed, how many verdict receptions the reference refuses
"""
import argparse
import concurrent.futures
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_kat_support as S  # noqa: E402

REF_FILES = ["lib/bitmask.c", "lib/io.c", "lib/nanorq.c", "lib/params.c", "lib/precode.c", "lib/rand.c", "lib/sched.c", "lib/spmat.c",
             "lib/tuple.c", "lib/wrkmat.c", "include/*.h"]
COMPILER_LINE = ("cc -std=c99 -D_DEFAULT_SOURCE -D_FILE_OFFSET_BITS=64 -O2 -Werror=implicit-function-declaration -I$(REF)/include "
                 "-Irefshim ref_kat.c refshim/refshim.c $(REF)/lib/*.c -lm")
SHIM_FILES = ["gf2.h", "oblas.h", "octmat.h", "refshim.c"]


def shim_sha():
    blob = b""
    for f in SHIM_FILES:
        with open(os.path.join(ROOT, "oracle", "refshim", f), "rb") as fh:
            blob += fh.read()
    return S.sha(blob)


def _chunks(table, n):
    """the slow cases first and spread out, so that no worker ends up with all of them"""
    order = sorted(table, key=lambda c: -sum(len(ln) for ln in c["lines"]))
    return [order[i::n] for i in range(n) if order[i::n]]


def run_table(table, workers=8):
    """full and --host answers of the reference for every case of the table"""
    ref, host = {}, {}
    with concurrent.futures.ThreadPoolExecutor(workers) as pool:
        # params cases answer at once or never: a short limit, so that the ones the reference spins on cost seconds
        par = [c for c in table if c["kind"] == "params"]
        rest = [c for c in table if c["kind"] != "params"]
        full = [pool.submit(S.run_cases, S.REF_BIN, ch, False, 900, 120) for ch in _chunks(rest, workers)]
        full.append(pool.submit(S.run_cases, S.REF_BIN, par, False, 5, 3))
        hst = pool.submit(S.run_cases, S.REF_BIN, rest, True, 300, 20)
        for f in full:
            ref.update(f.result())
        host.update(hst.result())
    return ref, host


def survey(timeout=300):
    """the four known-answer tests of tests/golden/survey_kat.json, from the reference's own code"""
    shapes = [(10, 8, 10, 13), (100, 1024, 100, 110), (1024, 1280, 1024, 1076), (8192, 1280, 8192, 8208)]
    lines = ["encode sv%d %d %d %d 0 8 1 0 0:%d-%d" % (i, K * T, T, K, lo, hi - 1) for i, (K, T, lo, hi) in enumerate(shapes)]
    recs, trouble = S.run_driver(S.REF_BIN, lines, timeout=timeout)
    if trouble:
        raise RuntimeError("survey known answers: %r" % (trouble,))
    out = {"small": None, "sha256_of_repair": [], "oti": []}
    for i, (K, T, lo, hi) in enumerate(shapes):
        rows = recs["sv%d" % i]
        syms = [r for r in rows if r[0] == "sym"]
        kv = dict(x.split("=") for x in next(r for r in rows if r[0] == "new")[2:])
        if i == 0:
            out["small"] = {"K": K, "T": T, "symbols": {r[2]: r[4] for r in syms}}
        else:
            out["sha256_of_repair"].append({"K": K, "T": T, "esi_lo": lo, "esi_hi": hi,
                                            "sha256": S.sha(bytes.fromhex("".join(r[4] for r in syms)))})
        if K in (10, 8192):
            out["oti"].append({"K": K, "T": T, "common": "0x" + kv["common"], "scheme": "0x" + kv["scheme"]})
    return out


def generate(seed=None):
    t0 = time.time()
    table = S.cases(seed)
    ref, host = run_table(table)
    doc = {
        "provenance": {
            "what": "answers of the reference's own lib/*.c (compiled in place over the stand-in field library oracle/refshim/, which is "
                    "this project's code, not upstream oblas) to the cases of tests/ref_kat_support.py, through oracle/ref_kat.c; "
                    "payload byte i = ((uint32) i * 2654435761) >> 24",
            "reference_files": REF_FILES,
            "refshim_sha256": shim_sha(),
            "compiler_line": COMPILER_LINE,
            "wall_seconds": None,
        },
        "verdict_seed": S.VERDICT_SEED if seed is None else seed,
        "dropped": S.DROPPED,
        "deviations": S.DEVIATIONS,
        "survey": survey(),
        "cases": {},
    }
    for c in table:
        e = {"ref": S.summarise(c, ref[c["id"]])}
        if c["id"] in host:
            e["host"] = S.summarise(c, host[c["id"]], host=True)
        # (params cases have no host entry: --host and the full run do the same for them)
        doc["cases"][c["id"]] = e
    # parameters the reference refuses to answer (it dies or never returns): this library returns NULL for each
    doc["params_no_answer"] = {c["id"]: dict(obj=list(c["obj"]), why=doc["cases"][c["id"]]["ref"]["no_answer"])
                               for c in table if c["kind"] == "params" and "no_answer" in doc["cases"][c["id"]]["ref"]}
    doc["provenance"]["wall_seconds"] = round(time.time() - t0, 1)
    return doc


def dump(doc):
    """canonical text: keys sorted, one line per case"""
    head = {k: v for k, v in doc.items() if k != "cases"}
    lines = ["{", '"cases":{']
    lines += ["%s:%s%s" % (json.dumps(k), S.canonical(v), "," if i + 1 < len(doc["cases"]) else "")
              for i, (k, v) in enumerate(sorted(doc["cases"].items()))]
    lines.append("},")
    lines += [json.dumps(head, indent=1, sort_keys=True)[2:]]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=S.GOLDEN)
    ap.add_argument("--search-seed", action="store_true")
    a = ap.parse_args()
    if not os.path.isfile(S.REF_BIN):
        sys.exit("oracle/_ref/ref_kat is not built (make -C oracle _ref/ref_kat, where the reference tree is)")
    if a.search_seed:
        for seed in range(1, 50):
            table = [c for c in S.cases(seed) if c["family"] == "decode_verdicts"]
            ref, _ = run_table(table)
            v = "".join(S.summarise(c, ref[c["id"]])["verdicts"] for c in table if c["id"].endswith("oh0"))
            print("seed %d: %d of %d receptions at overhead 0 refused" % (seed, v.count("0"), len(v)), flush=True)
            if v.count("0") >= 3:
                break
        return
    doc = generate()
    with open(a.out, "w") as f:
        f.write(dump(doc))
    print("%s: %d cases, %d bytes, %.1f s" % (a.out, len(doc["cases"]), os.path.getsize(a.out), doc["provenance"]["wall_seconds"]))


if __name__ == "__main__":
    main()
