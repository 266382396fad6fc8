"""Worker of tests/test_launch_bounds_emu.py: one group of cases of the fenced launch emulation (launch_emu_support.py), in a
process of its own -- an access outside an array ends the process in the emulation's signal handler, which names the array and the
side.  Prints every case before it starts; exit status 0 = every case bit-exact, no fence hit, the group's forms all reached.

    python launch_bounds_worker.py GROUP        (GROUPS below)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import launch_emu_support as S  # noqa: E402
from util import loss_pattern  # noqa: E402

# symbol sizes: single bytes, a partial last strip, a partial last line group (128 bytes), whole lines
TS = (1, 2, 3, 5, 15, 16, 17, 31, 64, 129, 200, 272)
TS12 = TS + (36, 44, 50)  # 12-byte strips: whole strips / strips + 8 bytes / not a multiple of 4
KS = (10, 101, 257)
# block counts at the octet edges of nrq_map_by_block: 8, 16 and 65 map by block octets (65: a last octet of one block, whose seven
# empty slots per group nrq_map_group must refuse), the others round-robin
NBLKS = (1, 7, 8, 9, 33, 16, 65)
NREPS = (0, 1, 40)

# what a context sets that solve_shape reads.  forced / default: gpu_support's two contexts; full768: the full-size workgroup at
# any size (the instance of big blocks: pipelined movers, late portions, ph_store's fast form); few: eight persistent workgroups,
# so that each runs many work slots (whole line groups, strip-less portions, both staging sets); few64: the same on single waves
CONTEXTS = {
    "forced": {"tiny_any": 1},
    "default": {},
    "full768": {"big_wg": 1},
    "few": {"solve_grid": 8},
    "few64": {"solve_grid": 8, "tiny_any": 1},
    "few768": {"solve_grid": 8, "big_wg": 1},
}
WIDTHS = {
    "w16": {},
    "w12": {"max_wb": 12},
    "w8": {"max_wb": 8},
    "w4": {"max_wb": 4},
    "w2": {"max_wb": 2},
    "w4sb16": {"max_wb": 4, "backsub_sb": 16},
    "w4nosplit": {"max_wb": 4, "no_split": 1},
    "wide2": {"wide_g": 2},
    "wide4": {"wide_g": 4},
}


def sweep(width):
    """encode cases of one strip width: every T with every context, K / block count / repair count / want_inter dealt round"""
    ts = TS12 if width == "w12" else TS
    n = 0
    for ci, (cname, copts) in enumerate(CONTEXTS.items()):
        if width.startswith("wide") and cname in ("full768", "few768", "few64", "forced"):
            continue  # (wide strips have one instance, 256 threads: the other contexts change nothing for them)
        for ti, T in enumerate(ts):
            K = KS[(ti + ci) % 3]
            nblk = NBLKS[n % len(NBLKS)]
            if K == 257 and nblk == 65:
                nblk = 16
            nrep = NREPS[(n // 2) % 3]
            want_inter = (n % 4) != 3 or nrep == 0
            # begin-side placement: right behind the page (aligned rows when the sizes allow), or 1 / 4 / 8 bytes behind it
            mis = (0, 1, 0, 4, 0, 8)[n % 6]
            n += 1
            yield dict(kind="encode", K=K, T=T, nblk=nblk, nrep=nrep, want_inter=want_inter, opts=dict(WIDTHS[width], **copts), mis=mis,
                       tag="%s/%s" % (width, cname))


def decode_cases():
    """a few lost symbols, overhead 0 and 5, with and without the intermediate symbols, one undecodable block in most batches; both
    sites that lay out a decode's arrays"""
    n = 0
    for width in ("w16", "w12", "w8", "w4", "w2", "w4sb16", "wide2"):
        for cname in ("forced", "default", "few", "full768"):
            if width.startswith("wide") and cname != "default":
                continue
            for T in (1, 17, 64, 129, 200):
                K = KS[n % 3]
                nblk = (7, 8, 9, 16, 33, 2)[n % 6]
                yield dict(kind="decode", K=K, T=T, nblk=nblk, loss=(0.05, 0.1, 0.3)[n % 3], overhead=(0, 5)[n % 2], want_inter=n % 3 == 0,
                           site=("host", "device")[(n // 2) % 2], bad_block=(None if n % 4 == 3 else (n * 5) % nblk),
                           opts=dict(WIDTHS[width], **CONTEXTS[cname]), mis=(0, 1, 4, 8)[n % 4], tag="decode/%s/%s" % (width, cname))
                n += 1


def needview_cases():
    """decodes without intermediate symbols on device plans that have no out view (the option plan_no_out_view): the needed-pivot view
    (needslot[nneed], wneed at stride need_pad) ends the arena, and the back-substitution of every strip walks it -- 16-, 12- and
    8-byte strips and 4-byte ones that do not split, every workgroup size"""
    n = 0
    for width in ("w16", "w12", "w8", "w4nosplit"):
        for cname in ("forced", "default", "few", "full768"):
            for T in (1, 17, 64, 200):
                K = KS[n % 3]
                yield dict(kind="decode", K=K, T=T, nblk=(7, 8, 9, 2)[n % 4], loss=(0.05, 0.1, 0.3)[(n // 3) % 3], overhead=(0, 5)[n % 2],
                           want_inter=False, site="device", bad_block=(None if n % 4 == 3 else (n * 5) % (7, 8, 9, 2)[n % 4]), no_out_view=True,
                           opts=dict(WIDTHS[width], **CONTEXTS[cname]), mis=(0, 1, 4, 8)[n % 4], tag="needview/%s/%s" % (width, cname))
                n += 1


def big_cases():
    for K, T in ((1024, 129), (3100, 64)):
        for cname in ("forced", "default", "few768"):
            for width in ("w16", "w12", "w4"):
                yield dict(kind="encode", K=K, T=T, nblk=(1 if cname == "default" else 3), nrep=9, want_inter=True,
                           opts=dict(WIDTHS[width], **CONTEXTS[cname]), mis=0, tag="big/%s/%s" % (width, cname))
    yield dict(kind="decode", K=1024, T=129, nblk=3, loss=0.1, overhead=2, want_inter=False, site="host", bad_block=None,
               opts=CONTEXTS["default"], mis=1, tag="big/decode")


def edge_cases(orc):
    """cases built for one rule each"""
    # NRQ_STORE_SLACK: the fast form of ph_store (the full-size workgroup) reads a trip of 32 entries from the start of EVERY lane's list,
    # and a second one when a lane of the wave has a list of NRQ_LT_LIST_MAX = 33.  No ESI has such a list (rq_math.h: 32 at most), so
    # these generated symbols are made up: sums of the intermediate symbols a list names.  The array's last list is the list of 33 /
    # a list of ONE entry with the list of 33 in its wave (the worst case: 63 entries past the end -- the
    # emulation runs a wave's lanes in step, tests/emu/wave_emu.h, so that lane does take the second trip) / the same with a wave full of lists.
    K = 257
    L = S.nanorq_amd.params(K)["L"]
    cols33 = [(7 * i + 3) % L for i in range(33)]
    some = [[(5 * q + i) % L for i in range(3 + q % 9)] for q in range(62)]
    for name, lists in (("the last list has 33 entries", some[:5] + [cols33]), ("a list of one entry behind one of 33", [cols33, [11]]),
                        ("a wave of lists, 33 first, one entry last", [cols33] + some + [[12]]), ("a list of 33 alone", [cols33]),
                        ("real lists, the last (ESI 298) of 32 entries", None)):
        for cname in ("full768", "few768"):
            for wopts in ({}, {"max_wb": 12}, {"max_wb": 4, "no_split": 1}):
                c = dict(kind="encode", K=K, T=64, nblk=2, nrep=len(lists) if lists else 42, want_inter=False, opts=dict(wopts, **CONTEXTS[cname]),
                         mis=0, tag="edge/slack: " + name)
                if lists:
                    c["lists"] = lists
                yield c
    # the output staging stride: ONE element to stage (ostage_stride is a single 256-byte step), 17 and 33 elements of 16 bytes (the last
    # element begins a new 256-byte step), in launches whose workgroups run several whole-line slots -- the last strip's buffer of the
    # second staging set of the last workgroup ends the staging area
    for width in ("w16", "w12", "w8", "w2", "w4nosplit", "wide2"):
        for nrep in (1, 17, 33):
            for cname in ("few", "few64", "few768"):
                if width == "wide2" and cname != "few":
                    continue
                yield dict(kind="encode", K=10, T=(384 if width == "w12" else 512 if width == "wide2" else 256), nblk=8, nrep=nrep, want_inter=False,
                           opts=dict(WIDTHS[width], **CONTEXTS[cname]), mis=0, tag="edge/ostage: %d elements" % nrep)


def seed0_trials():
    """the 30 (K, T, nblk, nrep) of tests/test_gpu_fuzz.py::_random_shapes for seed 0: the same generator, the same calls in the same
    order (the draws for the loss rate, the overhead and the block to compare are made to keep the stream in step)"""
    seed = 0
    rng = np.random.default_rng(4000 + seed)
    out = []
    for trial in range(30):
        K = int(rng.choice([1, 2, 7, 10, 11, 26, 55, 100, 101, 257, 400, 777, 1024, 1500, 2049, 2600, 3100]))
        T = int(rng.choice([1, 2, 3, 5, 8, 15, 16, 17, 31, 40, 64, 100, 128, 129, 200, 272]))
        nblk = int(rng.choice([1, 2, 3, 7, 8, 9, 16, 33]))
        if K * T * nblk > 24 << 20:
            nblk = max(1, (24 << 20) // (K * T))
        p = float(rng.choice([0.02, 0.1, 0.3, 0.6]))
        oh = int(rng.choice([0, 0, 1, 2, 5]))
        lost = [loss_pattern(K, p, seed=seed * 977 + trial, block=b) for b in range(nblk)]
        nrep = max(len(x) for x in lost) + oh
        rng.integers(nblk)
        out.append((K, T, nblk, nrep))
    return out


def seed0_cases():
    for i, (K, T, nblk, nrep) in enumerate(seed0_trials()):
        yield dict(kind="encode", K=K, T=T, nblk=nblk, nrep=nrep, want_inter=True, opts=CONTEXTS["forced"], mis=0, tag="seed0/trial%d" % i)


def forced_cases(orc, K):
    """the calls of tests/test_gpu_backsub_forms.py at block size K, one for one (forced_inact_support.GPU_CASES: plans at a forced
    number of inactive columns, which moves the cu, x and t4 regions of the image to sizes no other launch has): the same options,
    blocks, symbol sizes, reception and n; the launch must be the one the row names"""
    import forced_inact_support as F
    for i, (form, u, n_enc, n_dec, strip, threads, sb) in enumerate(F.GPU_CASES):
        f = F.FORMS[form]
        if f["K"] != K:
            continue
        common = dict(K=K, nblk=F.NBLK, opts=dict(F.GPU_FORCED, **f["opts"]), mis=0, expect=dict(wb=strip, NT=threads, backsub_strip=sb),
                      tag="forced/%s u=%d" % (form, u))
        for kind, T, want_inter in F.calls_of(i):
            if kind == "encode":
                yield dict(common, kind="encode", T=T, nrep=F.NREP, want_inter=want_inter, extra_inact=n_enc)
            else:
                yield dict(common, kind="decode", T=T, loss=0.1, overhead=2, want_inter=want_inter, site="host", bad_block=None,
                           extra_inact=n_dec, lost_all=F.gpu_reception(orc, K)[0])


def forced_must(K):
    """every row of the table at this K, reached at its number of inactive columns by the encode and by the decode"""
    import forced_inact_support as F
    return [dict(u=u, wb=strip, NT=threads, backsub_strip=sb, skipped=0) for form, u, _, _, strip, threads, sb in F.GPU_CASES
            if F.FORMS[form]["K"] == K]


FORCED_KS = (100, 1000, 3000, 5200, 10000, 15000)
GROUPS = {w: (lambda orc, w=w: sweep(w)) for w in WIDTHS}
GROUPS.update(decode=lambda orc: decode_cases(), needview=lambda orc: needview_cases(), big=lambda orc: big_cases(), seed0=lambda orc: seed0_cases(), edge=edge_cases)
GROUPS.update({"forced_k%d" % K: (lambda orc, K=K: forced_cases(orc, K)) for K in FORCED_KS})

# the forms a group must have reached (checked at its end): keys of the launch record
MUST = {
    "w16": [dict(NT=64), dict(NT=256), dict(NT=768), dict(AL=1), dict(AL=0), dict(by_block=1), dict(by_block=0), dict(multi=1), dict(stripless=1)],
    "w12": [dict(NT=768, wb=12, AL=1), dict(NT=768, wb=12, AL=0), dict(multi=1), dict(stripless=1)],
    "w8": [dict(wb=8, NT=64), dict(wb=8, NT=256), dict(wb=8, NT=768), dict(AL=1), dict(multi=1), dict(stripless=1)],
    "w4": [dict(wb=4, split=1, NT=64), dict(wb=4, split=1, NT=768), dict(AL=1), dict(backsub_strip=32), dict(multi=1)],
    "w2": [dict(wb=2, split=1, NT=64), dict(wb=2, split=1, NT=768), dict(multi=1)],
    "w4sb16": [dict(wb=4, split=1, backsub_strip=16)],
    "w4nosplit": [dict(wb=4, split=0, NT=768), dict(wb=4, split=0, NT=64)],
    "wide2": [dict(G=2), dict(G=2, multi=1)],
    "wide4": [dict(G=4)],
    "decode": [dict(split=1), dict(split=0), dict(by_block=1), dict(NT=768), dict(NT=64), dict(G=2), dict(skipped=1), dict(AL=1)],
    "needview": [dict(NT=768, wb=16, split=0), dict(NT=256, wb=16, split=0), dict(NT=64, wb=16, split=0), dict(wb=12, split=0), dict(wb=8, split=0),
                 dict(wb=4, split=0), dict(skipped=1), dict(skipped=0)],
    "big": [dict(NT=768, wb=16), dict(NT=256, wb=16)],
    "seed0": [dict(NT=64), dict(NT=256)],
    "edge": [dict(NT=768, wb=16, split=0), dict(NT=768, wb=12), dict(NT=768, wb=4, split=0), dict(multi=1, lsub=3, wb=16, NT=64),
             dict(multi=1, lsub=3, wb=16, NT=256), dict(multi=1, lsub=3, wb=16, NT=768), dict(multi=1, G=2)],
}
MUST.update({"forced_k%d" % K: forced_must(K) for K in FORCED_KS})


def main():
    group = sys.argv[1]
    import oracle
    oracle.lib()
    L = S.lemu()
    L.lemu_install_handler()
    seen = []
    n = 0
    for case in GROUPS[group](oracle):
        for side in (0, 1):
            c = dict(case)
            tag, kind, mis = c.pop("tag"), c.pop("kind"), c.pop("mis")
            line = "%s %s side=%d mis=%d %r" % (tag, kind, side, mis if side else 0, c)
            print("case:", line, flush=True)
            L.lemu_set_case(line.encode()[:250])
            run = S.run_encode if kind == "encode" else S.run_decode
            try:
                d = run(oracle, side=side, mis=mis, **c)
            except AssertionError as e:
                print("FAILED:", line, "\n ", e, flush=True)
                return 1
            d["multi"] = int(d["nslots"] > d["grid"])
            sub = 1 << d["lsub"]
            d["stripless"] = int(d["multi"] and d["nstrips"] % sub != 0)
            d["skipped"] = int(kind == "decode" and d.get("solved", 0) < c["nblk"])
            seen.append(d)
            n += 1
    missing = [m for m in MUST[group] if not any(all(d[k] == v for k, v in m.items()) for d in seen)]
    if missing:
        print("FAILED: the group never reached", missing, flush=True)
        return 1
    print("ok: %d runs, %d forms" % (n, len({(d["wb"], d["NT"], d["G"], d["AL"], d["split"], d["by_block"], d["lsub"]) for d in seen})), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
