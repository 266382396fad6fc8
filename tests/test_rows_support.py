"""CPU tier of the row-pipeline probe (tests/test_gpu_rows.py): the plain replay that serves as the reference there equals the
orders the device runs on every stream of the case table, stops being equal once the generator ignores rule R2, every stream of
the table is legal and fits the LDS, the macros the probe's instance table rests on are where they were, and the probe builds
without a GPU."""
import os
import re

import numpy as np
import pytest

import rows_support as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = [("fwd", 24), ("fwd", 36), ("fwd", 60), ("fwd", 120), ("rev", 0), ("wide", 2), ("wide", 4), ("wide", 8)]
MODEL = {"fwd": R.model_forward, "wide": R.model_wide, "rev": R.model_reverse}
REPLAY = {"fwd": R.replay_forward, "wide": R.replay_forward, "rev": R.replay_reverse}


def _streams(family, ring):
    """every stream a launch of the family uses: the shared small images, the 2-byte kinds, every width's full image"""
    out = list(R.small_cases(family, ring))
    if family == "fwd":
        out += list(R.small_cases(family, ring, True))
    widths = {w for f, r, w in R.INSTANCES.values() if (f, r) == (family, ring)}
    for w in sorted(widths):
        out += list(R.extreme_cases(family, ring, R.FULL[16] // ring if family == "wide" else R.FULL[w]))
    return out


@pytest.mark.parametrize("family,ring", FAMILIES)
def test_replay_equals_the_pipelined_order_on_every_case(family, ring):
    """the whole case table of the GPU tier, not a sample: on streams that obey R1 and R2 the order of the device (forward: apply
    q - NRQ_PIPE, read q; wide: read q, apply q - 1; reverse: from the last row down) gives the image of the plain replay"""
    cases = _streams(family, ring)
    assert len(cases) > 100
    for c in cases:
        img = c.image(2)  # (the orders do not depend on the width: two bytes a slot)
        want = REPLAY[family](img.copy(), c.dst, c.src)
        got = MODEL[family](img.copy(), c.dst, c.src)
        assert np.array_equal(got, want), c.name
        assert not want[:R.SCRATCH].any(), c.name
    # the forward cases under the one-row-deep order of the wide form as well (a legal stream is legal at any smaller depth)
    if family == "fwd" and ring == 24:
        for c in cases:
            img = c.image(2)
            assert np.array_equal(R.model_wide(img.copy(), c.dst, c.src), R.replay_forward(img.copy(), c.dst, c.src)), c.name


def test_the_models_are_sensitive_to_rule_r2():
    """with R2 switched off in the generator the pipelined orders and the replay disagree on most streams: the agreement above is the
    rules' doing, not the models' being the replay in other words"""
    bad = {"fwd": 0, "rev": 0, "legal": 0}
    n = 100
    for seed in range(n):
        dst, src = R.gen_stream(seed, 30, range(R.SCRATCH, 70), "a", hazard=False)
        words = R.pack(dst, src)
        assert R.obeys(words, 30, 70, (1,))
        bad["legal"] += R.obeys(words, 30, 70, (1, 2))
        img = R.Case("x", 30, 70, dst, src, seed).image(2)
        bad["fwd"] += not np.array_equal(R.model_forward(img.copy(), dst, src), R.replay_forward(img.copy(), dst, src))
        bad["rev"] += not np.array_equal(R.model_reverse(img.copy(), dst, src), R.replay_reverse(img.copy(), dst, src))
    assert bad["legal"] < n // 10 and bad["fwd"] > n // 2 and bad["rev"] > n // 2, bad
    # ... and the check refuses what the generator must not make: a row that reads its own target, an index past the image
    dst, src = R.gen_stream(1, 8, range(R.SCRATCH, 200), "b")
    d2 = dst.copy(); d2[3, 5] = src[3, 9]
    with pytest.raises(AssertionError, match="R1"):
        R.check_stream(R.pack(d2, src), 8, 200)
    s2 = src.copy(); s2[4, 0] = dst[3, 0]
    with pytest.raises(AssertionError, match="R[12]"):
        R.check_stream(R.pack(dst, s2), 8, 200)
    d3 = dst.copy(); d3[0, 0] = 200
    with pytest.raises(AssertionError, match="outside"):
        R.check_stream(R.pack(d3, src), 8, 200)
    w = R.pack(dst, src); w[R.op_index(9, 3)] = 0x00410042
    with pytest.raises(AssertionError, match="padding"):
        R.check_stream(w, 8, 200)


@pytest.mark.parametrize("name", sorted(R.INSTANCES))
def test_case_table_is_legal_and_complete(name):
    """every stream of an instance's launch passes R1, R2 and the bounds of its image, every image fits the LDS, and the table holds
    what it is meant to: every nrows of the instance's loop edges with every kind, full rows of 64 ops, 64 lanes on one target,
    and -- on the full image -- the first real slot, the last index and both sides of 0x8000 in both fields"""
    family, ring, width = R.INSTANCES[name]
    cases = R.instance_cases(name)
    nrows = R.fwd_nrows(ring) if family == "fwd" else list(R.REV_NROWS) if family == "rev" else R.wide_nrows(ring)
    kinds = set(R.KINDS) | {"e"} | (set(R.KINDS_W2) if width == 2 else set()) | ({"f"} if family == "wide" else set())
    seen = set()
    srcs, dsts = set(), set()
    full = R.FULL[16] // ring if family == "wide" else R.FULL[width]
    for c in cases:
        c.check()  # (R1, R2, the bounds, and that the packed words are the stream)
        d, s = c.dst, c.src
        assert c.nslots * width <= R.LDS_MAX and d.shape == (c.nrows, R.ROW) and not c.words.flags.writeable
        kind = c.name.split("-")[2]
        seen.add((c.nrows, kind))
        real = d >= R.SCRATCH
        if kind == "b" and c.nrows:
            assert real.all()
        if kind == "d" and c.nrows:
            assert all(len(set(row.tolist())) == 1 for row in d) and real.all()
        if kind == "d2" and c.nrows:
            assert all(len(set(row.tolist())) == 2 and len(set((row // 2).tolist())) == 1 for row in d)
        if kind == "e":
            assert c.nslots == full
            srcs |= set(s[real].tolist())
            dsts |= set(d[real].tolist())
    assert seen == {(n, k) for n in nrows for k in kinds}
    want = {R.SCRATCH, full - 1} | ({0x7FFF, 0x8000} if full > 0x8000 else set())
    assert want <= srcs and want <= dsts, (want - srcs, want - dsts)
    assert (full + 1) * width > R.LDS_MAX or full == 65536, "the full image is the largest the LDS, or a 16-bit field, holds"


def test_pinned_macros():
    """the probe's instance table (tests/gpu/rows_probe.hip) takes its rings from solve_roles.h and rows_support restates them:
    the #defines they rest on, read from the sources"""
    dev = open(os.path.join(ROOT, "nanorq_amd", "csrc", "nrq_device.hip")).read()
    roles = open(os.path.join(ROOT, "nanorq_amd", "csrc", "solve_roles.h")).read()
    plan = open(os.path.join(ROOT, "nanorq_amd", "csrc", "plan.h")).read()

    def define(text, name):
        found = re.findall(r"^#define %s (\S+)" % name, text, re.M)
        assert len(found) == 1, (name, found)
        return found[0]

    assert define(roles, "NRQ_RING_TINY") == "24u"
    assert define(roles, "NRQ_RING_5W") == "36u"
    assert define(roles, "NRQ_RING_4W") == "NRQ_RING"
    assert define(roles, "NRQ_BIG_RING") == "NRQ_RING_MAX"
    assert define(roles, "NRQ_W12_FW") == "3"
    assert define(plan, "NRQ_PIPE") == "2u"
    assert define(plan, "NRQ_RING_MULT") == "5u"
    assert (R.PIPE, R.RING, R.RING_MAX, R.PAD_ROWS) == (2, 60, 120, 246)
    # the rings of the table are those values, and the planner kernels take the default ring
    assert {r for f, r, w in R.INSTANCES.values() if f == "fwd"} == {24, 36, R.RING, R.RING_MAX}
    assert re.search(r"fwd_rows<16>\(ops_, pl_wfast_rows\(c\), tid\)", dev) and re.search(r"fwd_rows<2>\(gptr<uint32_t>", dev)
    assert re.search(r"rev_rows<4>\(ops_, pl_wfast_rows\(c\), tid\)", dev)


def test_probe_builds_without_a_gpu():
    """build_rows_probe cross-compiles; the library's instance table is the one rows_support restates (loading it needs no device)"""
    from nanorq_amd import build as nbuild
    path = nbuild.build_rows_probe()
    assert os.path.isfile(path) and os.path.basename(path) == "librows_probe.so"
    inst = R.probe_instances()
    assert {n: w for n, (i, w) in inst.items()} == {n: w for n, (f, r, w) in R.INSTANCES.items()}
    # a stream that names an index outside the LDS is refused before anything is launched
    c = next(c for c in R.small_cases("rev", 0) if c.nrows == 17 and c.nslots == 200 and c.name.split("-")[2] == "b")
    index = inst["rev_rows<16>"][0]
    rec = (R.ProbeCase * 1)()
    buf = np.zeros(1024, np.uint8)
    rec[0].ops, rec[0].ops_words, rec[0].nrows = c.words.ctypes.data, c.words.size, c.nrows
    rec[0].image_in = rec[0].image_out = buf.ctypes.data
    assert R.probe().rows_probe_run(index, rec, 1, 1024) == -2
    assert R.probe().rows_probe_run(index, rec, 1, 1000) == -1
