"""GPU tier of the reference known answers: the driver that produced tests/golden/ref_kat.json over the reference's own library,
built over THIS library (oracle/_ref/ref_kat_hip), must print the same records; and the receptions whose verdicts the reference
gave go through the block-level ABI in batches, on both context kinds.  Only the committed JSON and the tree's own binaries are used."""
import os

import numpy as np
import pytest

import ref_kat_support as S
from util import payload

pytestmark = pytest.mark.gpu

GOLD = S.load_golden()
TIMEOUT = {"params": 60, "encode": 300, "decode_orders": 120, "decode_verdicts": 300, "decode_scattered": 300}   # seconds, per child
_RUNS = {}


def _run_families():
    """One child process per family, one after the other, each under its own limit; after the first that fails none is started."""
    if _RUNS:
        return _RUNS
    failed = None
    for fam in S.FAMILIES:
        if failed:
            _RUNS[fam] = RuntimeError("not run: %s" % failed)
            continue
        try:
            _RUNS[fam] = S.run_cases(S.HIP_BIN, S.family(fam), timeout=TIMEOUT[fam], go_on=False)
        except (RuntimeError, OSError) as e:
            failed = "family %s failed (%s)" % (fam, e)
            _RUNS[fam] = RuntimeError(failed)
    return _RUNS


def _untouched_where_refused(case, rows):
    """the symbols a refused block still misses keep the driver's fill in the output buffer"""
    if isinstance(rows, dict) or not any(r[0] == "out" for r in rows):
        return True
    ks = [int(k) for k in next(r for r in rows if r[0] == "ks")[1:]]
    T = int(dict(x.split("=") for x in next(r for r in rows if r[0] == "new")[2:])["T"])
    out = np.frombuffer(bytes.fromhex(next(r for r in rows if r[0] == "out")[1]), np.uint8)
    offs = S.block_layout(ks, T)
    for f in (r for r in rows if r[0] == "final"):
        sbn, refused = int(f[1]), f[4] == "0"
        if not refused:
            continue
        held = set(int(r[2]) for r in rows if r[0] == "add" and int(r[1]) == sbn and r[3] == "0")
        for esi in range(ks[sbn]):
            if esi not in held:
                part = out[offs[sbn] + esi * T:offs[sbn] + (esi + 1) * T]
                if len(part) and not (part == S.FILL).all():
                    return False
    return True


@pytest.mark.parametrize("fam", S.FAMILIES)
def test_same_driver_same_answers(fam):
    """OTI, counts, return codes, every symbol digest, every verdict, every output digest: as the reference's library gave them."""
    assert os.path.isfile(S.HIP_BIN), "oracle/_ref/ref_kat_hip is not built"
    got = _run_families()[fam]
    if isinstance(got, Exception):
        raise got
    wrong, refused = [], 0
    for c in S.family(fam):
        dev = GOLD["deviations"].get(c["id"])
        want = dev["ours"] if dev else GOLD["cases"][c["id"]]["ref"]
        if "no_answer" in want:
            want = {"new": "null"}              # where the reference dies or spins this library returns NULL
        have = S.summarise(c, got[c["id"]])
        if have != want:
            wrong.append((c["id"], have, want))
        for rows in got[c["id"]]:
            refused += sum(1 for r in rows if r[0] == "final" and r[4] == "0")
            assert _untouched_where_refused(c, rows), "%s: a refused block's missing symbols were written" % c["id"]
    assert not wrong, wrong[:2]
    if fam == "decode_verdicts":
        assert refused >= 3


# ------------------------------------------------------------------------------------------------ the block-level ABI, in batches

def _receptions(name):
    """(K, T, [(lost, reps, verdict)]) of one group: a verdict K with its 150 receptions, or a scattered K with its receptions"""
    if name.startswith("v"):
        K = int(name[1:])
        recs = []
        for c in S.family("decode_verdicts"):
            if c["obj"][2] == K:
                bits = GOLD["cases"][c["id"]]["ref"]["verdicts"]
                recs += [(r["lost"], r["reps"], int(b)) for r, b in zip(c["receptions"], bits)]
        return K, 16, recs
    K = int(name[1:])
    recs = [(c["reception"]["lost"], c["reception"]["reps"], GOLD["cases"][c["id"]]["ref"]["final"][0][2])
            for c in S.family("decode_scattered") if c["obj"][2] == K]
    return K, 16, recs * (8 // len(recs))       # 8 blocks a call: every reception with more than one payload


GROUPS = ["v%d" % K for K in S.VERDICT_KS] + ["s1000", "s3000", "s8192", "s10000"]


@pytest.mark.parametrize("kind", ["forced", "default"])
@pytest.mark.parametrize("name", GROUPS)
def test_receptions_in_batches_through_the_block_abi(name, kind):
    """8 to 16 receptions of one K a call, so that the planner kernel gets them as a batch: each block's verdict is the reference's,
    recovered blocks equal the source, refused blocks are left as they came."""
    import gpu_support
    G = gpu_support.bound(kind)
    K, T, recs = _receptions(name)
    per_call = 15 if name.startswith("v") else 8
    assert len(recs) % per_call == 0
    seen_refused = 0
    for at in range(0, len(recs), per_call):
        part = recs[at:at + per_call]
        n = len(part)
        src = np.stack([payload(K * T, seed=300 + at, block=b).reshape(K, T) for b in range(n)])
        esis = sorted(set(e for _, reps, _ in part for e in reps))
        col = {e: i for i, e in enumerate(esis)}
        rep, _ = G.gpu_encode(src, K, T, esis)
        work = src.copy()
        for b, (lost, _, _) in enumerate(part):
            work[b][lost] = S.FILL
        given = work.copy()
        st, out, _ = G.gpu_decode(work, K, T, [np.array(l, np.uint32) for l, _, _ in part], [np.array(r, np.uint32) for _, r, _ in part],
                                  [rep[b][[col[e] for e in r]] for b, (_, r, _) in enumerate(part)])
        stats = G.ctx().stats()
        assert [int(bool(x)) for x in st] == [v for _, _, v in part], (name, at)
        for b, (_, _, v) in enumerate(part):
            assert np.array_equal(out[b], src[b] if v else given[b]), (name, at, b, v)
            seen_refused += not v
        if K >= 1000:
            assert stats["planner"] == 1 and stats["host_planned"] == 0, stats
    if name in ("v10", "v26", "v257"):
        assert seen_refused >= 1        # (seed 4: the reference refuses one reception at K=10, two at 26, one at 257)
