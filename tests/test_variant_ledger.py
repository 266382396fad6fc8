"""CPU tier: every kernel instantiation compiled into libnanorq_hip.so has a row in tests/variant_ledger.py -- pinned at a
default-option shape (tests/test_gpu_variants.py), covered by a named test that forces it, or recorded as never launched with
the reason.  A variant added without a row fails here."""
import os
import re
import shutil
import subprocess

import pytest

import variant_ledger as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SYM = re.compile(r"\bvoid (%s)<([^<>]*)>\(" % "|".join(V.KERNELS))


def _instantiations():
    from nanorq_amd import build
    path = build.build_lib()
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-C", path], check=True, capture_output=True, text=True).stdout
    found = set()
    for line in out.splitlines():
        if "__device_stub__" in line:
            continue
        m = _SYM.search(line)
        if m:
            found.add((m.group(1), tuple(a.strip() for a in m.group(2).split(","))))
    return found


@pytest.fixture(scope="module")
def inst():
    return _instantiations()


def _test_exists(ref):
    path, name = ref.split("::")
    with open(os.path.join(ROOT, path)) as f:
        return re.search(r"(?m)^def %s\(" % re.escape(name), f.read()) is not None


def test_every_kernel_family_is_compiled(inst):
    assert {k for k, _ in inst} == set(V.KERNELS)
    assert sum(1 for k, _ in inst if k == "nrq_solve_kernel") >= 37


def test_every_instantiation_has_a_ledger_row(inst):
    missing = sorted("%s<%s>" % (k, ", ".join(a)) for k, a in inst if V.ledger_row(k, a) is None)
    assert not missing, "kernel variants without a row in tests/variant_ledger.py: %s" % missing


def test_ledger_rows_are_well_formed(inst):
    for k, a in sorted(inst):
        row = V.ledger_row(k, a)
        what = "%s<%s>" % (k, ", ".join(a))
        assert row["status"] in ("default", "forced", "never"), what
        if row["status"] == "never":
            assert row.get("why"), what
        elif row["status"] == "forced":
            assert row.get("why") and _test_exists(row["test"]), what
        elif "test" in row:
            assert _test_exists(row["test"]), what
        else:
            assert "shape" in row or "via" in row, what
        if "rows" in row:  # the variant's row pipeline on its own (tests/test_gpu_rows.py)
            assert _test_exists(row["rows"]), what
        if "pinned" in row:  # a racy default row names the test that reaches the variant in every run
            assert row.get("racy") and _test_exists(row["pinned"]), what
    for name, row in V.FEATURES.items():
        assert "shape" in row if row["status"] == "default" else _test_exists(row["test"]), name


def test_ledger_has_no_stale_rows(inst):
    """a row for a variant that is no longer compiled is a claim about nothing"""
    keys = {(k, a) for k, a in inst}
    rows = set()
    for key in V.SOLVE:
        wb, nt, wv, g, al = key
        args = (str(wb), str(nt), str(wv), str(g)) + (("true" if al else "false"),)
        rows.add(("nrq_solve_kernel", args))
    rows |= {("nrq_backsub_kernel", (str(s),)) for s in V.BACKSUB}
    rows |= {("nrq_plan_kernel", (str(n), str(c))) for n, c in V.PLAN}
    for kernel, table in (("nrq_emit_kernel", V.EMIT), ("nrq_emit_held_kernel", V.EMIT_HELD), ("nrq_emit_set_kernel", V.EMIT_SET)):
        rows |= {(kernel, (str(m), "true" if flag else "false")) for m, flag in table}
    assert len(V.EMIT) == 8 and len(V.EMIT_HELD) == 8 and len(V.EMIT_SET) == 10
    assert rows <= keys, sorted(rows - keys)


def test_every_back_substitution_form_names_its_test():
    """BACKSUB_FORMS: every row's test exists, and the rows are exactly what the GPU case table (tests/forced_inact_support.py) runs"""
    import forced_inact_support as F
    for key, row in V.BACKSUB_FORMS.items():
        assert _test_exists(row["test"]), key
    ran = {}
    for form, u, _, _, strip, threads, sb in F.GPU_CASES:
        w = F.wpr_of(u)
        cls = F.nw_class(w) if not sb else "split<%d>x%d" % (sb, (w + 19) // 20)
        ran.setdefault((strip, threads, cls), set()).add((F.FORMS[form]["K"], u))
    assert {k: set(r["at"]) for k, r in V.BACKSUB_FORMS.items()} == ran
