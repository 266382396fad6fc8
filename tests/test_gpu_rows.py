"""The row pipelines of solve_body.h on the device against a plain replay of their op stream.

fwd_rows (and its half / third / two-thirds forms), rev_rows and fwd_rows_wide exist on the device only.  tests/gpu/rows_probe.hip
runs every form the kernels instantiate, one workgroup per case, and hands the whole LDS back; each test here is one launch whose
grid is the instance's case table (tests/rows_support.py: every nrows at an edge of the form's loop x random fill, full rows,
chains at the minimum distance, 64 lanes on one target, the full image's extremes, thin wide rows).  The comparison is the whole
LDS, byte for byte: the slots the ops name, the slots they do not, the 64 scratch slots (zero before and after) and the pattern
behind the image.  GF(2) arithmetic: there is no tolerance.

If a launch returns a HIP error the test fails and every later test of the file skips: nothing more is started on a device that
has just faulted.
"""
import time

import numpy as np
import pytest

import rows_support as R

pytestmark = pytest.mark.gpu

_BROKEN = []  # (instance, HIP status) of a probe call that failed: no further launch


def _launch_allowed():
    if _BROKEN:
        pytest.skip("the probe returned HIP status %d on %s: no further launches" % (_BROKEN[0][1], _BROKEN[0][0]))


def _where(case, width, a, b):
    """the parts of the LDS in which a and b differ, and the first byte that does"""
    diff = np.flatnonzero(a != b)
    named = np.unique(np.concatenate([case.dst.ravel(), case.src.ravel()]))
    named = set(named[named >= R.SCRATCH].tolist())
    parts = set()
    for i in diff[:4096]:
        idx = int(i) // width
        parts.add("scratch" if idx < R.SCRATCH else "behind the image" if idx >= case.nslots else "named slots" if idx in named else "unnamed slots")
    i = int(diff[0])
    return "%s: %d bytes differ in %s; first at byte %d (index %d + %d): got %#04x, want %#04x" % (
        case.name, diff.size, sorted(parts), i, i // width, i % width, int(a[i]), int(b[i]))


def _id(name):
    return name.replace("<", "-").replace(">", "").replace(",", "-")


@pytest.mark.parametrize("name", sorted(R.INSTANCES), ids=_id)
def test_rows(name):
    """one instance, one launch: the LDS after the pipeline is the LDS before it with the replayed image in front"""
    _launch_allowed()
    family, ring, width = R.INSTANCES[name]
    cases = R.instance_cases(name)
    t0 = time.time()
    status, lds_in, lds_out = R.run_instance(name, cases)
    t1 = time.time()
    if status != 0:
        _BROKEN.append((name, status))
        pytest.fail("%s: the probe returned status %d" % (name, status))
    bad = []
    for k, c in enumerate(cases):
        want = lds_in[k].copy()
        want[:c.nslots * width] = R.reference(name, c).ravel()
        assert not want[:R.SCRATCH * width].any()
        if not np.array_equal(lds_out[k], want):
            bad.append(_where(c, width, lds_out[k], want))
    print("%s: %d cases, probe call %.2f s, references %.2f s" % (name, len(cases), t1 - t0, time.time() - t1))
    assert not bad, "%d of %d cases differ:\n%s" % (len(bad), len(cases), "\n".join(bad[:12]))


def test_address_helpers():
    """row_addr_hi / row_addr_lo (the SDWA shift, the 24-bit multiply of the 12-byte strip) for every 16-bit field value in op words
    that hold it in both halves, the low one and the high one; t4_addr for the four bytes of 4096 words"""
    _launch_allowed()
    rng = np.random.default_rng(20)
    n = 4096
    x = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    x[:8] = (0, 0xFFFFFFFF, 0x80808080, 0x7F7F7F7F, 0x000000FF, 0x0000FF00, 0x00FF0000, 0xFF000000)
    base = rng.integers(0, R.LDS_MAX, n, dtype=np.uint64).astype(np.uint32)
    base[:2] = (0, 0xFFFFFF00)
    hl = np.full((3, 65536, 5, 2), 0xEEEEEEEE, np.uint32)
    t4 = np.full((n, 4), 0xEEEEEEEE, np.uint32)
    status = R.probe().rows_probe_addr(hl.ctypes.data, base.ctypes.data, x.ctypes.data, n, t4.ctypes.data)
    if status != 0:
        _BROKEN.append(("the address helpers", status))
        pytest.fail("the probe returned status %d" % status)
    v = np.arange(65536, dtype=np.uint32)
    ops = np.stack([v | v << 16, v, v << 16])
    for w, wb in enumerate((16, 12, 8, 4, 2)):
        assert np.array_equal(hl[:, :, w, 0], (ops >> 16) * wb), "row_addr_hi<%d>" % wb
        assert np.array_equal(hl[:, :, w, 1], (ops & 0xFFFF) * wb), "row_addr_lo<%d>" % wb
    for byte in range(4):
        assert np.array_equal(t4[:, byte], base + ((x >> (8 * byte)) & 0xFF)), "t4_addr byte %d" % byte
