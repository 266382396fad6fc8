"""-m gpu tier: every form of the solve kernel's back-substitution at a CHOSEN number of inactive columns.

ph_backsub (solve_body.h) picks its code by the plan's W-row width wpr = ceil(u / 32): backsub_fixed<NW> for wpr <= 4 / 8 / 12 / 24
and a plain loop beyond, each as a FAST form (the full-size workgroup) and a register-lean one (256 and 64 threads), and for 16-,
12- and 8-byte strips with a body of backsub_one that exists on the device only (packed nibbles, a byte-select add per table
address, the table's offset in the instruction's immediate, nrq_xor3) -- the CPU emulation runs the generic lines under it, so for
those bodies a decode on the GPU is the only check, and u used to be whatever the planner happened to produce.  Here the context
option "plan_force_inact" (host plans with n columns more inactive from the start: same system, same solution) puts u where a
class begins or ends: per boundary b | b + 1 words u = 32 b - 1, 32 b, 32 b + 1 (u % 32 = 31, 0, 1; u % 4 != 0 twice: ph_tables'
`x < u`), which is also where `if (w >= wpr) break` leaves an unrolled class early or not at all.

A case (tests/forced_inact_support.py GPU_CASES: form, u, the n found for the encode plan and for the decode plan, and what the
launch must be) is three calls of two blocks on the forced context with the host planner: an encode with intermediate symbols, a
decode without them (host plans have no needed-pivot view: the job carries the W' image of its lists, out_lists.h build_out_w, and
back-substitutes nothing -- tests/test_gpu_out_view.py asserts that on these plans) and one with them (every pivot), at T = 48 (three whole 16-byte strips) and T = 40
(a partial last strip) dealt over the three.  Every call is compared with the oracle byte for byte -- repair and intermediate
symbols; verdict, recovered block, intermediate symbols -- and asserts from the call stats that it ran where the row says:
strip_bytes, wg_threads, backsub_strip, u, and that every block was planned on the host (stats "planner" == 0, "encplan_device" ==
0; "host_planned" counts the device planner's capacity fallbacks only and stays 0).  GF arithmetic: no tolerance.

Reached, (strip bytes, threads): classes (0 = the plain loop):
  (16, 768): 8, 12, 24, 0 at K = 5200 (u 255 .. 769); 24, 0 also at K = 1000 (all 1071 columns inactive) and K = 3000
  (16, 256): 4, 8, 12, and 24 at its lower edge (13 words, K = 1000)
  (16, 64):  4 (K = 100: u 31 .. 128, npiv 97 .. 0, across npiv = 65, 64, 63 against the workgroup of 64)
  (12, 768): 8, 12, 24 at 13 words (K = 10000); 24 | 0 (K = 5200); 0 at 40 and 41 words (K = 3000)
  (8, 768):  8 | 12 (K = 10000); 12, 24, 0 (K = 15000)
  (8, 256):  12, 24, 0 up to 34 words; (8, 64): 4, 8, 12 at 9 words (K = 1000)
  split solve, 4- and 2-byte strips (K = 3000): nrq_backsub_kernel<32> at 20 words, <16> at 21, 40 and 41; 4-byte strips on the
  full-size workgroup with <16> at 40 and 41 words (K = 15000)
Not reachable on any context (tests/test_forced_inact_emu.py holds the table against solve_shape):
  (16, 256) beyond 13 words: the 256-thread workgroup is taken while two images fit the LDS; at 24 words the tables alone are
  48 KiB and the slots of the u >= 737 columns and their scratch rows 23 KiB more: the image passes 80 KiB at any K
  (16, 64) beyond 4 words at K = 100 (L = 128); single waves need seven images per CU (23 KiB)
  (12, 256) and (12, 64): 12-byte strips are compiled for the full-size workgroup only
More than 1280 inactive columns (the device planner's capacity; the host planner has none): 1281 run here on 12-, 4- and 2-byte
strips.  A plan whose split-solve tables exceed the LDS (98 words at K = 3000) is refused with a status before any launch.

After a HIP error every later test of the file skips: nothing more is started on a device that has just faulted."""
import numpy as np
import pytest

import nanorq_amd
import forced_inact_support as F
from util import received_set

pytestmark = pytest.mark.gpu

_BROKEN = []   # the case whose call returned an error from the HIP runtime: no further launch


@pytest.fixture(scope="module")
def G():
    import gpu_support
    gpu_support.ctx()
    return gpu_support


_REF = {}


def _reference(orc, K):
    """per block size, once: the blocks at T = 48, the reception, and from the oracle the repair symbols, the intermediate symbols
    and the decode's verdict and rows"""
    if K not in _REF:
        lost, esis, _, _ = F.gpu_reception(orc, K)
        src = F.gpu_source(K, 48)
        rep, inter = [], []
        for b in range(F.NBLK):
            r, i, _ = orc.encode_block(src[b], K, 48, esis, want_inter=True)
            rx = received_set(K, lost, len(esis) - len(lost))
            ok, out, _ = orc.decode_block(rx, np.concatenate([src[b][rx[rx < K]], r]), K, 48)
            assert ok and np.array_equal(out, src[b])
            rep.append(r)
            inter.append(i)
        _REF[K] = (lost, esis, src, np.stack(rep), np.stack(inter))
    return _REF[K]


class _forced_plans:
    """the forced context with the host planner, the form's options and n columns forced inactive; everything back in place on exit"""

    def __init__(self, G, opts):
        self.c, self.opts = G.ctx(), opts

    def __enter__(self):
        self.c.set_planner(False)
        for k, v in self.opts.items():
            self.c.set_option(k, v)
        return self

    def force(self, n):
        self.c.set_option("plan_force_inact", n)
        self.c.clear_plan_cache()   # (an encode plan is kept per K': the next encode builds it again, at this n)

    def __exit__(self, *a):
        self.c.set_option("plan_force_inact", 0)
        self.c.set_option("max_wb", 16)
        self.c.set_planner(True)
        self.c.clear_plan_cache()


def _ran_where_it_claims(s, strip, threads, sb, u, what):
    assert (s["strip_bytes"], s["wg_threads"], s["backsub_strip"], s["u"]) == (strip, threads, sb, u), (what, s)
    assert s["strip_bytes_b"] == 0 and s["host_planned"] == 0, (what, s)


@pytest.mark.parametrize("index", range(len(F.GPU_CASES)), ids=["%s-u%d" % (c[0], c[1]) for c in F.GPU_CASES])
def test_backsub_form(G, orc, index):
    if _BROKEN:
        pytest.skip("a call of case %s returned a HIP error: no further launches" % (_BROKEN[0],))
    form, u, n_enc, n_dec, strip, threads, sb = F.GPU_CASES[index]
    K = F.FORMS[form]["K"]
    lost, esis, src, rep, inter = _reference(orc, K)
    try:
        with _forced_plans(G, F.FORMS[form]["opts"]) as fp:
            for kind, T, want_inter in F.calls_of(index):
                what = (form, u, kind, T, want_inter)
                if kind == "encode":
                    fp.force(n_enc)
                    got_rep, got_inter = G.gpu_encode(np.ascontiguousarray(src[:, :, :T]), K, T, esis[:F.NREP], want_inter=True)
                    s = fp.c.stats()
                    _ran_where_it_claims(s, strip, threads, sb, u, what)
                    assert s["encplan_device"] == 0, (what, s)
                    assert np.array_equal(got_inter, inter[:, :, :T]), (what, "intermediate symbols")
                    assert np.array_equal(got_rep, rep[:, :F.NREP, :T]), (what, "repair symbols")
                else:
                    fp.force(n_dec)
                    work = np.ascontiguousarray(src[:, :, :T]).copy()
                    work[:, lost] = 0x3C
                    st, out, got_inter = G.gpu_decode(work, K, T, [lost] * F.NBLK, [esis] * F.NBLK,
                                                      [np.ascontiguousarray(rep[b][:, :T]) for b in range(F.NBLK)], want_inter=want_inter)
                    s = fp.c.stats()
                    _ran_where_it_claims(s, strip, threads, sb, u, what)
                    assert s["planner"] == 0 and s["plan_wg_threads"] == 0, (what, s)   # every block planned on the host
                    assert list(st) == [1] * F.NBLK, (what, "verdict", st)
                    assert np.array_equal(out, src[:, :, :T]), (what, "recovered block")
                    if want_inter:
                        assert np.array_equal(got_inter, inter[:, :, :T]), (what, "intermediate symbols of the decode")
    except nanorq_amd.NrqError:
        _BROKEN.append((form, u))
        raise


def test_tables_beyond_the_lds_are_refused_before_any_launch(G, orc):
    """K = 3000 with every column inactive (98 W words) on 4-byte strips: the split solve's tables would take 196 KiB.  The call
    fails with the library's status for it and the context goes on working.  (That the refusal comes before the solve kernel's
    launch: tests/test_host_model.py, on the model runtime's launch log.)"""
    if _BROKEN:
        pytest.skip("a call of case %s returned a HIP error: no further launches" % (_BROKEN[0],))
    K, T = 3000, 48
    lost, esis, src, rep, inter = _reference(orc, K)
    work = src.copy()
    work[:, lost] = 0x3C
    with _forced_plans(G, {"max_wb": 4}) as fp:
        fp.force(nanorq_amd.params(K)["W"])
        with pytest.raises(nanorq_amd.NrqError, match="back-substitution tables do not fit the LDS"):
            G.gpu_decode(work, K, T, [lost] * F.NBLK, [esis] * F.NBLK, list(rep))
        fp.c.sync()
    st, out, _ = G.gpu_decode(work, K, T, [lost] * F.NBLK, [esis] * F.NBLK, list(rep))
    assert list(st) == [1] * F.NBLK and np.array_equal(out, src)
