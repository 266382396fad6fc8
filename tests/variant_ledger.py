"""The ledger of compiled kernel variants: one row per instantiation in libnanorq_hip.so, saying how the suite pins it.

Plain data, no GPU imports: tests/test_variant_ledger.py (CPU) checks that every instantiation `nm -C` lists has a row, and
tests/test_gpu_variants.py (GPU) runs every "default" row at its shape on a context with no option set, asserts from the call
stats that the launch took that variant and compares the results with the oracle byte for byte.

A row is one of
  status "default": `shape` reaches the variant with default options (stats observed on an MI355X, 256 CUs);
  status "forced":  no default-option shape reaches it; `test` names the test that selects it through an option, `why` says
                    why the defaults cannot reach it;
  status "never":   no launch path selects it at all (dead code); `why` says why.
"""

# nrq_solve_kernel<WB, NT, WV, G, AL>: strip bytes, threads, waves per SIMD (compiled register budget), lanes per element
# (wide strips), movers without byte-wise paths.  Stats: strip_bytes = WB * G, wg_threads, wg_waves_per_simd, movers_aligned.
# A shape: K source symbols, T bytes, nblk blocks, decode loss rate; Kp: the K' row when it is not K's own.

_NARROW_SMALL = ("a narrower width is taken only when the next wider image exceeds the LDS, and the image shrinks by at most the "
                 "ratio of the widths (12 -> 8: 2/3, 8 -> 4, 4 -> 2: 1/2) plus a fixed part, so it still needs more than half the "
                 "LDS: the full-size workgroup")
_NARROW_TEST = "tests/test_gpu_parity.py::test_narrow_strip_paths_at_small_sizes"

# rows: the variant's row pipeline (fwd_rows_wide<G>) also runs on its own, against a plain replay of its op stream, whatever the
# launch options: the test's case [fwd_rows_wide-G]
_ROWS_TEST = "tests/test_gpu_rows.py::test_rows"

SOLVE = {
    # 16-byte strips, full-size workgroup
    (16, 768, 1, 1, True): dict(status="default", shape=dict(K=1500, T=1280, nblk=1, loss=0.2),
                                note="lone: a single block's 80 strips each get a CU (the reference's benchmark.c shape)"),
    (16, 768, 1, 1, False): dict(status="default", shape=dict(K=8192, T=1288, nblk=16, loss=0.1),
                                 note="full 16-byte image, T not a multiple of 16: general movers"),
    # 16-byte strips, 256-thread workgroups
    (16, 256, 4, 1, True): dict(status="default", shape=dict(K=3000, T=1280, nblk=8, loss=0.2)),
    (16, 256, 4, 1, False): dict(status="default", shape=dict(K=3000, T=1288, nblk=8, loss=0.2)),
    # (the five-per-CU build: a product context keeps the option small_waves4 set, so K=1000 T=64 x 4 blocks -- the candidate
    # shape -- runs 256/4; measured on an MI355X)
    (16, 256, 5, 1, True): dict(status="forced", test="tests/test_gpu_parity.py::test_five_workgroups_per_cu_variant",
                                why="only with the option small_waves4 cleared (default: set)"),
    (16, 256, 5, 1, False): dict(status="forced", test="tests/test_gpu_parity.py::test_five_workgroups_per_cu_variant",
                                 why="only with the option small_waves4 cleared (default: set)"),
    # 16-byte strips, single-wave workgroups
    (16, 64, 3, 1, True): dict(status="default", shape=dict(K=100, T=1024, nblk=64, loss=0.2)),
    # (64 blocks of T=100 are 448 strips, not more than 2 per CU: 256/4 on an MI355X; 128 blocks are 896)
    (16, 64, 3, 1, False): dict(status="default", shape=dict(K=100, T=100, nblk=128, loss=0.2)),
    # wide strips: never selected automatically (solve_shape: "wide_g" only)
    (16, 256, 4, 2, False): dict(status="forced", test="tests/test_gpu_parity.py::test_wide_strips", rows=_ROWS_TEST,
                                 why="wide strips are an experiment: only the option wide_g selects them"),
    (16, 256, 4, 4, False): dict(status="forced", test="tests/test_gpu_parity.py::test_wide_strips", rows=_ROWS_TEST,
                                 why="wide strips are an experiment: only the option wide_g selects them"),
    (16, 256, 4, 8, False): dict(status="forced", test="tests/test_gpu_parity.py::test_wide_strips", rows=_ROWS_TEST,
                                 why="wide strips are an experiment: only the option wide_g selects them"),
    # 12-byte strips (compiled for the full-size workgroup only)
    (12, 768, 1, 1, True): dict(status="default", shape=dict(K=10000, T=1280, nblk=2, loss=0.1)),
    (12, 768, 1, 1, False): dict(status="default", shape=dict(K=10000, T=40, nblk=2, loss=0.1)),
    # 8-byte strips
    (8, 768, 1, 1, True): dict(status="default", shape=dict(K=15000, T=16, nblk=2, loss=0.1)),
    (8, 768, 1, 1, False): dict(status="default", shape=dict(K=15000, T=24, nblk=2, loss=0.1)),
    # 4-byte strips: the solve stops after the dense stage, nrq_backsub_kernel finishes
    (4, 768, 1, 1, True): dict(status="default", shape=dict(K=27000, T=64, nblk=1, loss=0.1), backsub=32),
    (4, 768, 1, 1, False): dict(status="default", shape=dict(K=27000, T=72, nblk=1, loss=0.1), backsub=32),
    # 2-byte strips
    (2, 768, 1, 1, False): dict(status="default", shape=dict(K=56403, T=16, nblk=1, loss=0.1), backsub=32),
    (2, 768, 1, 1, True): dict(status="never", why="solve_shape allows the aligned movers only for WB >= 4"),
    (2, 256, 4, 1, True): dict(status="never", why="solve_shape allows the aligned movers only for WB >= 4"),
    (2, 256, 5, 1, True): dict(status="never", why="solve_shape allows the aligned movers only for WB >= 4"),
    (2, 64, 3, 1, True): dict(status="never", why="solve_shape allows the aligned movers only for WB >= 4"),
}
for _wb in (8, 4, 2):
    for _nt, _wv in ((256, 4), (256, 5), (64, 3)):
        for _al in (True, False):
            SOLVE.setdefault((_wb, _nt, _wv, 1, _al), dict(status="forced", test=_NARROW_TEST, why=_NARROW_SMALL))

# nrq_backsub_kernel<SB>: the second half of a narrow-strip (WB <= 4) solve; stats backsub_strip
BACKSUB = {
    32: dict(status="default", via=(4, 768, 1, 1, True)),
    # W rows of more than 20 words (u > 640 inactive columns).  Reached with default options at K'=56403, but not at a fixed
    # shape: the device planner's inactivation count depends on which wave claims a column first, and one reception (10 % loss,
    # overhead 2, loss pattern seed 3) gave u = 631 in one run and 671 in another on an MI355X.  racy: the test runs the shape and
    # compares with the oracle whichever strip it took; seeing 16 is not required.
    # pinned: the test that reaches the instance in EVERY run -- one block of K'=56403 whose plan comes from the HOST planner
    # (set_planner(False): the same plan each time, u = 655, 21 W words per row), so 2-byte strips, nrq_backsub_kernel<16> with its
    # loop over a second batch of W words, and the collect, at T = 16 and 40, with and without intermediate symbols, against the
    # oracle.  It does not cover the default launch path (device planner, no option set): that stays with the racy shape.
    16: dict(status="default", racy=True, shape=dict(K=56403, T=16, nblk=1, loss=0.1, oh=2, seed=3),
             pinned="tests/test_gpu_split.py::test_backsub16_second_word_batch"),
}

# The forms of the back-substitution INSIDE an instance: ph_backsub (solve_body.h) takes backsub_fixed<NW> for plans of at most 4 / 8 /
# 12 / 24 W words per row (wpr = ceil(u / 32), u the plan's inactive columns) and a plain loop beyond (class 0 here), in a fast form
# on 768 threads and a lean one on 256 and 64, with device-only bodies for 16-, 12- and 8-byte strips; the split solve's
# nrq_backsub_kernel<SB> asks for a pivot's W words in batches of 20 ("split<SB>xN": N batches).  One row per (strip bytes,
# threads, class) that a context can reach, the test that runs it on plans at a forced u (the option plan_force_inact) and the
# (K, u) it runs it at -- tests/forced_inact_support.py GPU_CASES is the table behind this one, tests/test_variant_ledger.py holds
# the two against each other.  What no context reaches, and why: the docstring of the test's module.
_FORMS_TEST = "tests/test_gpu_backsub_forms.py::test_backsub_form"
BACKSUB_FORMS = {
    (16, 768, 8): dict(test=_FORMS_TEST, at=[(5200, 255), (5200, 256)]),
    (16, 768, 12): dict(test=_FORMS_TEST, at=[(3000, 383), (3000, 384), (5200, 257), (5200, 383), (5200, 384)]),
    (16, 768, 24): dict(test=_FORMS_TEST, at=[(1000, 767), (1000, 768), (3000, 385), (3000, 767), (3000, 768), (5200, 385), (5200, 767), (5200, 768)]),
    (16, 768, 0): dict(test=_FORMS_TEST, at=[(1000, 769), (1000, 1071), (3000, 769), (5200, 769)]),
    (16, 256, 4): dict(test=_FORMS_TEST, at=[(1000, 127), (1000, 128), (3000, 127), (3000, 128)]),
    (16, 256, 8): dict(test=_FORMS_TEST, at=[(1000, 129), (1000, 255), (1000, 256), (3000, 129), (3000, 255), (3000, 256)]),
    (16, 256, 12): dict(test=_FORMS_TEST, at=[(1000, 257), (1000, 383), (1000, 384), (3000, 257)]),
    (16, 256, 24): dict(test=_FORMS_TEST, at=[(1000, 385)]),
    (16, 64, 4): dict(test=_FORMS_TEST, at=[(100, 31), (100, 32), (100, 33), (100, 63), (100, 64), (100, 65), (100, 95), (100, 96), (100, 97), (100, 127), (100, 128)]),
    (12, 768, 8): dict(test=_FORMS_TEST, at=[(10000, 255), (10000, 256)]),
    (12, 768, 12): dict(test=_FORMS_TEST, at=[(10000, 257), (10000, 383), (10000, 384)]),
    (12, 768, 24): dict(test=_FORMS_TEST, at=[(5200, 767), (5200, 768), (10000, 385)]),
    (12, 768, 0): dict(test=_FORMS_TEST, at=[(3000, 1279), (3000, 1280), (3000, 1281), (5200, 769)]),
    (8, 768, 8): dict(test=_FORMS_TEST, at=[(10000, 255), (10000, 256)]),
    (8, 768, 12): dict(test=_FORMS_TEST, at=[(10000, 257), (15000, 383), (15000, 384)]),
    (8, 768, 24): dict(test=_FORMS_TEST, at=[(15000, 385), (15000, 767), (15000, 768)]),
    (8, 768, 0): dict(test=_FORMS_TEST, at=[(15000, 769)]),
    (8, 256, 12): dict(test=_FORMS_TEST, at=[(1000, 383), (1000, 384)]),
    (8, 256, 24): dict(test=_FORMS_TEST, at=[(1000, 385), (1000, 767), (1000, 768)]),
    (8, 256, 0): dict(test=_FORMS_TEST, at=[(1000, 769), (1000, 1071)]),
    (8, 64, 4): dict(test=_FORMS_TEST, at=[(1000, 127), (1000, 128)]),
    (8, 64, 8): dict(test=_FORMS_TEST, at=[(1000, 129), (1000, 255), (1000, 256)]),
    (8, 64, 12): dict(test=_FORMS_TEST, at=[(1000, 257)]),
    (4, 768, 'split<16>x2'): dict(test=_FORMS_TEST, at=[(15000, 1280)]),
    (4, 768, 'split<16>x3'): dict(test=_FORMS_TEST, at=[(15000, 1281)]),
    (4, 256, 'split<16>x2'): dict(test=_FORMS_TEST, at=[(3000, 641), (3000, 1279), (3000, 1280)]),
    (4, 256, 'split<16>x3'): dict(test=_FORMS_TEST, at=[(3000, 1281)]),
    (4, 256, 'split<32>x1'): dict(test=_FORMS_TEST, at=[(3000, 639), (3000, 640)]),
    (2, 64, 'split<16>x2'): dict(test=_FORMS_TEST, at=[(3000, 641), (3000, 1279), (3000, 1280)]),
    (2, 64, 'split<16>x3'): dict(test=_FORMS_TEST, at=[(3000, 1281)]),
    (2, 64, 'split<32>x1'): dict(test=_FORMS_TEST, at=[(3000, 639), (3000, 640)]),
}

# nrq_plan_kernel<NT, compact>: the decode planner; stats plan_wg_threads, plan_compact_state (and plan_segmented)
PLAN = {
    (1024, 0): dict(status="default", shape=dict(K=1000, T=16, nblk=64, loss=0.2),
                    note="a batch of at most one block per CU: the 1024-thread workgroup"),
    (1024, 1): dict(status="default", shape=dict(K=27000, T=16, nblk=1, loss=0.1),
                    note="the peeling state does not fit the LDS: the compact form"),
    (256, 0): dict(status="default", shape=dict(K=2000, T=16, nblk=1024, loss=0.2)),
    (128, 0): dict(status="default", shape=dict(K=100, T=16, nblk=1024, loss=0.2)),
}

# what a call can do besides the kernel instance: the host planner for small calls, the segmented planner run, encode plans
# built by the planner kernel, a batch split into two block lists
FEATURES = {
    "host_small": dict(status="default", shape=dict(K=100, T=64, nblk=1, loss=0.2),
                       note="one small block: nrq_decode_blocks_lazy plans it on the host (plan_wg_threads 0)"),
    "plan_segmented": dict(status="default", shape=dict(K=56403, T=16, nblk=1, loss=0.1)),
    "encplan_device": dict(status="default", shape=dict(K=15000, T=16, nblk=2, loss=0.1),
                           note="L >= 12000 (encplan_dev_min_l)"),
    "two_block_lists": dict(status="forced", test="tests/test_gpu_parity.py::test_block_lists_per_launch",
                            why="one block in a few thousand at K=8192 needs the second list; the test forces it with lds_max"),
    # the planner's lists in row order, offsets from the prefix scan (planner_body.h pl_final_c2; stats plan_scan_lists): more than
    # 2 * qcap missing symbols.  The 256-thread instances (qcap 512 / 1024) at three blocks by plan_pack; the same test file reaches
    # them, and the 1024-thread one, with default options too (260 blocks of K = 1300; K = 4200 all missing)
    "plan_scan_lists": dict(status="forced", test="tests/test_gpu_high_loss.py::test_edge_of_the_scan_form",
                            why="75-100 % loss of a block AND more blocks than compute units (or plan_pack) for the 256-thread planner"),
}

# the emit kernel nrq_emit_kernel<MODE, MULTI> (one-segment and multi-segment tables) and the object layout kernel: each
# instance and a test that launches it
TX_MODES = {0: "TX_V16", 1: "TX_V16_SHIFT", 2: "TX_DWORD", 3: "TX_BYTE"}
_TX_TEST = "tests/test_gpu_tx.py::test_device_emit_matches_emulation"
EMIT = {
    (0, False): dict(status="default", test=_TX_TEST, why="16-byte rows, tags in a list"),
    (1, False): dict(status="default", test=_TX_TEST, why="16-byte rows, inline header"),
    (2, False): dict(status="default", test=_TX_TEST, why="stride a multiple of 4"),
    (3, False): dict(status="default", test=_TX_TEST, why="T odd / odd stride"),
}
EMIT.update({(m, True): dict(status="default", test="tests/test_gpu_variants.py::test_object_emit_modes",
                             why=TX_MODES[m] + ", an object of three segments") for m in TX_MODES})
# the held emit nrq_emit_held_kernel<MODE, MULTI> (a relay's tag-list emit with NRQ_TX_HELD: one reception, or an object's table of
# several segments) and the set emit nrq_emit_set_kernel<MODE, HELD> (MODE 4: the 16-byte form under key + FEC Payload ID)
_HELD_PARTIAL = "tests/test_gpu_held.py::test_partial_blocks"
EMIT_HELD = {
    (0, False): dict(status="default", test=_HELD_PARTIAL, why="T = 1280, tags in a list"),
    (1, False): dict(status="default", test="tests/test_gpu_held.py::test_second_round_of_the_shifted_form_matches_emulation",
                     why="T = 1040 behind the inline header, a 16-byte stride"),
    (2, False): dict(status="default", test=_HELD_PARTIAL, why="a packet stride of T + 4"),
    (3, False): dict(status="default", test=_HELD_PARTIAL, why="an odd packet stride"),
}
EMIT_HELD.update({(m, True): dict(status="default", test="tests/test_gpu_held.py::test_object_held_emit_modes",
                                  why=TX_MODES[m] + ", an object relay's table of two block classes") for m in TX_MODES})
TXS_MODES = dict(TX_MODES)
TXS_MODES[4] = "TXS_V16_KEY"
EMIT_SET = {(m, False): dict(status="default", test="tests/test_gpu_txset.py::test_device_matches_emulation_at_wave_edges",
                             why=TXS_MODES[m] + ": below one round of the wave, exactly one round, a later round") for m in TXS_MODES}
EMIT_SET.update({(m, True): dict(status="default", test="tests/test_gpu_txset.py::test_held_device_matches_emulation",
                                 why=TXS_MODES[m] + " over relays with NRQ_TX_HELD: one round and a second round") for m in TXS_MODES})
OBJ_LAYOUT = {
    16: dict(status="default", test="tests/test_gpu_obj.py::test_receiver_matches_host_decoder", why="T = 64, N = 1"),
    8: dict(status="default", test="tests/test_gpu_obj.py::test_receiver_matches_host_decoder", why="T = 1280, N = 3, Al = 8"),
    4: dict(status="default", test="tests/test_gpu_obj.py::test_receiver_matches_host_decoder", why="T = 52, N = 2, Al = 4"),
    2: dict(status="default", test="tests/test_gpu_variants.py::test_object_layout_widths", why="T = 28, N = 2, Al = 2"),
    1: dict(status="default", test="tests/test_gpu_obj.py::test_receiver_matches_host_decoder", why="T = 13, N = 2, Al = 1"),
}
OBJ_WORD = {"tx_u128": 16, "unsigned long": 8, "unsigned int": 4, "unsigned short": 2, "unsigned char": 1}


def ledger_row(kernel, args):
    """the row of one instantiation as `nm -C` prints it: kernel name and its template argument list (strings)"""
    if kernel == "nrq_solve_kernel":
        wb, nt, wv, g = (int(a) for a in args[:4])
        al = len(args) > 4 and args[4] == "true"
        return SOLVE.get((wb, nt, wv, g, al))
    if kernel == "nrq_backsub_kernel":
        return BACKSUB.get(int(args[0]))
    if kernel == "nrq_plan_kernel":
        return PLAN.get((int(args[0]), int(args[1]) if len(args) > 1 else 0))
    if kernel == "nrq_emit_kernel":
        return EMIT.get((int(args[0]), args[1] == "true"))
    if kernel == "nrq_emit_held_kernel":
        return EMIT_HELD.get((int(args[0]), args[1] == "true"))
    if kernel == "nrq_emit_set_kernel":
        return EMIT_SET.get((int(args[0]), args[1] == "true"))
    if kernel == "nrq_obj_layout_kernel":
        return OBJ_LAYOUT.get(OBJ_WORD.get(args[0]))
    raise KeyError(kernel)


KERNELS = ("nrq_solve_kernel", "nrq_backsub_kernel", "nrq_plan_kernel", "nrq_emit_kernel", "nrq_emit_held_kernel", "nrq_emit_set_kernel",
           "nrq_obj_layout_kernel")
