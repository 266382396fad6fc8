"""CPU tier: the library's HOST layer -- the host code of nrq_device.hip, planner_host.cpp, nanorq_api.c, io.c, compiled from the
same sources into tests/emu/libnanorq_model.so -- on a MODEL of the HIP runtime (tests/emu/hip_model.h): seven streams and about
twenty events per context, double- and triple-buffered arenas, the caching device pool, the object layer's error paths under
`fail_after`.  The model orders the operations as the runtime would (streams, events, synchronisations) and keeps every
allocation's lifetime; it reports
    H1  two operations on one allocation, one of them a write, that nothing orders,
    H2  a range outside every live allocation,
    H3  a host allocation released under a pending operation,
    H4  a page-locked upload source changed before the host synchronised behind the copy.
Kernels do not run (hip_model.h lists the assumptions); what the GPU tier cannot see -- an ordering that only holds by luck -- is
what these tests are about, what only kernels compute is not.  Each group runs once, in a child process (host_model_worker.py).
Group g runs the host layer with its context on a stream of the caller's own, where a call the library puts on stream 0 shows."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_RUNS = {}


def run(group):
    if group not in _RUNS:
        from nanorq_amd import build
        build.build_model_lib()
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "host_model_worker.py"), group], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=600)
        text = r.stdout.decode(errors="replace")
        lines = [x for x in text.splitlines() if x.startswith("RESULT ")]
        assert r.returncode == 0 and lines, "worker %s: exit status %d\n%s" % (group, r.returncode, text[-3000:])
        _RUNS[group] = json.loads(lines[-1][7:])
    return _RUNS[group]


# ------------------------------------------------------------------------------------------------ a. the detector ----
DETECTOR = [   # scenario, exactly these hazards
    ("ww_unordered", ["H1"]), ("ww_disjoint", []), ("ww_record_wait", []), ("ww_host_sync", []), ("ww_recorded_too_early", ["H1"]),
    ("wait_never_recorded", ["H1"]), ("rr_unordered", []), ("rw_unordered", ["H1"]),
    ("pinned_source_rewritten_early", ["H4"]), ("pinned_source_rewritten_after_sync", []),
    ("download_read_early", []), ("download_pageable", []),
    ("memset_one_past", ["H2"]), ("copy_one_past", ["H2"]), ("copy_to_the_last_byte", []), ("use_after_free", ["H2"]),
    ("host_free_under_pending_copy", ["H3"]), ("host_free_after_sync", []), ("unregister_under_pending_download", ["H3"]),
    ("launch_pointer_unordered", ["H1"]), ("launch_const_pointer_beside_a_read", []), ("launch_struct_word_unordered", ["H1"]),
    ("launch_record_word_unordered", ["H1"]), ("launch_record_word_ordered", []),
    ("launch_reads_pageable_memory", ["H2"]), ("launch_reads_page_locked_memory", []),
]


@pytest.mark.parametrize("name,kinds", DETECTOR, ids=[d[0] for d in DETECTOR])
def test_the_detector_reports_exactly_the_hazard_of_a_hand_built_scenario(name, kinds):
    s = run("detector")[name]
    assert s["kinds"] == kinds, s["text"]


def test_the_detector_names_both_operations_their_streams_and_the_allocation():
    d = run("detector")
    t = d["ww_unordered"]["text"][0]
    assert "hipMemsetAsync 8192 B [stream 1" in t and "hipMemsetAsync 8192 B [stream 2" in t and "allocation of 8192 bytes" in t, t
    assert d["wait_never_recorded"]["unrecorded"] == 1
    assert "through the word at +24 of what argument 0 points at" in d["launch_record_word_unordered"]["text"][0]
    assert "released" in d["use_after_free"]["text"][0]
    assert d["pending_at_end"] == 0


def test_a_download_shows_poison_until_the_host_has_synchronised_behind_it():
    d = run("detector")
    assert d["download_read_early"]["early"] == [0xDB, 0xDB] and d["download_read_early"]["late"] == [0x11, 0x11]
    # a copy into pageable memory returns with the bytes, and the host has then waited for the stream
    assert d["download_pageable"]["got"] == [0x11, 0x11] and d["download_pageable"]["pending"] == 0
    # page-locked memory that was unregistered under the copy is never written
    assert d["unregister_under_pending_download"]["untouched"]


# ---------------------------------------------------------------------------------------------------- b. the pool ----
def test_the_pool_reuses_a_block_only_within_its_rule():
    """a cached block serves a request of `want` bytes (rounded up to 4 KiB) iff want <= block <= 1.25 want + 64 KiB"""
    rule = run("pool")["rule"]
    assert [r["expect_reuse"] for r in rule] == [True, True, False, True, False, False]   # both sides of both bounds
    for r in rule:
        assert r["reused"] == r["expect_reuse"], r
        assert r["block_bytes"] >= r["req"], r


def test_the_pool_s_books_after_a_trim():
    t = run("pool")["trim"]
    assert t["before"][0] == 3 and t["before"][1] == 2 and t["before"][2] > 0, t
    assert t["after"] == [1, 0, 0] and t["live_after"] == 1 and t["y_alive"] and not t["x_alive"], t


def test_a_failed_allocation_leaves_the_pool_as_it_was():
    inj = run("pool")["inject"]
    assert [i["failed"] for i in inj] == [True, True, False], inj   # hipSetDevice, hipMalloc; the third call is past the allocation
    for i in inj:
        assert i["books_after"] == i["books_before"] == [0, 0, 0] or not i["failed"], i
        assert i["retry_ok"], i


def test_a_second_free_of_a_block_is_refused():
    """nrq_dev_free used to accept it: the block was then cached twice, handed to two owners, and released twice by a trim"""
    d = run("pool")["double_free"]
    assert d["refused"] and "freed already" in d["msg"], d
    assert d["books_after"] == d["books_before"], d
    assert d["q1_is_p"] and not d["q2_is_p"], d
    assert run("pool")["free_of_an_inner_address_refused"]


def test_no_block_has_two_live_owners_and_destroy_returns_everything():
    p = run("pool")
    assert p["walk"]["overlaps"] == 0 and p["walk"]["short"] == 0, p["walk"]
    assert p["walk"]["books"][0] - p["walk"]["books"][1] == p["walk"]["live"], p["walk"]
    assert p["destroy"]["live_after"] == 0, p["destroy"]     # 46 blocks were still handed out
    assert p["hazards"] == []


# ------------------------------------------------------------------------------------- c. the call that faulted ----
def _fuzz_clean(f):
    for kind in ("forced", "default"):
        r = f[kind]
        assert r["decodes"] == 30 and r["host_planned"] == 30, r     # stats(): every decode was planned on the host
        assert r["bad_downloads"] == [], r["bad_downloads"][:4]      # every download inside a live device block of its size
        assert r["pending_after_sync"] == [], r["pending_after_sync"]
        assert r["syncs"] == 60


def test_the_calls_of_random_shapes_0_raise_no_hazard():
    """the 30 encodes and 30 decodes tests/test_gpu_fuzz.py::test_random_shapes[0] draws, through gpu_support's alloc / upload /
    memset / encode / sync / download / free, on a forced and on a default context, host planner"""
    f = run("fuzz0")
    _fuzz_clean(f)
    assert f["hazards"] == [], f["hazards"][:6]
    assert f["counters"]["launches"] >= 100 and f["counters"]["unnamed_launches"] == 0 and f["counters"]["deferred"] == 0, f["counters"]


# --------------------------------------------------------------------------------- d. what nrq_ctx_sync promises ----
@pytest.mark.parametrize("planner", ["host_planner", "device_planner"])
def test_after_ctx_sync_nothing_pending_touches_the_caller_s_buffers(planner):
    """encode (behind nrq_precalculate), decode, five rounds of nrq_decode_plan_ahead + encode + decode without a wait in
    between, two planner runs issued ahead, one never consumed: behind nrq_ctx_sync no operation of ANY stream touches the three
    buffers the caller passed in, and no hazard was raised on the way.  (device_planner: the planner kernel's effect is
    tests/emu/model_effects.cpp -- the planner streams, the three arena sets and their events are in play.)"""
    s = run("sync")[planner]
    dev = planner == "device_planner"
    for step in ("encode", "decode", "plan_ahead"):
        assert s[step]["before_sync"] == [1, 1, 1] or step == "plan_ahead", (step, s[step])   # (the test sees work in flight at all)
        assert s[step]["after_sync"] == [0, 0, 0], (step, s[step])
    assert s["plan_ahead_two_deep"]["after_sync"] == [0, 0, 0]
    assert s["decode"]["planner"] == int(dev) and s["decode"]["status"] == [1] * 5
    assert all(r["status"] == [1] * 5 and r["plan_ahead"] == int(dev) and r["planner"] == int(dev) for r in s["plan_ahead"]["rounds"]), s["plan_ahead"]
    assert s["plan_ahead_two_deep"]["status"] == [1] * 10 and s["plan_ahead_two_deep"]["plan_ahead"] == int(dev)
    assert s["hazards"] == [], s["hazards"][:6]


def test_a_split_launch_whose_tables_exceed_the_lds_is_refused_before_any_launch():
    """A host plan may have more inactive columns than the device planner's 1280 (the option plan_force_inact makes one: K = 3000,
    all 3135 columns, 98 W words).  On 4-byte strips the split solve's back-substitution tables are then 196 KiB: the call ends
    with a status and has launched nothing -- it used to launch the solve kernel first and report afterwards -- and the next
    call on the context runs as ever (three launches: solve, back-substitution, collect)."""
    r = run("refusal")
    assert r["error"] and "back-substitution tables do not fit the LDS (wpr=98)" in r["error"], r
    assert r["launches_of_the_refused_call"] == 0, r
    assert r["next"]["status"] == [1, 1] and r["next"]["strip_bytes"] == 4 and r["next"]["backsub_strip"] == 32 and r["next"]["u"] < 200, r
    assert r["launches_of_the_next_call"] == 3, r
    assert r["hazards"] == [], r["hazards"][:6]


# ------------------------------------------------------------------- g. a context on a stream of the caller's own ----
# Every group above creates its contexts on stream 0, where an operation the library puts on stream 0 instead of the context's
# stream IS in stream order.  Here the context lives on a model stream of its own (host_model_worker.py "callerstream").
@pytest.mark.parametrize("planner", ["host_planner", "device_planner"])
def test_a_context_on_a_caller_s_stream_raises_no_hazard(planner):
    """the scenarios of group d, the device build of an encode plan (three times, the plan cache cleared in between), a decode whose
    blocks go out in two lists (and once more behind nrq_decode_plan_ahead), nrq_ctl_copy / nrq_scatter_symbols / nrq_move_rows_dev on
    the stream selectors 0 .. 3 ordered by the caller's events, and eight draws of random_shapes[0]: no hazard, nothing pending
    behind nrq_ctx_sync"""
    s = run("callerstream")[planner]
    dev = planner == "device_planner"
    for step in ("encode", "decode", "plan_ahead"):
        assert s[step]["after_sync"] == [0, 0, 0], (step, s[step])
    assert s["encode"]["before_sync"] == [1, 1, 1] and s["decode"]["before_sync"] == [1, 1, 1]   # (there was work in flight)
    assert s["decode"]["planner"] == int(dev) and s["decode"]["status"] == [1] * 5
    assert all(r["status"] == [1] * 5 and r["plan_ahead"] == int(dev) for r in s["plan_ahead"]["rounds"]), s["plan_ahead"]
    assert s["plan_ahead_two_deep"]["after_sync"] == [0, 0, 0] and s["plan_ahead_two_deep"]["status"] == [1] * 10
    m = s["more"]
    two = m["two_lists"]
    assert two and 0 < two["blocks_b"] < 8 and two["status"] == [1] * 8 and two["strip_bytes_b"] < two["strip_bytes"], two
    assert two["plan_ahead"] == int(dev), two
    assert [x["sel"] for x in m["movers"]] == [0, 1, 2, 3] and all(x["rc"] == [0, 0, 0] and x["moved"] for x in m["movers"]), m["movers"]
    f = s["fuzz"]
    assert f["decodes"] == 8 and f["bad_downloads"] == [] and f["pending_after_sync"] == [] and f["syncs"] == 16, f
    assert f["host_planned"] == (4 if dev else 8), f    # (a default context gives its calls of one or two blocks to the host planner)
    assert s["hazards"] == [], s["hazards"][:6]


def test_set_stream_between_two_calls_on_the_same_buffers():
    """nrq_ctx_set_stream to a second stream, to stream 0 and back, each time between an encode and a memset + encode over the same
    three buffers: the move waits for the stream it leaves, so nothing is pending on them when the new stream takes over"""
    s = run("callerstream")["set_stream"]
    assert s["pending_before_and_after_set_stream"] == [[1, 0]] * 3, s
    assert s["hazards"] == [], s["hazards"][:6]


CALLER_DETECTOR = [   # the library's own pattern for its tables: a blocking copy is an operation on stream 0 the host then waits for
    ("blocking_copy_beside_a_kernel_on_the_context_stream", ["H1"]), ("blocking_copy_behind_a_stream_synchronisation", []),
    ("kernel_behind_a_blocking_copy", []),
]


@pytest.mark.parametrize("name,kinds", CALLER_DETECTOR, ids=[d[0] for d in CALLER_DETECTOR])
def test_the_detector_sees_a_blocking_copy_as_an_operation_on_stream_0(name, kinds):
    d = run("callerstream")
    assert d["detector"][name]["kinds"] == kinds, d["detector"][name]["text"]
    if kinds:
        t = d["detector"][name]["text"][0]
        assert "hipMemcpy H2D 4096 B [stream 0" in t and "launch k_reads_table [stream" in t, t
    assert d["pending_at_end"] == 0 and d["counters"]["unnamed_launches"] == 0


# ------------------------------------------------------------- e. the object layer under fault injection, f. ----
FLOORS = {   # scenario: (runs that met their injected failure, batches taken back) at least -- the floors of tests/test_gpu_faults.py
    "batch_sync": (20, 3), "batch_async": (20, 3), "repair_all_device": (10, 0), "repair_all_host": (10, 0), "per_block": (10, 0),
    "repair_rows": (8, 3), "host_block_in_a_deferred_chunk": (0, 0), "rows_grown_under_a_deferred_batch": (0, 0),
}


@pytest.mark.parametrize("name", list(FLOORS))
def test_the_object_layer_under_fault_injection(name):
    """tests/test_gpu_faults.py's scenarios on the model (object_model_scenarios.py): for every n of the sweep no hazard, the
    reference's return conventions, books that match the results, a retry that succeeds, and the received source symbols --
    which travel by copies alone -- where they belong in the output."""
    s = run("process")["faults"][name]
    assert s["hazards"] == [], s["hazards"][:6]
    assert s["failures"] == [], s["failures"][:6]
    hit, rolled = FLOORS[name]
    assert s["hit"] >= hit and s["rolled_back"] >= rolled, (s["hit"], s["rolled_back"], "the sweep did not reach the runtime calls")


def test_the_process_that_faulted():
    """the object layer's fault sweeps, then random_shapes[0] on fresh contexts in the same process: no hazard, nothing pending
    from the sweeps, every download inside a live block"""
    p = run("process")
    assert p["faults"]["pending_at_end"] == 0
    _fuzz_clean(p["fuzz0"])
    assert p["hazards"] == [], p["hazards"][:6]
    assert p["counters"]["unnamed_launches"] == 0
