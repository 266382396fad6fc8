"""CPU tier: a whole solve launch on fenced memory (tests/emu/launch_emu.cpp, tests/launch_emu_support.py).

What the other emulation tests cannot see: they run ONE work slot of one block on numpy arrays, where a read or write a few bytes
past `src`, `rep`, `inter`, `out`, the plan arena, the lists or the staging buffers lands in numpy's heap and nothing notices.  Here
the launch is the one the host would make -- solve_lists / solve_shape on the call's plan headers, with the options the GPU tests
set -- and it runs as nrq_solve_kernel runs it: every workgroup of the grid, its work slots by nrq_map_group / nrq_next_group (the
kernel's own two functions), the first group gathered whole, per strip index the portions of the next group's gather and the
previous group's scatter with their late parts, moved by the threads that move them on the GPU (the single wave, the gather and
scatter waves, the waves the HDPC phase leaves idle), the strip-less portions, both staging sets, the last group's scatter; the
movers in the form the HOST chose (aligned only, or byte-wise; pipelined in the full-size workgroup); ph_store's list reads in
the device's unbounded form, its fast form under wave-wide ballots (a wave's 64 lanes in step); then nrq_backsub_kernel / nrq_collect_kernel behind a split launch.

Every array lives in a mapping of its own between two PROT_NONE pages at exactly the size the host gives it: staging area
stage_bytes(), work buffers nblk * ybuf_stride, the LDS image the launch's dynamic LDS, out_slots[] by the formula of the host site
the case mirrors (encode_blocks, decode_host, the device planner's pl_final_b inside the arena cut at total_bytes).  Every case runs
twice: arrays ending in front of the upper page, arrays beginning behind the lower page (there also 1 / 4 / 8 bytes behind it, so
that the byte-wise movers run on unaligned rows).  No sanitizer is involved.

The cases run in a child process per group (tests/launch_bounds_worker.py has the tables): a fence hit ends the child in the
emulation's signal handler, which prints the array, the side, the distance and where the launch was; the child prints every case
before it starts.  A group passes when the child ends clean: no fence hit, no byte next to an array changed, every block
bit-exact with the oracle (repair symbols, intermediate symbols, recovered rows, the verdict), rows that must stay as they were
untouched, and every form the group is there for reached.  All phases run for every strip: measured, 18 tests in 103 s on
one core with every library built (the fast form of ph_store runs each wave several times, tests/emu/wave_emu.h); from a clean
checkout the first test also builds the product library, the oracle and the emulators (about three minutes more)."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GROUPS = ("w16", "w12", "w8", "w4", "w2", "w4sb16", "w4nosplit", "wide2", "wide4", "decode", "needview", "big", "edge", "seed0",
          "forced_k100", "forced_k1000", "forced_k3000", "forced_k5200", "forced_k10000", "forced_k15000")


@pytest.mark.parametrize("group", GROUPS)
def test_launch_stays_inside_its_arrays(group):
    """w16 ... w2, w4sb16 (16-byte strips of the split tail), w4nosplit, wide2 / wide4: the encode sweep of one strip width over the
    contexts; decode: lost symbols, overhead 0 and 5, an undecodable block that nrq_next_group must skip, arrays as decode_host and as
    the device planner lay them out; big: K = 1024 and 3100; edge: the slack behind out_slots[] with lists of 33 entries and the
    output staging stride at 1, 17 and 33 elements; seed0: the 30 encodes tests/test_gpu_fuzz.py::test_random_shapes[0] draws, on the
    forced context's options with the intermediate symbols wanted; forced_k*: every call of tests/test_gpu_backsub_forms.py -- plans at
    a forced number of inactive columns, up to 1281 of them (forced_inact_support.GPU_CASES) -- before it may run on a GPU."""
    r = subprocess.run([sys.executable, os.path.join(HERE, "launch_bounds_worker.py"), group], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = r.stdout.decode(errors="replace")
    hits = [line for line in out.splitlines() if line.startswith("FENCE HIT")]
    assert not hits, "\n".join(hits + out.splitlines()[-2:])
    assert r.returncode == 0 and out.rstrip().splitlines()[-1].startswith("ok:"), out[-3000:]


def test_the_handler_names_the_array_and_the_side():
    """the fence itself: a read one byte past an array that ends at its upper page, a write one byte in front of one that begins behind
    its lower page -- the child ends with the handler's line, which names the array, the side and the distance"""
    code = ("import sys, ctypes as C; sys.path.insert(0, %r); import launch_emu_support as S; L = S.lemu(); L.lemu_install_handler();"
            "a, p = S.Arena(int(sys.argv[1])).place('probe', 48, fill=1);"
            "print('alive', a[47] if sys.argv[1] == '0' else a[0], flush=True);"
            "C.string_at(p + 48, 1) if sys.argv[1] == '0' else C.memset(p - 1, 0, 1)" % HERE)
    for side, where in ((0, "ABOVE"), (1, "BELOW")):
        r = subprocess.run([sys.executable, "-c", code, str(side)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        out = r.stdout.decode(errors="replace")
        assert r.returncode == 97 and "alive 1" in out, out
        assert "FENCE HIT" in out and "%s the array 'probe' (1 byte(s) outside)" % where in out, out


def test_margins_are_checked():
    """bytes of an array's own pages that are not the array's: a write there is no fault, lemu_check_margins finds it"""
    import launch_emu_support as S
    L = S.lemu()
    try:
        a, p = S.Arena(0).place("probe", 40, fill=0)
        assert L.lemu_check_margins() is None
        import ctypes as C
        C.memset(p - 1, 0, 1)
        assert L.lemu_check_margins() == b"probe"
    finally:
        L.lemu_release_all()


def test_seed0_trials_are_the_fuzz_test_s():
    """the worker's restatement of the generator calls gives the shapes the GPU test draws, all 30: the GPU test's own function runs
    on a stand-in for the GPU (the encode returns zeros of the right shapes, the decode the source) and a stand-in oracle that
    agrees with it, and every gpu_encode call is recorded"""
    import numpy as np
    import nanorq_amd
    import launch_bounds_worker as W
    import test_gpu_fuzz as F

    class FakeG:
        def __init__(self):
            self.calls = []

        def gpu_encode(self, src, K, T, esis, want_inter=False):
            self.calls.append((K, T, src.shape[0], len(esis)))
            self.src = src
            assert want_inter
            return np.zeros((src.shape[0], len(esis), T), np.uint8), np.zeros((src.shape[0], nanorq_amd.params(K)["L"], T), np.uint8)

        def gpu_decode(self, work, K, T, lost, esis, reps):
            return np.ones(len(lost), np.int32), self.src, None

    class FakeOrc:
        @staticmethod
        def encode_block(src, K, T, esis, want_inter=False):
            return np.zeros((len(esis), T), np.uint8), np.zeros((nanorq_amd.params(K)["L"], T), np.uint8), {}

        @staticmethod
        def decode_block(rx, syms, K, T):
            return True, None, {}

    g = FakeG()
    F._random_shapes(g, FakeOrc, 0)
    assert g.calls == W.seed0_trials() and len(g.calls) == 30


def test_a_wave_s_lanes_run_in_step():
    """wave_emu.h: under NRQ_WAVE_ANY every lane of a wave goes round a loop as often as its neediest lane, as under the device's ballot
    (ph_store's fast form reads its second trip of a short list that way)"""
    import launch_emu_support as S
    assert S.lemu().lemu_wave_selftest() == 5000


# What solve_roles() (nanorq_amd/csrc/solve_roles.h) must say of every instance of NRQ_SOLVE_INSTANCES, in that list's order:
# (WB, NT, WV, G, AL): (NFW, NGW, NSW, MPIPE, ALX, RU, HNT, SLATE, GLATE, ph_hdpc REGS, ph_dense_fold BATCH, ph_dense_free / _cu BATCH,
# ph_backsub / ph_store FAST, pf_commit PB).  Numbers, worked out once from the expressions the kernel and the emulation each held
# before there was one statement.  (NSW of the single wave: NMV - NGW = 0 - 1 in unsigned arithmetic; it has no mover waves and
# nobody reads it.)
ROLES = {
    (16, 768, 1, 1, 0): (2, 2, 2, 1, 0, 120, 512, 20, 40, 0, 0, 0, 1, 8),
    (16, 768, 1, 1, 1): (2, 2, 2, 1, 1, 120, 512, 20, 40, 0, 0, 0, 1, 8),
    (16, 256, 4, 1, 0): (1, 2, 1, 0, 0, 60, 256, 20, 40, 0, 0, 0, 0, 8),
    (16, 256, 4, 1, 1): (1, 2, 1, 0, 1, 60, 256, 20, 40, 0, 0, 0, 0, 8),
    (16, 256, 5, 1, 0): (1, 2, 1, 0, 0, 36, 256, 20, 40, 0, 0, 0, 0, 8),
    (16, 256, 5, 1, 1): (1, 2, 1, 0, 1, 36, 256, 20, 40, 0, 0, 0, 0, 8),
    (16, 64, 3, 1, 0): (1, 1, 4294967295, 0, 0, 24, 64, 20, 40, 0, 8, 1, 0, 4),
    (16, 64, 3, 1, 1): (1, 1, 4294967295, 0, 1, 24, 64, 20, 40, 0, 8, 1, 0, 4),
    (16, 256, 4, 2, 0): (1, 2, 1, 0, 0, 60, 256, 20, 40, 0, 0, 0, 0, 8),
    (16, 256, 4, 4, 0): (1, 2, 1, 0, 0, 60, 256, 20, 40, 0, 0, 0, 0, 8),
    (16, 256, 4, 8, 0): (1, 2, 1, 0, 0, 60, 256, 20, 40, 0, 0, 0, 0, 8),
    (12, 768, 1, 1, 0): (3, 2, 2, 1, 0, 120, 512, 20, 40, 0, 0, 0, 1, 8),
    (12, 768, 1, 1, 1): (3, 2, 2, 1, 1, 120, 512, 20, 40, 0, 0, 0, 1, 8),
    (8, 768, 1, 1, 0): (2, 2, 2, 1, 0, 120, 512, 20, 40, 0, 0, 0, 1, 8),
    (8, 768, 1, 1, 1): (2, 2, 2, 1, 1, 120, 512, 20, 40, 0, 0, 0, 1, 8),
    (8, 256, 4, 1, 0): (1, 2, 1, 0, 0, 60, 256, 20, 40, 0, 0, 0, 0, 8),
    (8, 256, 4, 1, 1): (1, 2, 1, 0, 1, 60, 256, 20, 40, 0, 0, 0, 0, 8),
    (8, 256, 5, 1, 0): (1, 2, 1, 0, 0, 36, 256, 20, 40, 0, 0, 0, 0, 8),
    (8, 256, 5, 1, 1): (1, 2, 1, 0, 1, 36, 256, 20, 40, 0, 0, 0, 0, 8),
    (8, 64, 3, 1, 0): (1, 1, 4294967295, 0, 0, 24, 64, 20, 40, 0, 8, 1, 0, 4),
    (8, 64, 3, 1, 1): (1, 1, 4294967295, 0, 1, 24, 64, 20, 40, 0, 8, 1, 0, 4),
    (4, 768, 1, 1, 0): (1, 2, 2, 1, 0, 120, 512, 10, 15, 1, 0, 0, 1, 8),
    (4, 768, 1, 1, 1): (1, 2, 2, 1, 1, 120, 512, 10, 15, 1, 0, 0, 1, 8),
    (4, 256, 4, 1, 0): (1, 2, 1, 0, 0, 60, 256, 10, 15, 0, 0, 0, 0, 8),
    (4, 256, 4, 1, 1): (1, 2, 1, 0, 1, 60, 256, 10, 15, 0, 0, 0, 0, 8),
    (4, 256, 5, 1, 0): (1, 2, 1, 0, 0, 36, 256, 10, 15, 0, 0, 0, 0, 8),
    (4, 256, 5, 1, 1): (1, 2, 1, 0, 1, 36, 256, 10, 15, 0, 0, 0, 0, 8),
    (4, 64, 3, 1, 0): (1, 1, 4294967295, 0, 0, 24, 64, 10, 15, 0, 8, 1, 0, 4),
    (4, 64, 3, 1, 1): (1, 1, 4294967295, 0, 1, 24, 64, 10, 15, 0, 8, 1, 0, 4),
    (2, 768, 1, 1, 0): (1, 2, 2, 1, 0, 120, 512, 10, 15, 1, 0, 0, 1, 8),
    (2, 768, 1, 1, 1): (1, 2, 2, 1, 0, 120, 512, 10, 15, 1, 0, 0, 1, 8),
    (2, 256, 4, 1, 0): (1, 2, 1, 0, 0, 60, 256, 10, 15, 0, 0, 0, 0, 8),
    (2, 256, 4, 1, 1): (1, 2, 1, 0, 0, 60, 256, 10, 15, 0, 0, 0, 0, 8),
    (2, 256, 5, 1, 0): (1, 2, 1, 0, 0, 36, 256, 10, 15, 0, 0, 0, 0, 8),
    (2, 256, 5, 1, 1): (1, 2, 1, 0, 0, 36, 256, 10, 15, 0, 0, 0, 0, 8),
    (2, 64, 3, 1, 0): (1, 1, 4294967295, 0, 0, 24, 64, 10, 15, 0, 8, 1, 0, 4),
    (2, 64, 3, 1, 1): (1, 1, 4294967295, 0, 0, 24, 64, 10, 15, 0, 8, 1, 0, 4),
}
KNOBS = {"NRQ_W12_FW": 3, "NRQ_W12_GW": 2, "NRQ_W12_SW": 2, "NRQ_MOVER_WAVES": 2, "NRQ_GATHER_WAVES_NARROW": 2, "NRQ_GATHER_WAVES_NARROW_WB": 2,
         "NRQ_PIPE_BIG": 1, "NRQ_PIPE_SMALL": 0, "NRQ_HDPC_NT": 512, "NRQ_HDPC_NT_SMALL": 256, "NRQ_SCATTER_LATE_PCT": 20, "NRQ_GATHER_LATE_PCT": 40,
         "NRQ_SCATTER_LATE_PCT_NARROW": 10, "NRQ_GATHER_LATE_PCT_NARROW": 15, "NRQ_HDPC_REGS_MAX_WB": 4, "NRQ_HDPC_REGS_12": 0, "NRQ_FOLD_PRE256": 0}


def test_the_kernel_s_roles_are_pinned():
    """the kernel and the emulation take their wave roles and phase forms from one statement (solve_roles.h); what it says is pinned
    here against numbers: the 17 role knobs as the emulation library was compiled with them (the macros themselves), and for every
    compiled instance the fields of solve_roles() that steer the kernel"""
    import ctypes as C
    import launch_emu_support as S
    L = S.lemu()
    L.lemu_role_knobs.restype = C.c_char_p
    L.lemu_instance_roles.restype = C.c_char_p
    L.lemu_instance_roles.argtypes = [C.c_int]
    knobs = {k: int(v) for k, v in (kv.split("=") for kv in L.lemu_role_knobs().decode().split())}
    assert len(KNOBS) == 17 and knobs == KNOBS
    got, i = [], 0
    while L.lemu_instance_roles(i) is not None:
        key, fields = L.lemu_instance_roles(i).decode().split(":")
        got.append((tuple(int(x) for x in key.split()), tuple(int(x) for x in fields.split())))
        i += 1
    assert len(ROLES) == 37 and got == list(ROLES.items())
