"""The launch decisions (nanorq_amd/csrc/launch_shape.h) on the CPU: solve_lists, solve_shape and plan_shape through
tests/emu/shape_emu.cpp, swept over sizes and over every knob a test can set.  Nothing here records today's numbers -- tuning may
move -- only what must hold for ANY tuning: the record names a compiled instance, what it sizes fits the LDS, the grid and the
work slots cover the launch, and a form is chosen only where its preconditions hold.  No GPU needed."""
import ctypes as C
import itertools

import pytest

from nanorq_amd import build as nbuild

U32 = C.c_uint32
WIDTHS = (16, 12, 8, 4, 2)
SOLVE_OUT = ("err", "WB", "NT", "WV", "G", "AL", "lds", "wg_threads", "wg_waves", "split", "by_block", "nstrips", "spl", "occ", "grid",
             "lsub", "nslots", "stage_stride", "ostage_stride", "ybuf_stride", "res_elems", "backsub_strip", "backsub_tbl", "nchunks", "stage_bytes_lo",
             "stage_bytes_hi")
PLAN_OUT = ("err", "wg_threads", "compact", "segmented", "mode", "nparts", "part0", "part1", "part2", "qcap", "lowcap", "sh_bytes",
            "dyn_bytes", "wentry_wgs", "wpass_wgs", "wpass_lds", "mh_wgs", "mh_dyn")

# every knob setting a test reaches through an option, one at a time (and the defaults)
SOLVE_KNOBS = [{}, {"tiny_any": 1}, {"no_tiny": 1}, {"small_waves4": 0}, {"big_wg": 1}, {"wide_g": 2}, {"wide_g": 4}, {"wide_g": 8},
               {"no_split": 1}, {"solve_grid": 64}, {"solve_grid": 1000}, {"reserve_cus": 0}, {"reserve_cus": 40},
               {"wide_g": 4, "big_wg": 1}, {"tiny_any": 1, "small_waves4": 0}, {"backsub_sb": 16}]
LIST_KNOBS = [{}, {"max_wb": 8}, {"max_wb": 12}, {"max_wb": 2}, {"no_wb12": 1}, {"lds_max": 60000}, {"lds_max": 20000}, {"no_lists": 1},
              {"lds_max": 100000, "no_wb12": 1}]
PLAN_KNOBS = [{}, {"plan_pack": 1}, {"plan_big_wg": 1}, {"plan_split_force": 1}, {"plan_wrong_instance": 1},
              {"plan_pack": 1, "plan_split_force": 1}, {"plan_pack": 1, "plan_wrong_instance": 1}, {"plan_no_out_view": 1},
              {"plan_no_out_view": 1, "plan_split_force": 1}]


@pytest.fixture(scope="module")
def emu():
    L = C.CDLL(nbuild.build_shape_emu())
    L.emu_tuning_new.restype = C.c_void_p
    L.emu_tuning_free.argtypes = [C.c_void_p]
    L.emu_tuning_set.argtypes = [C.c_void_p, C.c_char_p, C.c_longlong]
    L.emu_lds_need.argtypes = [C.c_void_p, U32]
    L.emu_widest_fit.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.emu_solve_lists.argtypes = [C.c_void_p, C.c_void_p, U32, C.c_int, C.c_void_p, C.c_void_p]
    L.emu_solve_shape.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, U32, C.c_void_p]
    L.emu_plan_shape.argtypes = [C.c_void_p, C.c_int, U32, U32, U32, U32, C.c_void_p]
    L.emu_map_group.argtypes = [U32, U32, U32, C.c_int, C.c_void_p]
    for f in (L.emu_lds_max, L.emu_lds_alloc, L.emu_lds_need, L.emu_map_by_block, L.emu_widest_fit):
        f.restype = U32
    return L


class Tuning:
    def __init__(self, emu, knobs):
        self.emu, self.knobs = emu, knobs
        self.p = emu.emu_tuning_new()
        for name, value in knobs.items():
            assert emu.emu_tuning_set(self.p, name.encode(), value) == 0, name

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.emu.emu_tuning_free(self.p)


def hdr_words(hdrs):
    """(M, r2, u, wpr, status) per header, flat"""
    return (U32 * (5 * len(hdrs)))(*itertools.chain.from_iterable(hdrs))


def lds_need(emu, h, w):
    return emu.emu_lds_need(hdr_words([h]), w)


def header_for(emu, wb, need, u):
    """a synthetic plan header whose strip image at width wb takes about `need` bytes of LDS (None: no such header)"""
    wpr = (u + 31) // 32
    base = lds_need(emu, (1, 0, u, wpr, 0), wb)
    if base > need:
        return None
    return (1 + (need - base) // wb, 0, u, wpr, 0)


def test_knob_names(emu):
    """an option name the table does not hold is refused; fault injection is not a knob"""
    with Tuning(emu, {}) as t:
        for name in (b"no_lists", b"no_wb12", b"max_wb", b"no_split", b"wide_g", b"lds_max", b"plan_ucap", b"tx_dword", b"host_plan_auto",
                     b"backsub_sb", b"plan_force_inact", b"plan_no_out_view"):
            assert emu.emu_tuning_set(t.p, name, 1) == 0, name
        for name in (b"fail_after", b"faults_injected", b"nonsense", b"NRQ_NO_LISTS", b""):
            assert emu.emu_tuning_set(t.p, name, 1) == -1, name


def test_compiled_instances(emu):
    """the key list: 37 solve instances -- 4 shapes x 2 mover forms of 16 / 8 / 4 / 2 bytes, the 12-byte pair, 3 wide -- and 4 planner ones"""
    keys = [(wb, nt, wv, g, al) for wb in (16, 12, 8, 4, 2, 1, 32) for nt, wv in ((768, 1), (256, 4), (256, 5), (64, 3), (512, 2), (256, 1))
            for g in (1, 2, 4, 8) for al in (0, 1)]
    have = [k for k in keys if emu.emu_solve_key_compiled(*k)]
    assert len(have) == 37
    assert all(nt == 768 for wb, nt, wv, g, al in have if wb == 12)
    assert all(wb == 16 and nt == 256 and not al for wb, nt, wv, g, al in have if g > 1)
    assert [k for k in itertools.product((1024, 256, 128, 64), (0, 1)) if emu.emu_plan_key_compiled(*k)] == [(1024, 0), (1024, 1), (256, 0), (128, 0)]


def test_solve_shape_holds_for_any_tuning(emu):
    LDS = emu.emu_lds_max()
    needs = (300, 2000, 9000, 13000, 23000, 32000, 40000, 81000, 82500, 120000, LDS)
    nblks = (1, 2, 7, 8, 16, 63, 64, 65, 256, 1000, 4000)  # (65: mapped by block octets, the last octet of one block)
    Ts = (16, 40, 64, 72, 100, 1024, 1280, 1288)
    out = (U32 * len(SOLVE_OUT))()
    cases = refused = 0
    for knobs in SOLVE_KNOBS:
        with Tuning(emu, knobs) as t:
            for wb, need, nblk, T, many, ncu, io in itertools.product(WIDTHS, needs, nblks, Ts, (False, True), (256, 64), (0, 1)):
                if (nblk + T + need // 100 + ncu + io) % 5 > 1 and knobs:  # (a fraction of the grid for the non-default knobs: seconds, not minutes)
                    continue
                u = 20 if need < 40000 else 700
                h = header_for(emu, wb, need, u)
                if h is None:
                    continue
                hdrs = [h] if not many else [h, (max(1, h[0] // 2), 3, u // 2, (u // 2 + 31) // 32, 0), (h[0], 0, 0, 0, 1)]
                lds = lds_need(emu, h, wb)
                assert lds <= LDS
                max_out = 0 if nblk == 7 else h[0] // 3 + 2
                emu.emu_solve_shape(t.p, (U32 * 8)(wb, nblk, T, lds, max_out, io, ncu, 2 if nblk == 2 else 0), hdr_words(hdrs), len(hdrs), out)
                s = dict(zip(SOLVE_OUT, out))
                what = "%r wb=%d need=%d nblk=%d T=%d many=%d ncu=%d io=%d: %r" % (knobs, wb, need, nblk, T, many, ncu, io, s)
                cases += 1
                assert s["err"] == 0, what
                # the instance exists, and it is the one the record was sized for
                assert emu.emu_solve_key_compiled(s["WB"], s["NT"], s["WV"], s["G"], s["AL"]), what
                assert s["WB"] == wb, what
                assert s["G"] == 1 or (wb == 16 and s["G"] == knobs.get("wide_g") and T >= 16 * s["G"]), what
                if s["G"] == 1:
                    assert (s["NT"], s["WV"]) == (s["wg_threads"], s["wg_waves"]), what
                assert wb != 12 or s["NT"] == 768, what
                if s["AL"]:
                    assert io and s["G"] == 1 and wb >= 4 and T % (4 if wb == 12 else wb) == 0, what
                # the workgroups a CU is given fit it: LDS by the allocation granule, 2048 threads
                assert s["occ"] >= 1 and s["occ"] * emu.emu_lds_alloc(s["lds"]) <= LDS, what
                assert s["occ"] * s["wg_threads"] <= 2048, what
                assert s["G"] > 1 or s["lds"] == lds, what
                # the split: exactly the narrow strips, unless it is switched off
                assert s["split"] == (1 if wb <= 4 and not knobs.get("no_split") else 0), what
                # work slots cover every strip of every block; the grid is at least 8 unless there are fewer slots
                wbe = wb * s["G"]
                assert s["nstrips"] == -(-T // wbe), what
                assert s["by_block"] == emu.emu_map_by_block(nblk), what
                sub = 1 << s["lsub"]
                assert sub <= s["spl"], what  # (a slot's strips each have a staging buffer of their own: there are spl per set)
                assert s["nslots"] == ((nblk + 7) // 8 * 8 if s["by_block"] else nblk) * -(-s["nstrips"] // sub), what
                assert 1 <= s["grid"] <= s["nslots"], what
                assert s["grid"] >= 8 or s["grid"] == s["nslots"], what
                assert not s["by_block"] or s["grid"] % 8 == 0, what
                # the slots as nrq_map_group deals them: each of the last eight (the last block octet) is a group of a block of the launch
                # or is refused (a partial octet), and the last group of the last block has a slot
                gpb, bg = -(-s["nstrips"] // sub), (U32 * 2)()
                for q in range(max(0, s["nslots"] - 8), s["nslots"]):
                    if emu.emu_map_group(q, nblk, gpb, s["by_block"], bg):
                        assert bg[0] < nblk and bg[1] < gpb, what
                    else:
                        assert s["by_block"] and nblk % 8 and bg[0] >= nblk, what
                        refused += 1
                q_last = (((nblk - 1) // 8 * gpb + gpb - 1) * 8 + (nblk - 1) % 8) if s["by_block"] else (nblk - 1) * gpb + gpb - 1
                assert q_last < s["nslots"] and emu.emu_map_group(q_last, nblk, gpb, s["by_block"], bg) and tuple(bg) == (nblk - 1, gpb - 1), what
                # staging holds the rows of a strip, in whole 256-byte pieces
                rows_out = h[0] + u if s["split"] else max_out
                assert s["stage_stride"] % 256 == 0 and s["stage_stride"] >= h[0] * wbe, what
                assert s["ostage_stride"] % 256 == 0 and s["ostage_stride"] >= rows_out * wbe, what
                # ... two sets of spl input and spl output buffers per workgroup: what the kernel strides through
                assert s["stage_bytes_lo"] | s["stage_bytes_hi"] << 32 == s["grid"] * 2 * s["spl"] * (s["stage_stride"] + s["ostage_stride"]), what
                if s["split"]:
                    assert s["ybuf_stride"] % 256 == 0 and s["ybuf_stride"] >= (h[0] + u) * T, what
                    assert s["res_elems"] == max_out, what
                    assert s["backsub_strip"] in (16, 32) and 1 <= s["nchunks"] <= 16, what
                    assert emu.emu_lds_alloc(s["backsub_tbl"]) * (2 if s["backsub_strip"] == 32 else 1) <= LDS, what
                    # 16-byte strips beyond 20 W words, or when the test knob asks for them; the tables are those of that strip
                    assert s["backsub_strip"] == (16 if (u + 31) // 32 > 20 or knobs.get("backsub_sb") == 16 else 32), what
                    assert s["backsub_tbl"] == (u + 31) // 32 * 128 * s["backsub_strip"], what
                else:
                    assert s["backsub_strip"] == 0, what
    assert cases > 20000 and refused > 500


def test_plan_shape_holds_for_any_tuning(emu):
    LDS = emu.emu_lds_max()
    out = (U32 * len(PLAN_OUT))()
    scan_rule_met = scan_rule_small = 0
    for knobs in PLAN_KNOBS:
        with Tuning(emu, knobs) as t:
            for K, nblk, oh, ncu in itertools.product((10, 100, 256, 500, 1000, 1500, 2500, 4000, 8192, 15000, 27000, 56403),
                                                      (1, 2, 8, 64, 256, 257, 1024, 4000), (0, 30, 2000), (256, 64)):
                where = emu.emu_plan_shape(t.p, ncu, K, nblk, oh, 0, out)
                s = dict(zip(PLAN_OUT, out))
                what = "%r K=%d nblk=%d overhead=%d ncu=%d: %r, state %d" % (knobs, K, nblk, oh, ncu, s, where)
                assert where >= 0 and s["err"] == 0, what
                assert emu.emu_plan_key_compiled(s["wg_threads"], s["compact"]), what
                assert s["dyn_bytes"] + s["sh_bytes"] <= LDS, what
                if knobs.get("plan_wrong_instance"):  # the wrong instance on purpose: blocks whose state fits the LDS get the compact one
                    assert s["wg_threads"] != 1024 or s["compact"] == 1, what
                else:
                    assert s["compact"] == (1 if where == 0 else 0), what
                if s["wg_threads"] == 128:
                    assert 6 * emu.emu_lds_alloc(s["dyn_bytes"] + s["sh_bytes"]) <= LDS, what
                elif s["wg_threads"] == 256:
                    assert 2 * emu.emu_lds_alloc(s["dyn_bytes"] + s["sh_bytes"]) <= LDS, what
                if knobs.get("plan_big_wg"):
                    assert s["wg_threads"] == 1024, what
                # the layout rule of the planner's prefix scan (planner_body.h pl_final_c2): a block may miss all K source symbols, and
                # with more than 2 * qcap missing the list offsets come from a scan whose wg_threads + 1 words start at the first
                # frontier queue and must end in front of the claim lists, 4 * qcap bytes on (two queues of qcap two-byte entries)
                if K > 2 * s["qcap"]:
                    scan_rule_met += 1
                    assert (s["wg_threads"] + 1) * 4 <= 4 * s["qcap"], what
                scan_rule_small += K > 2 * s["qcap"] and s["wg_threads"] < 1024
                # bit 10 of the jobs' mode: no out view (the option plan_no_out_view), and nothing else about the run
                nov = 0x400 if knobs.get("plan_no_out_view") else 0
                assert s["mode"] & 0x400 == nov, what
                if nov:
                    with Tuning(emu, {k: v for k, v in knobs.items() if k != "plan_no_out_view"}) as t0:
                        out0 = (U32 * len(PLAN_OUT))()
                        assert emu.emu_plan_shape(t0.p, ncu, K, nblk, oh, 0, out0) == where, what
                        s0 = dict(zip(PLAN_OUT, out0))
                        assert s0 == dict(s, mode=s["mode"] & ~0x400), what
                if knobs.get("plan_split_force"):
                    assert s["segmented"], what
                if s["segmented"]:
                    # the full-size compact instance, its state in the workspace; the helper kernels fit the LDS
                    assert (s["wg_threads"], s["compact"], where) == (1024, 1, 0), what
                    assert s["mode"] & ~0x400 in (0x100, 0x300), what
                    parts = [s["part0"], s["part1"], s["part2"]][:s["nparts"]]
                    assert parts == ([3, 4, 2] if s["mode"] & 0x300 == 0x300 else [1, 2]), what
                    assert s["mh_dyn"] + s["sh_bytes"] <= LDS and s["wpass_lds"] <= LDS, what
                    assert 2 <= s["wentry_wgs"] <= 8 and 1 <= s["mh_wgs"] <= 64 and s["wpass_wgs"] >= 2, what
                else:
                    assert (s["nparts"], s["part0"], s["mode"]) == (1, 0, nov), what
    # the sweep holds shapes the rule is about, 256-thread ones among them (K = 2500 in packed workgroups: qcap 1024)
    assert scan_rule_met > 100 and scan_rule_small > 10


def test_solve_lists_partition(emu):
    LDS = emu.emu_lds_max()
    # batches: everybody alike; one odd block with many inactive columns; a minority / a majority of big blocks; unsolvable ones
    small, mid, big, huge = (1100, 10, 40, 2, 0), (8400, 10, 150, 5, 0), (8400, 40, 900, 29, 0), (30000, 40, 900, 29, 0)
    dead = (8400, 10, 150, 5, 1)
    batches = [[small] * 9, [mid] * 12, [mid] * 11 + [big], [mid] * 5 + [big] * 7, [big, mid, dead, mid, mid], [dead] * 3,
               [mid, big], [huge, mid, mid, big], [small, huge], [big] * 4 + [huge] * 3 + [mid] * 8 + [dead]]
    out, need = (U32 * 7)(), U32()
    two_seen = 0
    for knobs in LIST_KNOBS:
        lds_max = knobs.get("lds_max", LDS)
        allowed = [w for w in WIDTHS if w <= knobs.get("max_wb", 16) and not (w == 12 and knobs.get("no_wb12"))]
        with Tuning(emu, knobs) as t:
            for hdrs, can_split in itertools.product(batches, (1, 0)):
                what = "%r %r can_split=%d" % (knobs, hdrs, can_split)
                wd = []
                for h in hdrs:  # widest_fit: the widest allowed width whose image fits
                    w = emu.emu_widest_fit(t.p, hdr_words([h]), C.byref(need))
                    fits = [x for x in allowed if lds_need(emu, h, x) <= lds_max]
                    assert w == (max(fits) if fits else 0) and need.value == (lds_need(emu, h, w) if w else 0), what
                    wd.append(w)
                on_b = (C.c_uint8 * len(hdrs))()
                emu.emu_solve_lists(t.p, hdr_words(hdrs), len(hdrs), can_split, out, on_b)
                err, nsolv, two, wa, need_a, wb, need_b = out
                solv = [i for i, h in enumerate(hdrs) if not h[4]]
                if any(wd[i] == 0 for i in solv):
                    assert err != 0, what
                    continue
                assert err == 0 and nsolv == len(solv), what
                if not solv:
                    continue
                top = max(wd[i] for i in solv)
                na = sum(1 for i in solv if wd[i] == top)
                nb = len(solv) - na
                # one list in exactly four cases
                single = nb == 0 or not can_split or bool(knobs.get("no_lists")) or na < nb
                assert two == (0 if single else 1), what
                if single:
                    w = top if nb == 0 else min(wd[i] for i in solv)
                    assert wa == w and need_a == max(lds_need(emu, hdrs[i], w) for i in solv) <= lds_max, what
                    assert not any(on_b), what
                else:
                    two_seen += 1
                    # every solvable header on exactly one list, at a width whose image fits
                    assert [on_b[i] for i in range(len(hdrs))] == [1 if i in solv and wd[i] < top else 0 for i in range(len(hdrs))], what
                    assert wa == top and wb == min(wd[i] for i in solv if wd[i] < top), what
                    assert need_a == max(lds_need(emu, hdrs[i], wa) for i in solv if not on_b[i]) <= lds_max, what
                    assert need_b == max(lds_need(emu, hdrs[i], wb) for i in solv if on_b[i]) <= lds_max, what
    assert two_seen >= 5
