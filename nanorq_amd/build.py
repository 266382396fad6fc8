"""Builds the in-tree native libraries.

  libnanorq_hip.so   product: gfx950 kernels + C ABI (include/nanorq_hip.h) + drop-in nanorq.h/io.h
                     layer, compiled with hipcc --offload-arch=gfx950 (cross-compiles without a GPU)
  tests/emu/lib*_emu.so       test support: the kernels' phase code and the launch decisions, built by g++ for the CPU tier
  tests/emu/libnanorq_model.so  test support: the library's HOST layer, from the same sources, over a model of the HIP runtime
  tests/gpu/librows_probe.so  test support: the row pipelines of solve_body.h behind kernels of their own (gfx950, needs a GPU to run)

The .so files are git-ignored but travel to the GPU box with the working tree.
"""
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libnanorq_hip.so")
EMU = os.path.join(ROOT, "tests", "emu", "libsolve_emu.so")
PEMU = os.path.join(ROOT, "tests", "emu", "libplanner_emu.so")
IEMU = os.path.join(ROOT, "tests", "emu", "libingest_emu.so")
XEMU = os.path.join(ROOT, "tests", "emu", "libemit_emu.so")
OEMU = os.path.join(ROOT, "tests", "emu", "libobj_emu.so")
SEMU = os.path.join(ROOT, "tests", "emu", "libshape_emu.so")
HEMU = os.path.join(ROOT, "tests", "emu", "libheld_emu.so")
WEMU = os.path.join(ROOT, "tests", "emu", "libwant_emu.so")
REMU = os.path.join(ROOT, "tests", "emu", "librxset_emu.so")
LEMU = os.path.join(ROOT, "tests", "emu", "librxset_lists_emu.so")
QEMU = os.path.join(ROOT, "tests", "emu", "librxset_want_emu.so")
TEMU = os.path.join(ROOT, "tests", "emu", "libtxset_emu.so")
KEMU = os.path.join(ROOT, "tests", "emu", "libtxset_range_emu.so")
YEMU = os.path.join(ROOT, "tests", "emu", "libsyms_emu.so")
ZEMU = os.path.join(ROOT, "tests", "emu", "libsyms_set_emu.so")
GEMU = os.path.join(ROOT, "tests", "emu", "libruns_emu.so")
JEMU = os.path.join(ROOT, "tests", "emu", "librxset_runs_emu.so")
NEMU = os.path.join(ROOT, "tests", "emu", "liblaunch_emu.so")
UEMU = os.path.join(ROOT, "tests", "emu", "libout_lists_emu.so")
VEMU = os.path.join(ROOT, "tests", "emu", "libout_view_emu.so")
MODEL = os.path.join(ROOT, "tests", "emu", "libnanorq_model.so")
ROWS = os.path.join(ROOT, "tests", "gpu", "librows_probe.so")

HIP_SOURCES = ["nrq_device.hip"]
CXX_SOURCES = ["planner_host.cpp"]
C_SOURCES = ["nanorq_api.c", "io.c"]


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found: the HIP extension cannot be built (no CPU fallback exists)")


def _newer(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps if os.path.exists(d))


def _deps():
    out = []
    for d in (CSRC, os.path.join(ROOT, "include")):
        for f in os.listdir(d):
            out.append(os.path.join(d, f))
    return out


def build_lib(force=False, verbose=False, out=None, extra=(), host_extra=(), reuse_hip_obj=False):
    """Build libnanorq_hip.so.  `out`/`extra` build a tuning variant (other file, extra compiler flags) that
    NANORQ_HIP_LIB=<path> makes the binding load instead -- for A/B runs on the GPU box.  `host_extra`: flags for the C / C++
    host sources only (gcc / g++: the sanitizer builds of tools/sanitize.sh); `reuse_hip_obj`: take the kernels' object of the
    regular build instead of compiling nrq_device.hip again."""
    if out is None and not force and not _newer(LIB, _deps()):
        return LIB
    hipcc = _hipcc()
    objdir = os.path.join(HERE, "build" if out is None else "build_" + os.path.basename(out))
    os.makedirs(objdir, exist_ok=True)
    objs = []
    common = ["-O3", "-fPIC", "-Wno-pass-failed", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
    common += list(extra)
    # an object is rebuilt when its source or any header is newer than it (the .hip takes ~100 s, the rest seconds)
    headers = [f for f in _deps() if f.endswith(".h")]

    def stale(o, src):
        return force or out is not None or _newer(o, [src] + headers)

    for s in HIP_SOURCES:
        o = os.path.join(objdir, s + ".o")
        if reuse_hip_obj and os.path.exists(os.path.join(HERE, "build", s + ".o")):
            objs.append(os.path.join(HERE, "build", s + ".o"))
            continue
        if stale(o, os.path.join(CSRC, s)):
            subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", *common, "-c", os.path.join(CSRC, s), "-o", o],
                           check=True)
        objs.append(o)
    for s in CXX_SOURCES:
        o = os.path.join(objdir, s + ".o")
        if stale(o, os.path.join(CSRC, s)):
            subprocess.run(["g++", "-std=c++17", "-Wall", *common, *host_extra, "-c", os.path.join(CSRC, s), "-o", o], check=True)
        objs.append(o)
    for s in C_SOURCES:
        src = os.path.join(CSRC, s)
        if not os.path.exists(src):
            continue
        o = os.path.join(objdir, s + ".o")
        if stale(o, src):
            subprocess.run(["gcc", "-std=gnu11", "-Wall", "-D_FILE_OFFSET_BITS=64", *common, *host_extra, "-c", src, "-o", o], check=True)
        objs.append(o)
    target = out or LIB
    subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", target, *objs, "-lpthread"], check=True)
    if verbose:
        print("built", target)
    return target


def build_tools(force=False):
    """tools/rqfile: the file encoder / decoder on the object API (C, linked against the library in place)."""
    src = os.path.join(ROOT, "tools", "rqfile.c")
    exe = os.path.join(ROOT, "tools", "rqfile")
    deps = [src, LIB] + [os.path.join(ROOT, "include", h) for h in ("nanorq.h", "nanorq_batch.h", "io.h")]
    if force or _newer(exe, deps):
        subprocess.run(["gcc", "-std=c99", "-D_DEFAULT_SOURCE", "-D_FILE_OFFSET_BITS=64", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"),
                        src, "-o", exe, "-L" + os.path.dirname(LIB), "-lnanorq_hip", "-Wl,-rpath,$ORIGIN/../nanorq_amd", "-lm"], check=True)
    return exe


def _build_emu(target, src, headers, force):
    """one CPU emulation library: a g++ build of `src` over the kernel bodies it includes (`headers`, in csrc)"""
    if force or _newer(target, [src] + [os.path.join(CSRC, h) for h in headers]):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fPIC", "-shared", "-o", target, src], check=True)
    return target


def build_emu(force=False):
    return _build_emu(EMU, os.path.join(ROOT, "tests", "emu", "solve_emu.cpp"),
                      ("solve_body.h", "solve_roles.h", "split_body.h", "plan.h", "rq_math.h", os.path.join(ROOT, "tests", "emu", "strip_emu.h")), force)


def build_launch_emu(force=False):
    """tests/emu/liblaunch_emu.so: a whole solve launch on the CPU -- the shape launch_shape.h decides, every workgroup's work slots,
    movers and staging sets as nrq_solve_kernel runs them -- on arrays between pages nobody may touch (tests/emu/launch_emu.cpp)."""
    return _build_emu(NEMU, os.path.join(ROOT, "tests", "emu", "launch_emu.cpp"),
                      ("launch_shape.h", "planner_body.h", "solve_body.h", "solve_roles.h", "split_body.h", "plan.h", "rq_math.h", "rfc6330_tables.h",
                       os.path.join(ROOT, "tests", "emu", "strip_emu.h"), os.path.join(ROOT, "tests", "emu", "wave_emu.h")), force)


def build_planner_emu(force=False):
    return _build_emu(PEMU, os.path.join(ROOT, "tests", "emu", "planner_emu.cpp"),
                      ("planner_body.h", "planner_seq.h", "solve_body.h", "plan.h", "rq_math.h"), force)


def build_out_lists_emu(force=False):
    """tests/emu/libout_lists_emu.so: the host's builder of a job's output lists (out_lists.h) behind a C interface; host code as
    it is, no emulation."""
    return _build_emu(UEMU, os.path.join(ROOT, "tests", "emu", "out_lists_emu.cpp"), ("out_lists.h", "rq_math.h"), force)


def build_out_view_emu(force=False):
    """tests/emu/libout_view_emu.so: the host's builder of the out view's image (out_lists.h build_out_w) behind a C interface;
    host code as it is, no emulation."""
    return _build_emu(VEMU, os.path.join(ROOT, "tests", "emu", "out_view_emu.cpp"), ("out_lists.h", "plan.h", "rq_math.h"), force)


def build_ingest_emu(force=False):
    """tests/emu/libingest_emu.so: CPU emulation of the device-resident receiver's ingest kernels (ingest_body.h)."""
    return _build_emu(IEMU, os.path.join(ROOT, "tests", "emu", "ingest_emu.cpp"), ("ingest_body.h",), force)


def build_emit_emu(force=False):
    """tests/emu/libemit_emu.so: CPU emulation of the device-resident emit kernel (csrc/emit_emu.cpp over emit_body.h)."""
    return _build_emu(XEMU, os.path.join(CSRC, "emit_emu.cpp"), ("emit_emu.h", "emit_body.h", "rq_math.h"), force)


def build_held_emu(force=False):
    """tests/emu/libheld_emu.so: CPU emulation of the held-symbol emit and of the held listing (csrc/held_emu.cpp over emit_body.h
    and held_body.h)."""
    return _build_emu(HEMU, os.path.join(CSRC, "held_emu.cpp"), ("emit_emu.h", "emit_body.h", "held_body.h", "ingest_body.h", "rq_math.h"), force)


def build_want_emu(force=False):
    """tests/emu/libwant_emu.so: CPU emulation of the listing of what a reception wants (csrc/want_emu.cpp over want_body.h)."""
    return _build_emu(WEMU, os.path.join(CSRC, "want_emu.cpp"), ("want_body.h", "held_body.h", "ingest_body.h"), force)


def build_rxset_emu(force=False):
    """tests/emu/librxset_emu.so: CPU emulation of a reception set's ingest (csrc/rxset_emu.cpp over ingest_set_body.h)."""
    return _build_emu(REMU, os.path.join(CSRC, "rxset_emu.cpp"), ("ingest_set_body.h", "ingest_body.h"), force)


def build_rxset_lists_emu(force=False):
    """tests/emu/librxset_lists_emu.so: CPU emulation of a reception set's listing passes and the grouping of its decode
    (csrc/rxset_lists_emu.cpp over lists_set_body.h and rxset_plan.h)."""
    return _build_emu(LEMU, os.path.join(CSRC, "rxset_lists_emu.cpp"),
                      ("lists_set_body.h", "rxset_plan.h", "ingest_set_body.h", "ingest_body.h"), force)


def build_rxset_want_emu(force=False):
    """tests/emu/librxset_want_emu.so: CPU emulation of a reception set's want and held listings with keys
    (csrc/rxset_want_emu.cpp over want_set_body.h)."""
    return _build_emu(QEMU, os.path.join(CSRC, "rxset_want_emu.cpp"),
                      ("emu_scan.h", "want_set_body.h", "lists_set_body.h", "want_body.h", "held_body.h", "ingest_set_body.h", "ingest_body.h"), force)


def build_txset_emu(force=False):
    """tests/emu/libtxset_emu.so: CPU emulation of a sender set's emit (csrc/txset_emu.cpp over emit_set_body.h)."""
    return _build_emu(TEMU, os.path.join(CSRC, "txset_emu.cpp"), ("emit_set_body.h", "emit_body.h", "rq_math.h"), force)


def build_txset_range_emu(force=False):
    """tests/emu/libtxset_range_emu.so: CPU emulation of the map pass of a sender set's range mode (csrc/txset_range_emu.cpp over
    emit_set_range_body.h)."""
    return _build_emu(KEMU, os.path.join(CSRC, "txset_range_emu.cpp"), ("emit_set_range_body.h", "emit_set_body.h", "emit_body.h", "rq_math.h"), force)


def build_syms_emu(force=False):
    """tests/emu/libsyms_emu.so: CPU emulation of the emit and ingest of packets of several symbols (csrc/syms_emu.cpp over
    syms_body.h), with the count rule, the range packetisation and the path rules behind C entry points."""
    return _build_emu(YEMU, os.path.join(CSRC, "syms_emu.cpp"), ("emit_emu.h", "syms_body.h", "emit_body.h", "ingest_body.h", "rq_math.h"), force)


def build_syms_set_emu(force=False):
    """tests/emu/libsyms_set_emu.so: CPU emulation of a reception set's ingest and a sender set's emit of packets of several
    symbols (csrc/syms_set_emu.cpp over syms_set_body.h), with the set's path and word rules behind C entry points."""
    return _build_emu(ZEMU, os.path.join(CSRC, "syms_set_emu.cpp"),
                      ("syms_set_body.h", "syms_body.h", "ingest_set_body.h", "emit_set_body.h", "emit_body.h", "ingest_body.h", "rq_math.h"), force)


def build_runs_emu(force=False):
    """tests/emu/libruns_emu.so: CPU emulation of the want and held listings as runs and of the held emit of packets of several
    symbols (csrc/runs_emu.cpp over runs_body.h)."""
    return _build_emu(GEMU, os.path.join(CSRC, "runs_emu.cpp"),
                      ("emit_emu.h", "runs_emu_walks.h", "runs_body.h", "syms_body.h", "want_body.h", "held_body.h", "emit_body.h", "ingest_body.h",
                       "rq_math.h"), force)


def build_rxset_runs_emu(force=False):
    """tests/emu/librxset_runs_emu.so: CPU emulation of a reception set's want and held listings as runs and of a sender set's
    held emit of packets of several symbols (csrc/rxset_runs_emu.cpp over runs_set_body.h)."""
    return _build_emu(JEMU, os.path.join(CSRC, "rxset_runs_emu.cpp"),
                      ("emu_scan.h", "runs_emu_walks.h", "runs_set_body.h", "runs_body.h", "syms_set_body.h", "want_set_body.h", "lists_set_body.h",
                       "syms_body.h", "want_body.h", "held_body.h", "emit_set_body.h", "emit_body.h", "ingest_set_body.h", "ingest_body.h", "rq_math.h"), force)


def build_obj_emu(force=False):
    """tests/emu/libobj_emu.so: CPU emulation of the device-resident object layout kernel (obj_body.h)."""
    return _build_emu(OEMU, os.path.join(ROOT, "tests", "emu", "obj_emu.cpp"), ("obj_body.h", "emit_body.h", "rq_math.h"), force)


def build_shape_emu(force=False):
    """tests/emu/libshape_emu.so: the launch decisions (launch_shape.h) behind a C interface; host code as it is, no emulation."""
    return _build_emu(SEMU, os.path.join(ROOT, "tests", "emu", "shape_emu.cpp"),
                      ("launch_shape.h", "planner_body.h", "solve_body.h", "solve_roles.h", "plan.h", "rq_math.h", "rfc6330_tables.h"), force)


def build_model_lib(force=False, out=None, sanitize=False):
    """tests/emu/libnanorq_model.so: the host layer of the library -- the host-only object of nrq_device.hip, with every launch
    turned into a call of the model by the force-included tests/emu/hip_model.h, planner_host.cpp, nanorq_api.c, io.c -- linked
    with the model runtime tests/emu/hip_model.cpp (and the effects of the library's own kernels, tests/emu/model_effects.cpp)
    instead of the HIP runtime.  Kernels do not run in it.  `out` + `sanitize`: another file, every source compiled by the
    clang that hipcc drives with -fsanitize=address,undefined (host code only: there is no device code in this library)."""
    emu = os.path.join(ROOT, "tests", "emu")
    hook, model, effects = os.path.join(emu, "hip_model.h"), os.path.join(emu, "hip_model.cpp"), os.path.join(emu, "model_effects.cpp")
    target = out or MODEL
    if not force and not _newer(target, _deps() + [hook, model, effects]):
        return target
    hipcc = _hipcc()
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    objdir = os.path.join(HERE, "build_model" if out is None else "build_" + os.path.basename(out))
    os.makedirs(objdir, exist_ok=True)
    common = ["-O2", "-g1", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I" + emu]
    cc, cxx, san, hip_san = "gcc", "g++", [], []
    if sanitize:
        llvm = os.path.join(rocm, "lib", "llvm", "bin")
        cc, cxx = os.path.join(llvm, "clang"), os.path.join(llvm, "clang++")
        san = ["-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
        hip_san = [x for f in san for x in ("-Xarch_host", f)]
    objs = []

    def obj(cmd, src, name):
        o = os.path.join(objdir, name + ".o")
        subprocess.run([*cmd, *common, "-c", src, "-o", o], check=True)
        objs.append(o)
        return o

    dev = obj([hipcc, "--offload-host-only", "-std=c++17", "-Wno-pass-failed", "-DNRQ_HIP_MODEL_HOOK", "-include", hook, *hip_san],
              os.path.join(CSRC, HIP_SOURCES[0]), HIP_SOURCES[0])
    for s in CXX_SOURCES:
        obj([cxx, "-std=c++17", "-Wall", *san], os.path.join(CSRC, s), s)
    for s in C_SOURCES:
        obj([cc, "-std=gnu11", "-Wall", "-D_FILE_OFFSET_BITS=64", *san], os.path.join(CSRC, s), s)
    # (plain C++ over the runtime's own prototypes: the headers that ship next to the compiler)
    obj([cxx, "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), *san], model, "hip_model.cpp")
    # the library's own kernels' effects.  (UBSan only in a sanitizer build: with AddressSanitizer's global instrumentation the
    # runtime refuses this object's string literals at load time as "not properly aligned", before main runs; the file is test
    # support on top of the model, not host-layer code)
    obj([cxx, "-std=c++17", "-Wall", "-Wno-unknown-pragmas", *[f for f in san if f != "-fsanitize=address,undefined"],
         *(["-fsanitize=undefined"] if sanitize else [])], effects, "model_effects.cpp")
    # the host-only object still names the device code's image; nobody reads it here: the symbol gets a value at link time
    undefined = subprocess.run(["nm", "-u", dev], check=True, stdout=subprocess.PIPE).stdout.decode().split()
    defs = ["-Wl,--defsym=%s=0" % n for n in undefined if n.startswith("__hip_fatbin")]
    subprocess.run([cxx, "-shared", "-fPIC", *san, "-o", target, *objs, *defs, "-lpthread", "-ldl"], check=True)
    return target


def build_rows_probe(force=False):
    """tests/gpu/librows_probe.so: tests/gpu/rows_probe.hip, the device-only row pipelines of solve_body.h (fwd_rows and its half /
    third forms, rev_rows, fwd_rows_wide) and its address helpers in kernels that run them on images of the caller's.  A library
    of its own, so that libnanorq_hip.so holds no kernel it does not ship; cross-compiles without a GPU."""
    src = os.path.join(ROOT, "tests", "gpu", "rows_probe.hip")
    if force or _newer(ROWS, [src, os.path.join(CSRC, "solve_body.h"), os.path.join(CSRC, "solve_roles.h"), os.path.join(CSRC, "plan.h")]):
        subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + CSRC, "-shared", "-fPIC", src, "-o", ROWS], check=True)
    return ROWS


def build_model_exercise(force=False, sanitize=True):
    """tests/emu/model_exercise(_asan): tests/emu/model_exercise.cpp, a program of its own over the model library -- with
    `sanitize` over tests/emu/libnanorq_model_asan.so, host layer, model and program under AddressSanitizer / UBSan.  Run it
    directly: a sanitizer report or a failed check makes its exit status non-zero."""
    emu = os.path.join(ROOT, "tests", "emu")
    src = os.path.join(emu, "model_exercise.cpp")
    exe = os.path.join(emu, "model_exercise_asan" if sanitize else "model_exercise")
    lib = build_model_lib(force=force, out=os.path.join(emu, "libnanorq_model_asan.so") if sanitize else None, sanitize=sanitize)
    if force or _newer(exe, [src, lib]):
        cxx, san = "g++", []
        if sanitize:
            cxx = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(_hipcc()))), "lib", "llvm", "bin", "clang++")
            san = ["-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
        subprocess.run([cxx, "-std=c++17", "-Wall", "-g1", *san, "-I" + os.path.join(ROOT, "include"), "-I" + emu, src, "-o", exe,
                        "-L" + emu, "-l:" + os.path.basename(lib), "-Wl,-rpath,$ORIGIN", "-lpthread"], check=True)
    return exe


if __name__ == "__main__":
    build_lib(force="-f" in sys.argv, verbose=True)
    build_emu(force="-f" in sys.argv)
    build_planner_emu(force="-f" in sys.argv)
    build_ingest_emu(force="-f" in sys.argv)
    build_emit_emu(force="-f" in sys.argv)
    build_held_emu(force="-f" in sys.argv)
    build_want_emu(force="-f" in sys.argv)
    build_rxset_emu(force="-f" in sys.argv)
    build_rxset_lists_emu(force="-f" in sys.argv)
    build_rxset_want_emu(force="-f" in sys.argv)
    build_txset_emu(force="-f" in sys.argv)
    build_txset_range_emu(force="-f" in sys.argv)
    build_syms_emu(force="-f" in sys.argv)
    build_syms_set_emu(force="-f" in sys.argv)
    build_runs_emu(force="-f" in sys.argv)
    build_rxset_runs_emu(force="-f" in sys.argv)
    build_obj_emu(force="-f" in sys.argv)
    build_shape_emu(force="-f" in sys.argv)
    build_launch_emu(force="-f" in sys.argv)
    build_out_lists_emu(force="-f" in sys.argv)
    build_out_view_emu(force="-f" in sys.argv)
    build_model_lib(force="-f" in sys.argv)
    build_rows_probe(force="-f" in sys.argv)
    build_tools(force="-f" in sys.argv)
