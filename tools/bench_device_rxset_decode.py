"""A reception set decoded in one call (nrq_rxset_decode) against the per-member decode loop it replaces.  HIP-event time from
"packets ingested" (the stream idle) to "last solve and marking complete", median of --reps per process, every rep on fresh
receivers fed by one ReceiverSet.add (not timed).
  shape 1   64 receptions x 4 blocks of K = 1000, T = 1280, a tenth of the source symbols lost, two spare repair symbols: the
            many-small-members case, where the member loop is 64 host-planned calls of four blocks
  shape 2   8 objects x 32 blocks of K = 8192, T = 1280, a tenth of the source symbols lost, 911 repair symbols per block (the
            decode takes two beyond the gaps up front): comparison (b) of tools/bench_device_rxset.py, decoded
  route set       ReceiverSet.decode()
  route members   decode() member by member (Receiver.decode / ObjectReceiver.decode)
One process measures one route and prints one JSON line:
    python tools/bench_device_rxset_decode.py --route set|members [--shape 1|2|both] [--reps 10]
The comparison alternates fresh processes, route `set` on this library and route `members` on the library --parent-lib names (a
build of the parent commit; NANORQ_HIP_LIB in the child), plus route `members` on this library as a cross-check, --procs each:
    python tools/bench_device_rxset_decode.py --ab --parent-lib PATH [--procs 2]
and prints a summary line: the medians per process, route members' spread across its processes (the margin), the ratios."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT]

ap = argparse.ArgumentParser()
ap.add_argument("--route", choices=("set", "members"), default="set")
ap.add_argument("--shape", choices=("1", "2", "both"), default="both")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--ab", action="store_true")
ap.add_argument("--parent-lib")
ap.add_argument("--procs", type=int, default=2)
a = ap.parse_args()


def ab():
    """alternate the routes process by process (fresh children; this process never opens the GPU)"""
    runs = {"set": [], "members_parent": [], "members_here": []}
    plan = [("set", None), ("members_parent", a.parent_lib), ("members_here", None)] * a.procs
    for name, lib in plan:
        env = dict(os.environ)
        env.pop("NANORQ_HIP_LIB", None)
        if lib:
            env["NANORQ_HIP_LIB"] = os.path.abspath(lib)
        cmd = [sys.executable, os.path.abspath(__file__), "--route", "set" if name == "set" else "members", "--shape", a.shape, "--reps", str(a.reps)]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit("a %s process ended with %d: nothing further is started" % (name, r.returncode))
        line = [x for x in r.stdout.splitlines() if x.startswith("{")][-1]
        print(name, line, flush=True)
        runs[name].append(json.loads(line))
    out = {"tool": "bench_device_rxset_decode", "mode": "ab", "procs": a.procs, "reps": a.reps}
    for s in ("shape1", "shape2"):
        k = s + "_ms_median"
        if k not in runs["set"][0]:
            continue
        med = {n: [r[k] for r in v] for n, v in runs.items()}
        out[s] = {n + "_ms": v for n, v in med.items()}
        out[s]["members_parent_spread_ms"] = round(max(med["members_parent"]) - min(med["members_parent"]), 3)
        out[s]["set_over_members_parent"] = round(max(med["set"]) / min(med["members_parent"]), 4)   # (the least favourable pairing)
        out[s]["members_here_over_parent"] = round(sum(med["members_here"]) / sum(med["members_parent"]), 4)
    print(json.dumps(out))


if a.ab:
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        raise SystemExit("--ab needs --parent-lib: a libnanorq_hip.so built from the parent commit")
    ab()
    raise SystemExit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: torch's HIP runtime must find the device first)

torch.cuda.init()
torch.empty(1, device="cuda")
import nanorq_amd  # noqa: E402

T = 1280
ctx = nanorq_amd.Context(0)
res = {"tool": "bench_device_rxset_decode", "route": a.route, "lib": os.path.basename(nanorq_amd.lib_path()), "T": T, "reps": a.reps}
g = torch.Generator(device="cuda").manual_seed(1)
rng = np.random.default_rng(1)


def timed(fn):
    torch.cuda.synchronize()
    ctx.sync()
    ctx.timer_start()
    out = fn()
    return ctx.timer_stop_ms(), out


def measure(key, fresh, pk, keys):
    """fresh() -> (set, members, data check); one add, then the timed decode of the route"""
    ts = []
    for _ in range(a.reps):
        st, members, check = fresh()
        st.add(pk, keys=keys, inline=True)
        if a.route == "set":
            ms, (status, _) = timed(st.decode)
        else:
            ms, parts = timed(lambda: [m.decode()[0] for m in members])
            status = np.concatenate(parts)
        assert status.all(), "%d of %d blocks were not recovered" % (int((status == 0).sum()), len(status))
        check(members)
        ts.append(ms)
        st.close()
        for m in members:
            m.close()
    res[key + "_ms_median"] = round(float(np.median(ts)), 3)
    res[key + "_ms_min"] = round(float(min(ts)), 3)
    res[key + "_ms_max"] = round(float(max(ts)), 3)


if a.shape in ("1", "both"):
    K, R, NB = 1000, 64, 4
    src = torch.randint(0, 256, (R * NB, K, T), dtype=torch.uint8, device="cuda", generator=g)
    tags = []
    for b in range(R * NB):
        lost = rng.choice(K, K // 10, replace=False)
        keep = np.setdiff1d(np.arange(K), lost)
        tags.append((b << 24) | np.concatenate([keep, K + np.arange(len(lost) + 2)]))
    tags = np.concatenate(tags).astype(np.uint32)
    tags = tags[rng.permutation(len(tags))]
    t_d = torch.from_numpy(tags.view(np.int32)).cuda()
    keys1 = torch.from_numpy(((tags >> 24) // NB).astype(np.int32)).cuda()   # reception i under key i, SBNs 4i .. 4i+3
    torch.cuda.synchronize()
    with nanorq_amd.Sender(ctx, K, T, R * NB, src) as tx:
        tx.encode()
        pk1 = tx.emit(t_d, inline=True)
        ctx.sync()
    res["shape1_packets"] = int(pk1.shape[0])

    def fresh1():
        st = nanorq_amd.ReceiverSet(ctx, T)
        mem = [nanorq_amd.Receiver(ctx, K, T, NB, K // 10 + 2, sbn0=NB * i) for i in range(R)]
        for i, m in enumerate(mem):
            st.attach(i, m)

        def check(mem):
            ctx.sync()
            assert torch.equal(mem[R - 1].source, src[NB * (R - 1):]), "the last reception's rows are not the data"
        return st, mem, check
    measure("shape1", fresh1, pk1, keys1)
    del src, pk1

if a.shape in ("2", "both"):
    K, NOBJ, ZB, NREP = 8192, 8, 32, 911
    bufs, otis, last = [], [], None
    for i in range(NOBJ):
        ob = torch.randint(0, 256, (ZB * K * T,), dtype=torch.uint8, device="cuda", generator=g)
        torch.cuda.synchronize()
        with nanorq_amd.ObjectSender(ctx, ob, T, Z=ZB) as tx:
            tx.encode()
            p = tx.emit_all(NREP, interleave=False, inline=True)   # block-major: packet k is ESI k % (K + NREP)
            ctx.sync()
            otis.append(tx.oti)
        esi = torch.arange(p.shape[0], device="cuda") % (K + NREP)
        keep = (esi >= K) | (torch.rand(p.shape[0], device="cuda", generator=g) >= 0.10)
        bufs.append(p[keep])
        last = ob
    per = [int(b.shape[0]) for b in bufs]
    keys2 = torch.cat([torch.full((n,), i, dtype=torch.int32, device="cuda") for i, n in enumerate(per)])
    perm = torch.randperm(sum(per), device="cuda", generator=g)
    pk2 = torch.cat(bufs)[perm].contiguous()
    keys2 = keys2[perm].contiguous()
    del bufs
    torch.cuda.synchronize()
    res["shape2_packets"] = int(pk2.shape[0])

    def fresh2():
        st = nanorq_amd.ReceiverSet(ctx, T)
        mem = [nanorq_amd.ObjectReceiver(ctx, *o, rep_cap=NREP) for o in otis]
        for i, m in enumerate(mem):
            st.attach(i, m)

        def check(mem):
            out, left = mem[NOBJ - 1].write()
            ctx.sync()
            assert left == 0 and torch.equal(out, last), "the last object is not the data"
        return st, mem, check
    measure("shape2", fresh2, pk2, keys2)

print(json.dumps(res))
