"""The request of a whole reception set in one call (nrq_rxset_want / nrq_rxset_held: ReceiverSet.want / held) against the route it
replaces: want(extra=2) / held() member by member, the keys by torch.full per member, torch.cat of both.  Wall-clock time around
each route including its waits (each route ends with its lists complete in device memory), best and median of --reps, the two
routes alternated rep by rep in ONE process, their results compared byte for byte every rep.
  shape 1   64 receptions x 4 blocks of K = 1000: the many-small-members case, 64 blocking round trips against one
  shape 2   8 objects x 32 blocks of K = 8192: few members, long bitmaps (256 seen words per block and more)
Each shape after one ReceiverSet.add of every source symbol but a tenth, chosen at random (not timed).  The listings read the
books only, so the payload bytes are arbitrary and T is small (16).  Prints one JSON line:
    python tools/bench_device_rxset_want.py [--shape 1|2|both] [--reps 10]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT]

ap = argparse.ArgumentParser()
ap.add_argument("--shape", choices=("1", "2", "both"), default="both")
ap.add_argument("--reps", type=int, default=10)
a = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: torch's HIP runtime must find the device first)

torch.cuda.init()
torch.empty(1, device="cuda")
import nanorq_amd  # noqa: E402

T = 16
ctx = nanorq_amd.Context(0)
res = {"tool": "bench_device_rxset_want", "lib": os.path.basename(nanorq_amd.lib_path()), "T": T, "reps": a.reps}
rng = np.random.default_rng(1)
g = torch.Generator(device="cuda").manual_seed(1)


def wall(fn):
    torch.cuda.synchronize()
    ctx.sync()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()  # (the members' route ends with torch.full / torch.cat on torch's stream; the set's route has waited)
    return (time.perf_counter() - t0) * 1e3, out


def members_route(members, call):
    """the route a set-wide call replaces: the list of each member, its key repeated, both concatenated"""
    lists = [call(m) for _, m in members]
    keys = torch.cat([torch.full((int(t.numel()),), key, dtype=torch.int32, device="cuda") for (key, _), t in zip(members, lists)])
    return keys, torch.cat(lists)


def measure(name, st, members):
    """members = [(key, handle)] in block order"""
    for what, set_call, mem_call in (("want", lambda: st.want(extra=2), lambda m: m.want(extra=2)), ("held", lambda: st.held(), lambda m: m.held())):
        ts = {"set": [], "members": []}
        for rep in range(a.reps + 1):  # (the first rep warms both routes up and is not counted)
            ms_s, (k1, t1) = wall(set_call)
            ms_m, (k2, t2) = wall(lambda: members_route(members, mem_call))
            assert torch.equal(t1, t2) and torch.equal(k1, k2), "%s %s: the two routes differ" % (name, what)
            if rep:
                ts["set"].append(ms_s)
                ts["members"].append(ms_m)
        res["%s_%s_tags" % (name, what)] = int(t1.numel())
        for r, v in ts.items():
            res["%s_%s_%s_ms_best" % (name, what, r)] = round(min(v), 4)
            res["%s_%s_%s_ms_median" % (name, what, r)] = round(float(np.median(v)), 4)
        res["%s_%s_members_over_set_median" % (name, what)] = round(float(np.median(ts["members"]) / np.median(ts["set"])), 2)


def feed(st, nblocks_of_key, K):
    """every source symbol of every block but a tenth, shuffled, in one add (keys beside the packets)"""
    keys = np.concatenate([np.full(nb * K, key, np.uint32) for key, nb, _ in nblocks_of_key])
    tags = np.concatenate([((sbn0 + np.arange(nb, dtype=np.uint32))[:, None] << 24 | np.arange(K, dtype=np.uint32)[None, :]).ravel()
                           for _, nb, sbn0 in nblocks_of_key])
    keep = rng.permutation(np.flatnonzero(rng.random(len(tags)) >= 0.10))
    k_d = torch.from_numpy(keys[keep].view(np.int32)).cuda()
    t_d = torch.from_numpy(tags[keep].view(np.int32)).cuda()
    pl = torch.randint(0, 256, (len(keep), T), dtype=torch.uint8, device="cuda", generator=g)
    torch.cuda.synchronize()
    st.add(pl, keys=k_d, tags=t_d)
    ctx.sync()
    return int(len(keep))


if a.shape in ("1", "both"):
    K, R, NB = 1000, 64, 4
    st = nanorq_amd.ReceiverSet(ctx, T)
    mem = [(i, nanorq_amd.Receiver(ctx, K, T, NB, K // 10 + 2, sbn0=NB * i)) for i in range(R)]
    for key, m in mem:
        st.attach(key, m)
    res["shape1_packets"] = feed(st, [(i, NB, NB * i) for i in range(R)], K)
    measure("shape1", st, mem)
    st.close()
    for _, m in mem:
        m.close()

if a.shape in ("2", "both"):
    K, NOBJ, ZB = 8192, 8, 32
    ob = torch.zeros(ZB * K * T, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with nanorq_amd.ObjectSender(ctx, ob, T, Z=ZB) as tx:
        oti = tx.oti
        assert tx.blocks == [(K, tx.blocks[0][1])] * ZB
    st = nanorq_amd.ReceiverSet(ctx, T)
    mem = [(i, nanorq_amd.ObjectReceiver(ctx, *oti, rep_cap=K // 10 + 2)) for i in range(NOBJ)]
    for key, m in mem:
        st.attach(key, m)
    res["shape2_packets"] = feed(st, [(i, ZB, 0) for i in range(NOBJ)], K)
    measure("shape2", st, mem)
    st.close()
    for _, m in mem:
        m.close()

print(json.dumps(res))
