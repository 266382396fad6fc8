"""The request of a whole reception set in PACKETS of several symbols (nrq_rxset_want_syms / nrq_rxset_held_syms:
ReceiverSet.want_syms / held_syms) and "forward what the relays hold" over a set (held_syms + SenderSet.emit_syms(held=True)),
against the routes they replace:
  (a) want: the members' own want_syms calls, torch.cat of their lists and a keys tensor (torch.full per member);
  (b) want: ReceiverSet.want / held and a torch coalescing pass over (keys, tags); forward: ReceiverSet.held,
      SenderSet.emit(held=True) into one-symbol packets and a torch repack into packets of G.
64 receptions x 4 blocks of K = 1000 after one ReceiverSet.add of nine tenths of their source symbols and of 40 repair symbols
per block (not timed), at T = 64 / G = 16 and T = 256 / G = 5, and at G = 1 (T = 64) against the one-symbol set calls themselves.
Wall-clock time around each route including its waits (each route ends with its result complete in device memory), median and
best of --reps after --warmup, the routes alternated rep by rep in ONE process, their results compared every rep.  Prints one
JSON line:
    python tools/bench_device_rxset_want_syms.py [--reps 10] [--warmup 2]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT]

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
a = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: torch's HIP runtime must find the device first)

torch.cuda.init()
torch.empty(1, device="cuda")
import nanorq_amd  # noqa: E402

K, R, NB, NREP = 1000, 64, 4, 40
ctx = nanorq_amd.Context(0)
res = {"tool": "bench_device_rxset_want_syms", "K": K, "receptions": R, "blocks_each": NB, "reps": a.reps, "warmup": a.warmup}
rng = np.random.default_rng(1)
g = torch.Generator(device="cuda").manual_seed(1)


def wall(fn):
    torch.cuda.synchronize()
    ctx.sync()
    t0 = time.perf_counter()
    fn()
    ctx.sync()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def coalesce(keys, t, G):
    """the torch pass over a one-symbol set listing: a run breaks where the tag is not the one before plus one, where the key
    changes and where the ESI reaches K (every member here has the same K) -> (keys, first tags, counts, index of each packet's
    first symbol in the list)"""
    n = t.numel()
    v = t.to(torch.int64) & 0xFFFFFFFF
    idx = torch.arange(n, device=t.device)
    brk = torch.ones(n, dtype=torch.bool, device=t.device)
    brk[1:] = (v[1:] != v[:-1] + 1) | (keys[1:] != keys[:-1]) | ((v[1:] & 0xFFFFFF) == K)
    start = torch.cummax(torch.where(brk, idx, torch.zeros_like(idx)), 0).values
    first = torch.nonzero((idx - start) % G == 0).flatten()
    nxt = torch.cat([first[1:], torch.tensor([n], device=t.device)])
    nxt_run = torch.cat([torch.nonzero(brk).flatten()[1:], torch.tensor([n], device=t.device)])
    run_end = nxt_run[torch.cumsum(brk.to(torch.int64), 0)[first] - 1]
    cnt = torch.minimum(nxt, run_end) - first
    return keys[first], t[first], cnt.to(torch.uint8), first


def rounds(lab, routes, same):
    """routes = {name: fn}, alternated; the first is the new call"""
    ts = {k: [] for k in routes}
    for _ in range(a.warmup + a.reps):
        for k, fn in routes.items():
            ts[k].append(wall(fn))
        assert same(), "%s: the routes disagree" % lab
    names = list(routes)
    for k in names:
        v = ts[k][a.warmup:]
        res["%s_%s_ms_median" % (lab, k)] = round(float(np.median(v)), 4)
        res["%s_%s_ms_best" % (lab, k)] = round(float(min(v)), 4)
    for k in names[1:]:
        res["%s_%s_over_%s" % (lab, k, names[0])] = round(float(np.median(ts[k][a.warmup:]) / np.median(ts[names[0]][a.warmup:])), 2)


def shape(T, G):
    lab = "T%d_G%d" % (T, G)
    st, sset = nanorq_amd.ReceiverSet(ctx, T), nanorq_amd.SenderSet(ctx, T)
    mem = [(i, nanorq_amd.Receiver(ctx, K, T, NB, K // 4, sbn0=NB * i)) for i in range(R)]
    for key, m in mem:
        st.attach(key, m)
    esis = np.arange(K + NREP, dtype=np.uint32)
    keys = np.repeat(np.arange(R, dtype=np.uint32), NB * len(esis))
    tags = ((np.arange(R * NB, dtype=np.uint32))[:, None] << 24 | esis[None, :]).ravel()
    keep = rng.permutation(np.flatnonzero(rng.random(len(tags)) >= 0.10))
    k_d = torch.from_numpy(keys[keep].view(np.int32)).cuda()
    t_d = torch.from_numpy(tags[keep].view(np.int32)).cuda()
    pl = torch.randint(0, 256, (len(keep), T), dtype=torch.uint8, device="cuda", generator=g)
    torch.cuda.synchronize()
    st.add(pl, keys=k_d, tags=t_d)
    ctx.sync()
    relays = [(key, m.relay()) for key, m in mem]
    for key, r in relays:
        sset.attach(key, r)
    box = {}

    def eq(x, y):
        return all(torch.equal(p, q) for p, q in zip(box[x], box[y]))

    for what, kw in (("want", dict(source=True)), ("want_rep", dict(extra=2))):
        def new():
            box["n"] = st.want_syms(G, **kw)

        def members():
            lists = [m.want_syms(G, **kw) for _, m in mem]
            ks = torch.cat([torch.full((int(t.numel()),), key, dtype=torch.int32, device="cuda") for (key, _), (t, _) in zip(mem, lists)])
            box["a"] = (ks, torch.cat([t for t, _ in lists]), torch.cat([c for _, c in lists]))

        def coalesced():
            ks, t = st.want(**kw)
            box["b"] = coalesce(ks, t, G)[:3]

        def one():
            box["b"] = st.want(**kw)
        if G == 1:
            rounds("%s_%s" % (what, lab), {"set_syms": new, "set_one_symbol": one, "members": members},
                   lambda: eq("n", "a") and torch.equal(box["n"][1], box["b"][1]))
        else:
            rounds("%s_%s" % (what, lab), {"set_syms": new, "members": members, "coalesce": coalesced}, lambda: eq("n", "a") and eq("n", "b"))
        res["%s_%s_packets" % (what, lab)] = int(box["n"][1].numel())
        res["%s_%s_symbols" % (what, lab)] = int(box["n"][2].sum())

    # forwarding what the relays hold (nothing is ready: every packet is copies of held rows)
    nh = int(st.held()[1].numel())
    stride = G * T
    out_a = torch.zeros((nh, stride), dtype=torch.uint8, device="cuda")
    out_b = torch.zeros((nh, stride), dtype=torch.uint8, device="cuda")
    one_sym = torch.zeros((nh, T), dtype=torch.uint8, device="cuda")
    lane = torch.arange(G, device="cuda", dtype=torch.int64)[None, :]
    torch.cuda.synchronize()

    def fwd_new():
        ks, t, c = st.held_syms(G)
        box["np"] = int(t.numel())
        sset.emit_syms(ks, t, G, nsym=c, out=out_a[:box["np"]], held=True)
        box["c"] = c

    def fwd_old():
        ks, t = st.held()
        sset.emit(ks, t, out=one_sym, held=True)
        if G == 1:
            return
        _, _, c, first = coalesce(ks, t, G)
        ctx.sync()  # (the library's stream and torch's are not ordered: a caller of this route waits here too)
        idx = first[:, None] + torch.minimum(lane, c.to(torch.int64)[:, None] - 1)
        out_b[:first.numel()] = one_sym[idx.reshape(-1)].view(first.numel(), stride)

    def fwd_same():
        if G == 1:
            return torch.equal(out_a, one_sym)
        n, c = box["np"], box["c"].to(torch.int64)
        valid = (lane < c[:, None]).repeat_interleave(T, 1)
        return torch.equal(out_a[:n][valid], out_b[:n][valid])
    rounds("fwd_" + lab, {"set_syms": fwd_new, "one_symbol" if G == 1 else "repack": fwd_old}, fwd_same)
    res["fwd_%s_packets" % lab] = box["np"]
    res["fwd_%s_symbols" % lab] = nh
    for h in [sset, st] + [r for _, r in relays] + [m for _, m in mem]:
        h.close()
    torch.cuda.empty_cache()


for T, G in ((64, 16), (256, 5), (64, 1)):
    shape(T, G)
print(json.dumps(res))
