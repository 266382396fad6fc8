"""The want and held listings in packets of several symbols (Receiver.want_syms / held_syms) and the held emit of such packets
(emit_syms(held=True) on a relay) against the routes a caller had before them.  One JSON line with best and median HIP-event times
over --reps (after --warmup reps that the statistics leave out; the first one's time is reported as *_warm), the routes of a
comparison alternated rep by rep in one process.  A relay tree's child: 64 blocks of K = 1024 that lost 10 % of their source
symbols, at (T, G) = (64, 16), (256, 5) and (1280, 1):
  want_syms_ms      ONE Receiver.want_syms(G, source=True): (first tags, counts) listed on the device
  want_coalesce_ms  the route it replaces: Receiver.want(source=True), then a torch pass that finds the runs of consecutive tags,
                    cuts them into packets of G and compacts first tags and counts
  want_rep_*        the same two routes in repair mode (extra = 2)
  fwd_syms_ms       forwarding what the relay holds: held_syms(G), then ONE relay.emit_syms(tags, G, nsym, held=True)
  fwd_repack_ms     the route it replaces: held(), relay.emit(tags, held=True) into [symbols, T], the same torch coalescing pass, then a
                    torch gather of the symbols into packets of G
  (1280, 1) only: want_syms_g1 / fwd_syms_g1 against want_one / fwd_one, the one-symbol calls themselves (want(source=True);
  held() + emit(held=True)) on the same work.
Each pair's results are compared: lists word for word, packets byte for byte.
    python tools/bench_device_want_syms.py [--reps 10] [--warmup 2]"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT]
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: torch's HIP runtime must find the device first)

torch.cuda.init()
torch.empty(1, device="cuda")
import nanorq_amd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
a = ap.parse_args()
K, NBLK, LOSS = 1024, 64, 0.1

ctx = nanorq_amd.Context(0)  # (the null stream, as torch's default: the events below bracket torch's work too)
res = {"tool": "bench_device_want_syms", "K": K, "nblk": NBLK, "loss": LOSS, "reps": a.reps, "warmup": a.warmup}
g = torch.Generator(device="cuda").manual_seed(1)


def timed(fn):
    torch.cuda.synchronize()
    ctx.sync()
    ctx.timer_start()
    fn()
    return ctx.timer_stop_ms()


def stats(key, ts):
    res[key + "_warm"] = round(float(ts[0]), 3)
    ts = ts[a.warmup:]
    res[key] = round(float(min(ts)), 3)
    res[key + "_median"] = round(float(np.median(ts)), 3)
    res[key + "_spread"] = round(float(max(ts) - min(ts)), 3)


def coalesce(t, G):
    """the torch pass over a one-symbol tag list (one side of K: source symbols only, or a want list in repair mode):
    -> (first tags, counts, index of each packet's first symbol in the list)"""
    n = t.numel()
    v = t.to(torch.int64) & 0xFFFFFFFF
    idx = torch.arange(n, device=t.device)
    brk = torch.ones(n, dtype=torch.bool, device=t.device)
    brk[1:] = v[1:] != v[:-1] + 1
    start = torch.cummax(torch.where(brk, idx, torch.zeros_like(idx)), 0).values
    first = torch.nonzero((idx - start) % G == 0).flatten()
    nxt = torch.cat([first[1:], torch.tensor([n], device=t.device)])
    nxt_run = torch.cat([torch.nonzero(brk).flatten()[1:], torch.tensor([n], device=t.device)])
    run_end = nxt_run[torch.cumsum(brk.to(torch.int64), 0)[first] - 1]
    cnt = torch.minimum(nxt, run_end) - first
    return t[first], cnt.to(torch.uint8), first


def pair(key_new, key_old, lab, new, old, same):
    t_a, t_b = [], []
    for _ in range(a.warmup + a.reps):
        t_a.append(timed(new))
        t_b.append(timed(old))
    torch.cuda.synchronize()
    ctx.sync()
    assert same(), "%s: the two routes disagree" % key_new
    stats("%s_%s_ms" % (key_new, lab), t_a)
    stats("%s_%s_ms" % (key_old, lab), t_b)
    res["%s_vs_%s_%s" % (key_new, key_old, lab)] = round(float(np.median(t_a[a.warmup:]) / np.median(t_b[a.warmup:])), 3)


def shape(T, G):
    lab = "T%d_G%d" % (T, G)
    src = torch.randint(0, 256, (NBLK, K, T), dtype=torch.uint8, device="cuda", generator=g)
    torch.cuda.synchronize()
    tx = nanorq_amd.Sender(ctx, K, T, NBLK, src)
    tx.encode()
    pk = tx.emit_range(0, K, interleave=True, inline=True)
    ctx.sync()
    keep = torch.nonzero(torch.rand(pk.shape[0], device="cuda", generator=g) >= LOSS).flatten()
    rx = nanorq_amd.Receiver(ctx, K, T, NBLK, K // 4)
    torch.cuda.synchronize()
    rx.add(pk[keep].contiguous(), inline=True)
    relay = rx.relay()
    box = {}

    if G == 1:  # the new calls against the one-symbol calls themselves: nothing to coalesce, nothing to repack
        nh = int(rx.held().numel())
        out_a = torch.zeros((nh, T), dtype=torch.uint8, device="cuda")
        out_b = torch.zeros((nh, T), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

        def want_new():
            box["a"] = rx.want_syms(1, source=True)[0]

        def want_one():
            box["b"] = rx.want(source=True)

        def fwd_new():
            t, c = rx.held_syms(1)
            relay.emit_syms(t, 1, nsym=c, out=out_a, held=True)

        def fwd_one():
            relay.emit(rx.held(), out=out_b, held=True)
        pair("want_syms", "want_one", "g1", want_new, want_one, lambda: torch.equal(box["a"], box["b"]))
        pair("fwd_syms", "fwd_one", "g1", fwd_new, fwd_one, lambda: torch.equal(out_a, out_b))
        res["fwd_symbols_g1"] = nh
        for h in (relay, rx, tx):
            h.close()
        torch.cuda.empty_cache()
        return

    for key, kw in (("want", dict(source=True)), ("want_rep", dict(extra=2))):
        def new():
            box["a"] = rx.want_syms(G, **kw)

        def old():
            t = rx.want(**kw)
            box["b"] = coalesce(t, G)[:2]
            torch.cuda.synchronize()
        pair(key + "_syms", key + "_coalesce", lab, new, old,
             lambda: torch.equal(box["a"][0], box["b"][0]) and torch.equal(box["a"][1], box["b"][1]))
        res["%s_packets_%s" % (key, lab)] = int(box["a"][0].numel())
        res["%s_symbols_%s" % (key, lab)] = int(box["a"][1].sum())

    # forwarding what the relay holds (nothing is ready: every packet is copies of held rows)
    nh = int(rx.held().numel())
    stride = G * T
    out_a = torch.zeros((nh, stride), dtype=torch.uint8, device="cuda")
    out_b = torch.zeros((nh, stride), dtype=torch.uint8, device="cuda")
    one = torch.zeros((nh, T), dtype=torch.uint8, device="cuda")
    lane = torch.arange(G, device="cuda", dtype=torch.int64)[None, :]
    torch.cuda.synchronize()

    def fwd_new():
        t, c = rx.held_syms(G)
        box["n"] = int(t.numel())
        relay.emit_syms(t, G, nsym=c, out=out_a[:box["n"]], held=True)
        box["c"] = c

    def fwd_old():
        t = rx.held()
        relay.emit(t, out=one, held=True)
        _, c, first = coalesce(t, G)
        ctx.sync()  # (the library's stream and torch's are not ordered: a caller of this route waits here too)
        idx = first[:, None] + torch.minimum(lane, c.to(torch.int64)[:, None] - 1)
        out_b[:first.numel()] = one[idx.reshape(-1)].view(first.numel(), stride)
        torch.cuda.synchronize()

    def same():
        n, c = box["n"], box["c"].to(torch.int64)
        valid = (lane < c[:, None]).repeat_interleave(T, 1)
        return torch.equal(out_a[:n][valid], out_b[:n][valid])
    pair("fwd_syms", "fwd_repack", lab, fwd_new, fwd_old, same)
    res["fwd_packets_" + lab] = box["n"]
    res["fwd_symbols_" + lab] = nh
    for h in (relay, rx, tx):
        h.close()
    torch.cuda.empty_cache()


for T, G in ((64, 16), (256, 5), (1280, 1)):
    shape(T, G)
print(json.dumps(res))
