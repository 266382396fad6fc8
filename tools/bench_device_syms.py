"""Packets of several symbols (nrq_*_syms) against the route a caller had before them.  One JSON line with best and median
HIP-event times over --reps (after --warmup reps that the statistics leave out; the first one's time is reported as *_warm), the routes of
a comparison alternated rep by rep in one process.  64 blocks of K = 1024, ESIs 0 .. K + 10 % of every block, interleaved,
FEC Payload ID inline, at (T, G) = (64, 16), (256, 5), (1280, 1):
  emit_syms_ms      ONE Sender.emit_range_syms into packets of G symbols
  emit_repack_ms    the route it replaces: Sender.emit_range (one symbol per packet, tags apart) into [symbols, T], then a torch
                    gather by a prebuilt index into the G-symbol packets and the headers written with torch (the index and the
                    header bytes are built outside the timed region)
  add_syms_ms       ONE Receiver.add_syms of those packets (counts given)
  add_split_ms      the route it replaces: a torch gather of the packets' symbols into [symbols, T] by a prebuilt index, then
                    Receiver.add with a prebuilt tag list
  G = 1 only: emit_one_ms / add_one_ms, the one-symbol calls (emit_range inline, add inline) on the same work.
The two emit routes' packets are compared byte for byte, the two receptions' lists entry for entry.
    python tools/bench_device_syms.py [--reps 10] [--warmup 2]"""
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
K, NBLK = 1024, 64
NESI = K + (K + 9) // 10

ctx = nanorq_amd.Context(0)  # (the null stream, as torch's default: the events below bracket torch's work too)
res = {"tool": "bench_device_syms", "K": K, "nblk": NBLK, "esis_per_block": NESI, "reps": a.reps, "warmup": a.warmup}
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


def shape(T, G):
    lab = "T%d_G%d" % (T, G)
    src = torch.randint(0, 256, (NBLK, K, T), dtype=torch.uint8, device="cuda", generator=g)
    torch.cuda.synchronize()
    tx = nanorq_amd.Sender(ctx, K, T, NBLK, src)
    tx.encode()
    stride = tx.stride_syms(G, True)
    out_a, tg, ns = tx.emit_range_syms(0, NESI, G, interleave=True, inline=True)
    ctx.sync()
    npkt = int(tg.numel())
    # the repack route's prebuilt pieces: row of symbol i of packet p among the one-symbol packets (interleaved: ESI * nblk + block)
    tags = tg.to(torch.int64) & 0xFFFFFFFF
    blk, esi, cnt = tags >> 24, tags & 0xFFFFFF, ns.to(torch.int64)
    i = torch.arange(G, device="cuda", dtype=torch.int64)[None, :]
    idx = ((esi[:, None] + torch.minimum(i, cnt[:, None] - 1)) * NBLK + blk[:, None]).reshape(-1)
    valid = (i < cnt[:, None]).reshape(-1)
    hdr = torch.stack([(tags >> s) & 0xFF for s in (24, 16, 8, 0)], 1).to(torch.uint8)
    one = torch.zeros((NESI * NBLK, T), dtype=torch.uint8, device="cuda")
    out_b = torch.zeros((npkt, stride), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def emit_new():
        tx.emit_range_syms(0, NESI, G, interleave=True, inline=True, out=out_a)

    def emit_old():
        tx.emit_range(0, NESI, interleave=True, inline=False, out=one)
        ctx.sync()  # (the library's stream and torch's are not ordered: a caller of this route waits here too)
        out_b[:, 4:4 + G * T] = one[idx].view(npkt, G * T)
        out_b[:, :4] = hdr
        torch.cuda.synchronize()

    t_a, t_b = [], []
    for _ in range(a.warmup + a.reps):
        t_a.append(timed(emit_new))
        t_b.append(timed(emit_old))
    torch.cuda.synchronize()
    ctx.sync()
    keep = torch.zeros((npkt, stride), dtype=torch.bool, device="cuda")
    keep[:, :4] = True
    keep[:, 4:4 + G * T] = valid.view(npkt, G).repeat_interleave(T, 1)
    assert torch.equal(out_a[keep], out_b[keep]), "the two emit routes wrote different packets"
    res["packets_" + lab] = npkt
    stats("emit_syms_%s_ms" % lab, t_a)
    stats("emit_repack_%s_ms" % lab, t_b)
    res["emit_syms_vs_repack_" + lab] = round(float(np.median(t_a[a.warmup:]) / np.median(t_b[a.warmup:])), 3)

    # ingest
    rep_cap = NESI - K + 8
    rx_a = nanorq_amd.Receiver(ctx, K, T, NBLK, rep_cap)
    rx_b = nanorq_amd.Receiver(ctx, K, T, NBLK, rep_cap)
    sel = torch.nonzero(valid).flatten()
    p, s = sel // G, sel % G
    one_tags = ((blk[p] << 24) | (esi[p] + s)).to(torch.int32).contiguous()
    torch.cuda.synchronize()

    def add_new():
        rx_a.add_syms(out_a, G, nsym=ns, inline=True)

    def add_old():
        syms = out_a[:, 4:4 + G * T].reshape(npkt * G, T)[sel]
        torch.cuda.synchronize()
        rx_b.add(syms, tags=one_tags)

    t_a, t_b = [], []
    for _ in range(a.warmup + a.reps):
        rx_a.reset()
        rx_b.reset()
        t_a.append(timed(add_new))
        t_b.append(timed(add_old))
    la, lb = rx_a.lists(), rx_b.lists()
    assert all(np.array_equal(x, y) for x, y in zip(la[0] + la[1], lb[0] + lb[1])), "the two ingest routes left different books"
    stats("add_syms_%s_ms" % lab, t_a)
    stats("add_split_%s_ms" % lab, t_b)
    res["add_syms_vs_split_" + lab] = round(float(np.median(t_a[a.warmup:]) / np.median(t_b[a.warmup:])), 3)

    if G == 1:  # the new calls against the one-symbol calls themselves
        out_1 = torch.zeros((NESI * NBLK, stride), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        t_n, t_o, u_n, u_o = [], [], [], []
        for _ in range(a.warmup + a.reps):
            t_n.append(timed(emit_new))
            t_o.append(timed(lambda: tx.emit_range(0, NESI, interleave=True, inline=True, out=out_1)))
            rx_a.reset()
            rx_b.reset()
            u_n.append(timed(add_new))
            u_o.append(timed(lambda: rx_b.add(out_1, inline=True)))
        ctx.sync()
        assert torch.equal(out_1[:, :T + 4], out_a[:, :T + 4])
        stats("emit_syms_g1_ms", t_n)
        stats("emit_one_ms", t_o)
        stats("add_syms_g1_ms", u_n)
        stats("add_one_ms", u_o)
        res["emit_syms_vs_one"] = round(float(np.median(t_n[a.warmup:]) / np.median(t_o[a.warmup:])), 3)
        res["add_syms_vs_one"] = round(float(np.median(u_n[a.warmup:]) / np.median(u_o[a.warmup:])), 3)
    for h in (rx_a, rx_b, tx):
        h.close()
    torch.cuda.empty_cache()


for T, G in ((64, 16), (256, 5), (1280, 1)):
    shape(T, G)
print(json.dumps(res))
