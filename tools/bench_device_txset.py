"""Sender sets (nrq_txset_*) against what they replace.  One JSON line with best and median HIP-event times over --reps, the
routes of a comparison alternated rep by rep in one process:
  (1) many members: every source ESI plus 911 repair ESIs of every block, the packets interleaved over all members, each packet
      key | FEC Payload ID | payload at a stride of T + 8 rounded up to 16
        set_emit_<m>_ms       ONE SenderSet.emit(key_inline=True, inline=True)
        members_emit_<m>_ms   the route it replaces: one emit per member into a buffer of its own (behind the four key bytes,
                              so at a 4-byte alignment), the keys written with torch, torch.cat, the index by the interleaving
                              permutation
      <m> = obj8: 8 objects of 32 blocks of K = 8192 (2.33 M packets); tx64: 64 senders of 4 blocks of K = 1000.  The two
      routes' packets are compared byte for byte.
  (2) what the table costs: the 256 x 8192 transmission, the same interleaved tag list
        sender_emit_ms        Sender.emit, header inline
        set1_emit_ms          a one-member set, header inline, no key (the same bytes)
        set1_key_emit_ms      the same set with the key inline: the 16-byte form of the 8-byte header
    python tools/bench_device_txset.py [--reps 10] [--skip-1] [--skip-2]"""
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
ap.add_argument("--skip-1", action="store_true")
ap.add_argument("--skip-2", action="store_true")
a = ap.parse_args()
T, NREP = 1280, 911
KSTRIDE = (T + 8 + 15) // 16 * 16

ctx = nanorq_amd.Context(0)  # (the null stream, as torch's default: the events below bracket torch's work too)
res = {"tool": "bench_device_txset", "T": T, "reps": a.reps}
g = torch.Generator(device="cuda").manual_seed(1)


def timed(fn):
    torch.cuda.synchronize()
    ctx.sync()
    ctx.timer_start()
    fn()
    return ctx.timer_stop_ms()


def stats(key, ts):
    res[key] = round(float(min(ts)), 3)
    res[key + "_median"] = round(float(np.median(ts)), 3)
    res[key + "_spread"] = round(float(max(ts) - min(ts)), 3)


def member_tags(K, nblk):
    """ESIs 0 .. K + NREP - 1 of every block, sorted by (ESI, SBN)"""
    k = torch.arange((K + NREP) * nblk, device="cuda", dtype=torch.int64)
    return (((k % nblk) << 24) | (k // nblk)).to(torch.int32)


def many(label, nmem, K, nblk, make):
    """nmem members of nblk blocks of K under keys 0 .. nmem-1"""
    txs = []
    for i in range(nmem):
        src = torch.randint(0, 256, (nblk * K * T,), dtype=torch.uint8, device="cuda", generator=g)
        torch.cuda.synchronize()
        txs.append(make(src))
        txs[-1].encode()
        ctx.sync()
    st = nanorq_amd.SenderSet(ctx, T)
    for i, tx in enumerate(txs):
        st.attach(i, tx)
    mt = member_tags(K, nblk)
    per = int(mt.numel())
    n = per * nmem
    k = torch.arange(n, device="cuda", dtype=torch.int64)
    keys = (k % nmem).to(torch.int32)  # packet k: member k % nmem, its packet k // nmem
    tags = mt[k // nmem].contiguous()
    perm = ((k % nmem) * per + k // nmem)  # row of packet k in the members' buffers, one after the other
    out_a = torch.zeros((n, KSTRIDE), dtype=torch.uint8, device="cuda")
    bufs = [torch.zeros((per, KSTRIDE), dtype=torch.uint8, device="cuda") for _ in range(nmem)]
    keyb = [torch.tensor(list(int(i).to_bytes(4, "big")), dtype=torch.uint8, device="cuda") for i in range(nmem)]
    torch.cuda.synchronize()
    box = {}

    def route_a():
        st.emit(keys, tags, out=out_a, inline=True, key_inline=True)

    def route_b():
        for i, tx in enumerate(txs):
            tx.emit(mt, out=bufs[i][:, 4:], inline=True)
            bufs[i][:, :4] = keyb[i]
        box["b"] = torch.cat(bufs)[perm]

    t_a, t_b = [], []
    for _ in range(a.reps):
        t_a.append(timed(route_a))
        t_b.append(timed(route_b))
    torch.cuda.synchronize()
    assert torch.equal(out_a[:, :T + 8], box["b"][:, :T + 8]), "the two routes wrote different packets"
    res["packets_" + label] = n
    stats("set_emit_%s_ms" % label, t_a)
    stats("members_emit_%s_ms" % label, t_b)
    res["set_vs_members_" + label] = round(float(np.median(t_a) / np.median(t_b)), 3)
    st.close()
    for tx in txs:
        tx.close()


if not a.skip_1:
    many("obj8", 8, 8192, 32, lambda src: nanorq_amd.ObjectSender(ctx, src, T, Z=32))
    torch.cuda.empty_cache()
    many("tx64", 64, 1000, 4, lambda src: nanorq_amd.Sender(ctx, 1000, T, 4, src))
    torch.cuda.empty_cache()

if not a.skip_2:
    K, Z = 8192, 256
    src = torch.randint(0, 256, (Z * K * T,), dtype=torch.uint8, device="cuda", generator=g)
    torch.cuda.synchronize()
    tx = nanorq_amd.Sender(ctx, K, T, Z, src)
    tx.encode()
    ctx.sync()
    st = nanorq_amd.SenderSet(ctx, T)
    st.attach(0, tx)
    tags = member_tags(K, Z)
    n = int(tags.numel())
    keys = torch.zeros(n, dtype=torch.int32, device="cuda")
    out_s = torch.zeros((n, KSTRIDE), dtype=torch.uint8, device="cuda")
    out_1 = torch.zeros((n, KSTRIDE), dtype=torch.uint8, device="cuda")
    out_k = torch.zeros((n, KSTRIDE), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    t_s, t_1, t_k = [], [], []
    for _ in range(a.reps):
        t_s.append(timed(lambda: tx.emit(tags, out=out_s, inline=True)))
        t_1.append(timed(lambda: st.emit(None, tags, out=out_1, inline=True)))
        t_k.append(timed(lambda: st.emit(keys, tags, out=out_k, inline=True, key_inline=True)))
    torch.cuda.synchronize()
    assert torch.equal(out_s[:, :T + 4], out_1[:, :T + 4]) and torch.equal(out_s[:, :T + 4], out_k[:, 4:T + 8]), "the set wrote other bytes"
    res["packets_set1"] = n
    stats("sender_emit_ms", t_s)
    stats("set1_emit_ms", t_1)
    stats("set1_key_emit_ms", t_k)
    res["set1_vs_sender"] = round(float(np.median(t_1) / np.median(t_s)), 3)
    res["set1_key_vs_sender"] = round(float(np.median(t_k) / np.median(t_s)), 3)
    st.close()
    tx.close()

print(json.dumps(res))
