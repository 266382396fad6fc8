"""Reception sets (nrq_rxset_*) against what they replace.  One JSON line with best and median HIP-event times over --reps, the
routes of a comparison alternated rep by rep in one process, every rep on fresh receivers:
  (a) the headline object, F = 256*8192*1280 - 128,077 bytes, T = 1280, Z = 256 (156 blocks of K=8192, 100 of K=8191), its own
      emit_all(911) packets (inline FEC Payload IDs):
        set_add_headline_ms   ReceiverSet.add with the object attached (one pass over a two-member table)
        orx_add_headline_ms   ObjectReceiver.add (a pass per block class and one for SBN >= Z)
        rx_add_ms             one-class Receiver.add of a 256 x 8192 object's packets (100 packets more): the figure the 1.25x
                              target of the two-class ingest refers to
  (b) 8 objects of 32 blocks of K = 8192 in one packet buffer, keys in a device array, packets in a random order:
        set_add_8_ms          one ReceiverSet.add
        split_add_8_ms        the packets split per object by torch indexing, then 8 ObjectReceiver.add calls (the split is timed:
                              without a set it is part of the ingest)
        split_only_8_ms       the 8 ObjectReceiver.add calls alone, on buffers split beforehand
    python tools/bench_device_rxset.py [--reps 10] [--skip-a] [--skip-b]"""
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
ap.add_argument("--skip-a", action="store_true")
ap.add_argument("--skip-b", action="store_true")
a = ap.parse_args()
T, Z, K, NREP = 1280, 256, 8192, 911
F = Z * K * T - 128077
STRIDE = (T + 4 + 15) // 16 * 16

ctx = nanorq_amd.Context(0)  # (the null stream, as torch's default: the events below bracket torch's indexing too)
res = {"tool": "bench_device_rxset", "T": T, "reps": a.reps}


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


g = torch.Generator(device="cuda").manual_seed(1)

if not a.skip_a:
    obj1 = torch.randint(0, 256, (Z * K * T,), dtype=torch.uint8, device="cuda", generator=g)
    torch.cuda.synchronize()
    with nanorq_amd.ObjectSender(ctx, obj1[:F].contiguous(), T, Z=Z) as htx:  # 156 x 8192 and 100 x 8191
        htx.encode()
        pk_h = htx.emit_all(NREP, interleave=True, inline=True)
        ctx.sync()
        oti_h = htx.oti
    with nanorq_amd.Sender(ctx, K, T, Z, obj1) as tx:  # one class
        tx.encode()
        pk_o = tx.emit_range(0, K + NREP, interleave=True, inline=True)
        ctx.sync()
    del obj1
    res["headline_packets"] = int(pk_h.shape[0])
    t_s, t_o, t_r = [], [], []
    for _ in range(a.reps):
        orx = nanorq_amd.ObjectReceiver(ctx, *oti_h, rep_cap=NREP)
        srx = nanorq_amd.ObjectReceiver(ctx, *oti_h, rep_cap=NREP)
        rx = nanorq_amd.Receiver(ctx, K, T, Z, NREP)
        st = nanorq_amd.ReceiverSet(ctx, T)
        st.attach(0, srx)
        t_s.append(timed(lambda: st.add(pk_h, inline=True)))
        t_o.append(timed(lambda: orx.add(pk_h, inline=True)))
        t_r.append(timed(lambda: rx.add(pk_o, inline=True)))
        for x, y in zip(srx.counts(), orx.counts()):
            assert np.array_equal(x, y), "the set and ObjectReceiver.add booked the packets differently"
        for h in (st, orx, srx, rx):
            h.close()
    stats("set_add_headline_ms", t_s)
    stats("orx_add_headline_ms", t_o)
    stats("rx_add_ms", t_r)
    res["set_vs_orx_headline"] = round(float(np.median(t_s) / np.median(t_o)), 3)
    res["set_vs_rx_add"] = round(float(np.median(t_s) / np.median(t_r)), 3)
    res["orx_vs_rx_add"] = round(float(np.median(t_o) / np.median(t_r)), 3)
    del pk_h, pk_o

if not a.skip_b:
    NOBJ, ZB = 8, 32
    bufs, otis = [], []
    for i in range(NOBJ):
        ob = torch.randint(0, 256, (ZB * K * T,), dtype=torch.uint8, device="cuda", generator=g)
        torch.cuda.synchronize()
        with nanorq_amd.ObjectSender(ctx, ob, T, Z=ZB) as tx:
            tx.encode()
            bufs.append(tx.emit_all(NREP, interleave=True, inline=True))
            ctx.sync()
            otis.append(tx.oti)
        del ob
    per = int(bufs[0].shape[0])
    perm = torch.randperm(NOBJ * per, device="cuda", generator=g)
    pk = torch.cat(bufs)[perm].contiguous()
    keys = (perm // per).to(torch.int32).contiguous()  # object i's packets carry key i
    del bufs
    torch.cuda.synchronize()
    res["objects"], res["packets_8"] = NOBJ, int(pk.shape[0])
    pre = [pk[torch.nonzero(keys == i).squeeze(1)].contiguous() for i in range(NOBJ)]
    torch.cuda.synchronize()
    t_s, t_p, t_q = [], [], []

    def split_add(rxs):
        for i, r in enumerate(rxs):
            r.add(pk[torch.nonzero(keys == i).squeeze(1)], inline=True)

    def pre_add(rxs):
        for r, p in zip(rxs, pre):
            r.add(p, inline=True)

    for _ in range(a.reps):
        groups = [[nanorq_amd.ObjectReceiver(ctx, *o, rep_cap=NREP) for o in otis] for _ in range(3)]
        st = nanorq_amd.ReceiverSet(ctx, T)
        for i, r in enumerate(groups[0]):
            st.attach(i, r)
        t_s.append(timed(lambda: st.add(pk, keys=keys, inline=True)))
        t_p.append(timed(lambda: split_add(groups[1])))
        t_q.append(timed(lambda: pre_add(groups[2])))
        for x, y, z in zip(*groups):
            assert np.array_equal(x.counts()[0], y.counts()[0]) and np.array_equal(x.counts()[1], z.counts()[1])
        st.close()
        for grp in groups:
            for r in grp:
                r.close()
    stats("set_add_8_ms", t_s)
    stats("split_add_8_ms", t_p)
    stats("split_only_8_ms", t_q)
    res["set_vs_split_8"] = round(float(np.median(t_s) / np.median(t_p)), 3)
    res["set_vs_split_only_8"] = round(float(np.median(t_s) / np.median(t_q)), 3)

print(json.dumps(res))
