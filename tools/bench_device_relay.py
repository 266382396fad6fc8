"""Forwarding an object on the device: from "packets ingested" to "emit_all(911) written", at the headline object (F = 256*8192*1280
- 128,077 bytes, T = 1280, Z = 256: 156 blocks of K=8192, 100 of K=8191).  Two routes over the same reception:
  relay   ObjectReceiver.decode -> relay.encode (the blocks no decode made ready) -> relay.emit_all            (nrq_orx_relay)
  resend  ObjectReceiver.decode -> write -> ObjectSender over the written object -> encode -> emit_all         (no relay needed)
The reception: the origin's emit_all(920) packets, `--loss` of every block's packets dropped, the rest shuffled (--loss 0: exactly
the source packets, so that no block needs a decode).  One JSON line with, as best and median HIP-event times over --reps,
forward_ms (the whole route) and, from one more rep with a wait after each step, the steps' times.  The route "resend" uses no
call a library without relays lacks, so NANORQ_HIP_LIB=<an older build> runs it on that build (A/B, process by process).
Two more legs, each its own timing of single calls (best, median and all of --reps HIP-event times):
  ready   the object relay with every block ready: emit_all(--nrep), and the tag-list emit of the same packets in shuffled
          order.  Uses no call a library without held symbols lacks: NANORQ_HIP_LIB=<the parent's build> runs it there (A B A B).
  held    a flat reception of --blocks x K before any decode (no block ready): the held emit (NRQ_TX_HELD) of everything the
          reception holds (Receiver.held()), against Sender.emit of the same tag list over the original blocks (the same bytes
          moved; there a repair packet costs its LT gathers); the repair row lookup's share, from the same list with every
          repair tag replaced by a held source tag of its block; and what cut-through buys: "a batch (--batch of the reception)
          ingested -> its packets forwarded" the held way (the add and the emit enqueued back to back, one interval over both, and
          each alone after a wait), against "everything ingested -> decode -> the same packets forwarded".
    python tools/bench_device_relay.py --route relay|resend|ready|held [--loss 0.1] [--reps 10] [--nrep 911] [--N 1] [--no-check]"""
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
ap.add_argument("--route", choices=("relay", "resend", "ready", "held"), required=True)
ap.add_argument("--batch", type=float, default=0.125, help="route held: the share of the reception that makes the first batch")
ap.add_argument("--loss", type=float, default=0.1)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--nrep", type=int, default=911)
ap.add_argument("--N", type=int, default=1)
ap.add_argument("--blocks", type=int, default=256)
ap.add_argument("--K", type=int, default=8192)
ap.add_argument("--T", type=int, default=1280)
ap.add_argument("--no-check", action="store_true", help="do not compare the forwarded packets with the origin's")
a = ap.parse_args()
T, Z, K, NREP = a.T, a.blocks, a.K, a.nrep
F = Z * K * T - (128077 if Z > 1 else 77)
FEED = NREP + 9  # repair packets per block the origin sends towards the reception
flags = nanorq_amd.EXT_SUBBLOCKS if a.N > 1 else 0

ctx = nanorq_amd.Context(0)
res = {"tool": "bench_device_relay", "route": a.route, "lib": os.path.basename(os.environ.get("NANORQ_HIP_LIB") or nanorq_amd.lib_path()), "F": F, "T": T, "Z": Z, "N": a.N,
       "loss": a.loss, "nrep": NREP, "reps": a.reps}

g = torch.Generator(device="cuda").manual_seed(1)
stride = (T + 4 + 15) // 16 * 16


def lossy(sbn, n, nblk):
    """indices of the packets that arrive: all but --loss of every block's, in block order (the caller shuffles)"""
    key = sbn.double() + torch.rand(n, generator=g, device="cuda", dtype=torch.float64) * 0.5
    order = torch.argsort(key)
    per = torch.bincount(sbn.long(), minlength=nblk)
    start = torch.cumsum(per, 0) - per
    rank = torch.arange(n, device="cuda") - start[sbn[order].long()]
    keep = per - (per.double() * a.loss).long()
    return order[rank < keep[sbn[order].long()]]


def timed(fn):
    """fn() enqueued a.reps times, each between HIP events on the context's stream (after one untimed call)"""
    fn()
    ctx.sync()
    ts = []
    for _ in range(a.reps):
        ctx.timer_start()
        fn()
        ts.append(ctx.timer_stop_ms())
    return {"ms": round(float(min(ts)), 3), "ms_median": round(float(np.median(ts)), 3), "ms_all": [round(float(x), 3) for x in ts]}


def held_leg():
    """route held (see the head of this file)"""
    src = torch.randint(0, 256, (Z, K, T), dtype=torch.uint8, device="cuda", generator=g)
    torch.cuda.synchronize()
    with nanorq_amd.Sender(ctx, K, T, Z, src) as tx:
        tx.encode()
        n = (K + FEED) * Z
        tags = torch.zeros(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        pk = tx.emit_range(0, K + FEED, interleave=True, inline=True, tags_out=tags)
        ctx.sync()
        kept = lossy((tags >> 24) & 0xFF, n, Z)
        kept = kept[torch.randperm(len(kept), generator=g, device="cuda")]
        rx_pk, rx_tags = pk[kept].contiguous(), tags[kept].contiguous()
        del pk, tags
        torch.cuda.synchronize()
        res["packets_in"] = int(rx_pk.shape[0])
        with nanorq_amd.Receiver(ctx, K, T, Z, rep_cap=FEED) as rx, rx.relay() as relay:
            rx.add(rx_pk, inline=True)
            ht = rx.held()
            nh = int(ht.shape[0])
            assert nh == res["packets_in"] and not relay.ready().any()
            res["packets_out"] = nh
            sbn, esi = ((ht >> 24) & 0xFF).long(), ht & 0xFFFFFF
            is_rep = esi >= K
            res["held_repair"] = int(is_rep.sum())
            # the same list with every repair tag replaced by a held source tag of its block (the list is block-major, a
            # block's source tags first)
            per = torch.bincount(sbn, minlength=Z)
            start = torch.cumsum(per, 0) - per
            ns = torch.bincount(sbn[~is_rep], minlength=Z)
            pos = torch.arange(nh, device="cuda") - start[sbn]
            nolook = torch.where(is_rep, ht[start[sbn] + (pos - ns[sbn]).clamp(min=0) % ns[sbn]], ht).contiguous()
            assert bool(((nolook & 0xFFFFFF) < K).all())
            out_a = torch.empty((nh, stride), dtype=torch.uint8, device="cuda")
            out_b = torch.empty((nh, stride), dtype=torch.uint8, device="cuda")
            code = torch.full((nh,), 77, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            relay.emit(ht, out=out_a, inline=True, results=code, held=True)
            tx.emit(ht, out=out_b, inline=True)
            ctx.sync()
            assert bool((code == 0).all()), "a held symbol was not written"
            if not a.no_check:
                assert torch.equal(out_a[:, :T + 4], out_b[:, :T + 4]), "the held packets differ from the origin's"
                res["checked"] = True
            res["held_emit"] = timed(lambda: relay.emit(ht, out=out_a, inline=True, held=True))
            res["sender_emit"] = timed(lambda: tx.emit(ht, out=out_b, inline=True))
            res["held_emit_no_lookup"] = timed(lambda: relay.emit(nolook, out=out_a, inline=True, held=True))
            h, s_, nl = (res[k]["ms_median"] for k in ("held_emit", "sender_emit", "held_emit_no_lookup"))
            res["held_over_sender"] = round(h / s_, 3)
            res["lookup_share"] = round((h - nl) / h, 3)
            res["held_GBps"] = round(nh * T / h / 1e6, 1)
            # what cut-through buys: the first batch's packets, forwarded as soon as the batch is ingested ...
            nb = max(1, int(len(rx_tags) * a.batch))
            b_pk, b_tags, rest_pk = rx_pk[:nb].contiguous(), rx_tags[:nb].contiguous(), rx_pk[nb:].contiguous()
            torch.cuda.synchronize()
            # (the add and the held emit enqueued back to back, no host wait between them: one interval from "the batch is in
            # device memory" to "its packets are written"; the add alone and the emit alone, each after a wait, beside it)
            add_only, emit_only, first, ingest_rest, late = [], [], [], [], []
            for _ in range(a.reps + 1):
                rx.reset()
                ctx.sync()
                ctx.timer_start()
                rx.add(b_pk, inline=True)
                add_only.append(ctx.timer_stop_ms())
                ctx.timer_start()
                relay.emit(b_tags, out=out_a[:nb], inline=True, held=True)
                emit_only.append(ctx.timer_stop_ms())
                rx.reset()
                ctx.sync()
                ctx.timer_start()
                rx.add(b_pk, inline=True)
                relay.emit(b_tags, out=out_a[:nb], inline=True, held=True)
                first.append(ctx.timer_stop_ms())
                # ... against: the rest ingested, the blocks decoded (the relay attached: they become ready), the same packets
                ctx.timer_start()
                rx.add(rest_pk, inline=True)
                ingest_rest.append(ctx.timer_stop_ms())
                ctx.timer_start()
                st, _ = rx.decode()
                relay.emit(b_tags, out=out_a[:nb], inline=True)
                late.append(ctx.timer_stop_ms())
                assert st.all()
            med = lambda v: round(float(np.median(v[1:])), 3)  # noqa: E731  (the first round warms up)
            res["latency"] = {"batch_packets": nb, "batch_ingest_ms": med(add_only), "held_emit_ms": med(emit_only),
                              "held_ingest_and_forward_ms": med(first), "ingest_rest_ms": med(ingest_rest),
                              "decode_then_forward_ms": med(late)}
    print(json.dumps(res))


if a.route == "held":
    held_leg()
    sys.exit(0)

# ---- the origin and the reception's packets ----
obj = torch.randint(0, 256, (F,), dtype=torch.uint8, device="cuda", generator=g)
torch.cuda.synchronize()
with nanorq_amd.ObjectSender(ctx, obj, T, Z=Z, N=a.N, flags=flags) as tx:
    tx.encode()
    n_ref = tx.count_all(NREP)
    ref = None if a.no_check else tx.emit_all(NREP, interleave=True, inline=True)
    n = tx.count_all(FEED)
    tags = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    pk = tx.emit_all(FEED, interleave=True, inline=True, tags_out=tags)
    ctx.sync()
    common, specific = tx.oti
    blocks = tx.blocks
sbn = (tags >> 24) & 0xFF
esi = tags & 0xFFFFFF
if a.loss > 0:
    kept = lossy(sbn, n, Z)
else:
    Ks = torch.tensor([k for k, _ in blocks], device="cuda")
    kept = torch.nonzero(esi < Ks[sbn.long()]).flatten()
kept = kept[torch.randperm(len(kept), generator=g, device="cuda")]
rx_pk = pk[kept].contiguous()
del pk, tags, sbn, esi
torch.cuda.synchronize()
res["packets_in"] = int(rx_pk.shape[0])
res["packets_out"] = n_ref

out_pk = torch.empty((n_ref, stride), dtype=torch.uint8, device="cuda")
out_obj = torch.zeros(F, dtype=torch.uint8, device="cuda") if a.route == "resend" else None
torch.cuda.synchronize()


def ready_leg():
    """route ready (see the head of this file)"""
    rx = nanorq_amd.ObjectReceiver(ctx, common, specific, flags=flags, rep_cap=FEED)
    relay = rx.relay()
    rx.add(rx_pk, inline=True)
    st, _ = rx.decode()
    assert st.all(), "the reception does not decode: blocks %s" % np.flatnonzero(st == 0)[:8]
    relay.encode()
    assert relay.ready().all()
    tl = torch.zeros(n_ref, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    relay.emit_all(NREP, interleave=True, inline=True, out=out_pk, tags_out=tl)
    ctx.sync()
    if ref is not None:
        assert torch.equal(out_pk[:, :T + 4], ref[:, :T + 4]), "the relay's packets differ from the origin's"
        res["checked"] = True
    tl = tl[torch.randperm(n_ref, generator=g, device="cuda")].contiguous()
    torch.cuda.synchronize()
    res["emit_all"] = timed(lambda: relay.emit_all(NREP, interleave=True, inline=True, out=out_pk))
    res["emit_list"] = timed(lambda: relay.emit(tl, out=out_pk, inline=True))
    relay.close()
    rx.close()
    print(json.dumps(res))


if a.route == "ready":
    ready_leg()
    sys.exit(0)


def forward(step):
    """one forwarding over a fresh receiver; step(name) is called after each step"""
    rx = nanorq_amd.ObjectReceiver(ctx, common, specific, flags=flags, rep_cap=FEED)
    relay = rx.relay() if a.route == "relay" else None
    rx.add(rx_pk, inline=True)
    ctx.sync()
    step(None)
    st, _ = rx.decode()
    assert st.all(), "the reception does not decode: blocks %s" % np.flatnonzero(st == 0)[:8]
    step("decode")
    if relay is not None:
        relay.encode()
        step("encode")
        relay.emit_all(NREP, interleave=True, inline=True, out=out_pk)
        step("emit_all")
        relay.close()
    else:
        _, left = rx.write(out_obj)
        assert left == 0
        step("write")
        otx = nanorq_amd.ObjectSender(ctx, out_obj, T, Z=Z, N=a.N, flags=flags)
        step("sender")
        otx.encode()
        step("encode")
        otx.emit_all(NREP, interleave=True, inline=True, out=out_pk)
        step("emit_all")
        otx.close()
    rx.close()


def whole():
    t = []

    def step(name):
        if name is None:
            ctx.timer_start()
        elif name == "emit_all":
            t.append(ctx.timer_stop_ms())
    forward(step)
    return t[0]


def parts():
    out = {}

    def step(name):
        if name is not None:
            out[name + "_ms"] = round(ctx.timer_stop_ms(), 3)
        ctx.timer_start()
    forward(step)
    ctx.timer_stop_ms()
    return out


whole()  # warm-up: code objects, plans, the pool's blocks
if ref is not None:
    ctx.sync()
    assert torch.equal(out_pk[:, :T + 4], ref[:, :T + 4]), "the forwarded packets differ from the origin's"
    res["checked"] = True
    del ref
ts = [whole() for _ in range(a.reps)]
res["forward_ms"] = round(float(min(ts)), 3)
res["forward_ms_median"] = round(float(np.median(ts)), 3)
res["forward_ms_max"] = round(float(max(ts)), 3)
res["forward_ms_all"] = [round(float(x), 3) for x in ts]
res["steps"] = parts()
print(json.dumps(res))
