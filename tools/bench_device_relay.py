"""Forwarding an object on the device: from "packets ingested" to "emit_all(911) written", at the headline object (F = 256*8192*1280
- 128,077 bytes, T = 1280, Z = 256: 156 blocks of K=8192, 100 of K=8191).  Two routes over the same reception:
  relay   ObjectReceiver.decode -> relay.encode (the blocks no decode made ready) -> relay.emit_all            (nrq_orx_relay)
  resend  ObjectReceiver.decode -> write -> ObjectSender over the written object -> encode -> emit_all         (no relay needed)
The reception: the origin's emit_all(920) packets, `--loss` of every block's packets dropped, the rest shuffled (--loss 0: exactly
the source packets, so that no block needs a decode).  One JSON line with, as best and median HIP-event times over --reps,
forward_ms (the whole route) and, from one more rep with a wait after each step, the steps' times.  The route "resend" uses no
call a library without relays lacks, so NANORQ_HIP_LIB=<an older build> runs it on that build (A/B, process by process).
    python tools/bench_device_relay.py --route relay|resend [--loss 0.1] [--reps 10] [--nrep 911] [--N 1] [--no-check]"""
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
ap.add_argument("--route", choices=("relay", "resend"), required=True)
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

# ---- the origin and the reception's packets ----
g = torch.Generator(device="cuda").manual_seed(1)
obj = torch.randint(0, 256, (F,), dtype=torch.uint8, device="cuda", generator=g)
torch.cuda.synchronize()
stride = (T + 4 + 15) // 16 * 16
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
    key = sbn.double() + torch.rand(n, generator=g, device="cuda", dtype=torch.float64) * 0.5
    order = torch.argsort(key)
    per = torch.bincount(sbn.long(), minlength=Z)
    start = torch.cumsum(per, 0) - per
    rank = torch.arange(n, device="cuda") - start[sbn[order].long()]
    keep = per - (per.double() * a.loss).long()
    kept = order[rank < keep[sbn[order].long()]]
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
