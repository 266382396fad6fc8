"""What a reception wants, listed on the device against the host path it replaces, at the headline reception: --blocks x K source
symbols of T bytes, --loss of every block's source symbols missing, no repair symbol in yet, rep_cap = the most a block lost + 2 + 3
(what bench.py's decode may take per block).  Two routes to the same device tensor of tags, each timed on the host clock from the
call to the completed list (best and median of --reps, after one untimed call):
  want   Receiver.want(extra=2): count, allocate, fill -- the list never leaves the device                          (nrq_rx_want)
  host   Receiver.lists() brings the books down, numpy builds the same tag list (per block its lost + 2 - nrep lowest repair ESIs
         that are not in its repair list, at most its free rows), torch uploads it
The two lists are compared.  One JSON line.
    python tools/bench_device_want.py [--blocks 256] [--K 8192] [--T 1280] [--loss 0.1] [--extra 2] [--reps 10]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: torch's HIP runtime must find the device first)

torch.cuda.init()
torch.empty(1, device="cuda")
import nanorq_amd  # noqa: E402
from util import loss_pattern  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--blocks", type=int, default=256)
ap.add_argument("--K", type=int, default=8192)
ap.add_argument("--T", type=int, default=1280)
ap.add_argument("--loss", type=float, default=0.1)
ap.add_argument("--extra", type=int, default=2)
ap.add_argument("--reps", type=int, default=10)
a = ap.parse_args()
K, T, NB = a.K, a.T, a.blocks

lost = [loss_pattern(K, a.loss, seed=1000, block=b) for b in range(NB)]
rep_cap = max(len(x) for x in lost) + 2 + 3
ctx = nanorq_amd.Context(0)
rx = nanorq_amd.Receiver(ctx, K, T, NB, rep_cap=rep_cap)
CH = 16  # blocks per ingest call: the packets' bytes do not matter to the books, one buffer serves every call
pkts = torch.empty((CH * K, T), dtype=torch.uint8, device="cuda")
for b0 in range(0, NB, CH):
    tg = np.concatenate([(b << 24) | np.setdiff1d(np.arange(K), lost[b]).astype(np.uint32) for b in range(b0, min(NB, b0 + CH))]).astype(np.uint32)
    d_tg = torch.from_numpy(tg.view(np.int32)).cuda()
    torch.cuda.synchronize()
    rx.add(pkts[:len(tg)], tags=d_tg)
    ctx.sync()
del pkts


def route_want():
    return rx.want(extra=a.extra)


def route_host():
    lost_l, reps_l = rx.lists()
    out = []
    for b in range(NB):
        g, r = len(lost_l[b]), len(reps_l[b])
        if g == 0:
            continue
        need = min(max(g + a.extra - r, 0), rep_cap - r)
        es = np.setdiff1d(np.arange(K, K + need + r, dtype=np.uint32), reps_l[b], assume_unique=True)[:need]
        out.append((np.uint32(b << 24) | es).astype(np.uint32))
    t = torch.from_numpy(np.concatenate(out).view(np.int32)).cuda()
    torch.cuda.synchronize()
    return t


def timed(fn):
    fn()
    ms = []
    for _ in range(a.reps):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"best_ms": round(min(ms), 4), "median_ms": round(float(np.median(ms)), 4)}


w, h = route_want(), route_host()
assert torch.equal(w, h), "the two routes give different lists"
res = {"tool": "bench_device_want", "blocks": NB, "K": K, "T": T, "loss": a.loss, "extra": a.extra, "rep_cap": rep_cap, "tags": int(w.numel()),
       "reps": a.reps, "want": timed(route_want), "host": timed(route_host)}
res["host_over_want"] = round(res["host"]["median_ms"] / res["want"]["median_ms"], 2)
print(json.dumps(res))
