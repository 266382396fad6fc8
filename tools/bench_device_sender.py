"""The device-resident sender (nrq_tx_*) at the headline emission: 256 blocks of K=8192, T=1280, every block's source ESIs and
911 repair ESIs (enough for a 10 % loss at overhead 0), interleaved, with inline FEC Payload IDs at a 1296-byte stride -- 2,330,368
packets, 3.02 GB written -- against what a caller has without it: nrq_encode_blocks with the repair list, then the packets put
together with torch ops.  One JSON line.
    python tools/bench_device_sender.py [--blocks 256] [--K 8192] [--T 1280] [--repair 911] [--reps 10] [--no-baseline] [--ab]
emit_ms: HIP events around nrq_tx_emit_range; --ab alternates the 16-byte and the 4-byte ("tx_dword") store paths rep by rep.
The floor is bytes over the copy rate DESIGN.md section 10 uses (6.29 TB/s): the source rows read and the packets written, plus
the repair gathers when every gathered row comes from HBM (floor_hbm_ms) or nothing when they are served on-die (floor_ondie_ms)."""
import argparse
import json
import os
import re
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT]
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: torch's HIP runtime must find the device first)

torch.cuda.init()
torch.empty(1, device="cuda")
import nanorq_amd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--blocks", type=int, default=256)
ap.add_argument("--K", type=int, default=8192)
ap.add_argument("--T", type=int, default=1280)
ap.add_argument("--repair", type=int, default=911)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--no-baseline", action="store_true", help="sender only (profiler runs)")
ap.add_argument("--ab", action="store_true", help="also time the 4-byte store path")
a = ap.parse_args()
K, T, Z, R = a.K, a.T, a.blocks, a.repair
COPY_TBPS = 6.29


def lt_degrees(Kp, isis):
    """number of rows rq_lt_columns XORs for each ISI (RFC 6330 5.3.5.2-4: d LT neighbours plus d1 PI neighbours)"""
    txt = open(os.path.join(ROOT, "nanorq_amd", "csrc", "rfc6330_tables.h")).read()
    body = txt[txt.index("#define RQ_V_WORDS"):]
    body = body[:body.index("\n\n")] if "\n\n" in body else body
    V = [int(x, 0) for x in re.findall(r"0x[0-9A-Fa-f]+|\b\d+u?\b", body.replace("u", ""))][:1024]
    degF = [0, 5243, 529531, 704294, 791675, 844104, 879057, 904023, 922747, 937311, 948962, 958494, 966438, 973160, 978921,
            983914, 988283, 992138, 995565, 998631, 1001391, 1003887, 1006157, 1008229, 1010129, 1011876, 1013490, 1014983,
            1016370, 1017662, 1048576]
    p = nanorq_amd.params(Kp)
    J, W = p["J"], p["W"]

    def rnd(y, i, m):
        return (V[(y + i) & 255] ^ V[256 + (((y >> 8) + i) & 255)] ^ V[512 + (((y >> 16) + i) & 255)] ^
                V[768 + (((y >> 24) + i) & 255)]) % m
    A = 53591 + J * 997
    A += (A & 1) == 0
    B1 = 10267 * (J + 1)
    out = []
    for X in isis:
        y = (B1 + X * A) & 0xFFFFFFFF
        v = rnd(y, 0, 1 << 20)
        d = next(k for k in range(31) if v < degF[k])
        d = min(d, W - 2)
        d1 = 2 + rnd(X, 3, 2) if d < 4 else 2
        out.append(d + d1)
    return np.array(out)


ctx = nanorq_amd.Context(0)
Kp = nanorq_amd.params(K)["Kp"]
g = torch.Generator().manual_seed(1)
src = torch.randint(0, 256, (Z, K, T), dtype=torch.uint8, generator=g).cuda()
torch.cuda.synchronize()
per = K + R
n = Z * per
stride = (T + 4 + 15) // 16 * 16
pk = torch.empty((n, stride), dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()

cols = lt_degrees(Kp, np.arange(K, K + R) + (Kp - K))
b_src, b_pkt = Z * K * T, n * (T + 4)
b_gather = int(cols.sum()) * Z * T
floor_ondie = (b_src + b_pkt) / (COPY_TBPS * 1e12) * 1e3             # the gathers served on-die
floor_hbm = (b_src + b_pkt + b_gather) / (COPY_TBPS * 1e12) * 1e3  # every gathered row read from HBM

tx = nanorq_amd.Sender(ctx, K, T, Z, src)
ctx.sync()
t0 = time.perf_counter()
tx.encode()
ctx.sync()
enc_ms = 1e3 * (time.perf_counter() - t0)
times = {"v16": [], "dword": []}
modes = ["v16", "dword"] if a.ab else ["v16"]
for r in range(a.reps + 1):
    for m in modes:
        ctx.set_option("tx_dword", 1 if m == "dword" else 0)
        ctx.sync()
        ctx.timer_start()
        tx.emit_range(0, per, interleave=True, inline=True, out=pk)
        ms = ctx.timer_stop_ms()
        if r:  # (the first run pays first-use costs)
            times[m].append(ms)
ctx.set_option("tx_dword", 0)
ctx.sync()
t0 = time.perf_counter()
tx.encode()
tx.emit_range(0, per, interleave=True, inline=True, out=pk)
ctx.sync()
enc_emit_ms = 1e3 * (time.perf_counter() - t0)

base = None
if not a.no_baseline:
    # what a caller does today: the repair symbols by nrq_encode_blocks, then the packets put together with torch
    rep = torch.empty((Z, R, T), dtype=torch.uint8, device="cuda")
    hdr = torch.from_numpy(((np.arange(Z, dtype=np.uint32)[None, :] << 24) | np.arange(per, dtype=np.uint32)[:, None])
                           .astype(">u4").view(np.uint8).reshape(per, Z, 4).copy()).cuda()
    out = torch.empty((n, stride), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    esis = np.arange(K, K + R, dtype=np.uint32)
    bt = []
    for r in range(min(a.reps, 3) + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.encode_blocks(K, T, Z, src.data_ptr(), K * T, rep.data_ptr(), R * T, esis)
        ctx.sync()
        o = out.view(per, Z, stride)
        o[:, :, :4] = hdr
        o[:K, :, 4:4 + T] = src.permute(1, 0, 2)
        o[K:, :, 4:4 + T] = rep.permute(1, 0, 2)
        torch.cuda.synchronize()
        if r:
            bt.append(1e3 * (time.perf_counter() - t0))
    same = bool(torch.equal(out[:, :4 + T], pk[:, :4 + T]))
    base = {"encode_blocks_plus_torch_ms": round(min(bt), 2), "packets_equal": same}
    del out, rep

em = min(times["v16"])
res = {"K": K, "T": T, "blocks": Z, "repair_per_block": R, "packets": n, "stride": stride, "written_gb": round(b_pkt / 1e9, 3),
       "avg_rows_per_repair": round(float(cols.mean()), 3), "gather_gb": round(b_gather / 1e9, 3), "source_gb": round(b_src / 1e9, 3),
       "emit_ms": round(em, 3), "emit_ms_median": round(float(np.median(times["v16"])), 3),
       "floor_ondie_ms": round(floor_ondie, 3), "floor_hbm_ms": round(floor_hbm, 3), "x_ondie_floor": round(em / floor_ondie, 2),
       "encode_ms": round(enc_ms, 2), "encode_emit_ms": round(enc_emit_ms, 2), "baseline": base}
if a.ab:
    res["emit_ms_dword"] = round(min(times["dword"]), 3)
    res["emit_ms_dword_median"] = round(float(np.median(times["dword"])), 3)
tx.close()
print(json.dumps(res))
