"""The device-resident receiver (nrq_rx_*) at the headline reception: packets already in HBM -> ingest -> decode, against the
host-list path a caller has without it (tags down to the host, de-duplicated and booked there with numpy, rows placed by
nrq_scatter_symbols, nrq_decode_blocks_lazy).  One JSON line.
    python tools/bench_device_receiver.py [--blocks 256] [--K 8192] [--T 1280] [--loss 0.1] [--reps 5] [--inline]
Ingest time per batch from HIP events around nrq_rx_add; ingest + decode as wall time to the end of the solve (both paths)."""
import argparse
import ctypes as C
import json
import os
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
ap.add_argument("--loss", type=float, default=0.1)
ap.add_argument("--dup", type=float, default=0.03)
ap.add_argument("--late", type=float, default=0.01)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--inline", action="store_true")
ap.add_argument("--no-host", action="store_true", help="device path only")
a = ap.parse_args()
K, T, Z = a.K, a.T, a.blocks

ctx = nanorq_amd.Context(0)
L = ctx._L
L.nrq_scatter_symbols.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]

# ---- the reception: encode on the device, drop, shuffle, duplicate, and a few packets after completion ----
g = torch.Generator().manual_seed(1)
src = torch.randint(0, 256, (Z, K, T), dtype=torch.uint8, generator=g).cuda()
keep = torch.rand((Z, K), generator=g) >= a.loss
nlost = (~keep).sum(1)
R = int(nlost.max())
rep = torch.empty((Z, R, T), dtype=torch.uint8, device="cuda")
ctx.encode_blocks(K, T, Z, src.data_ptr(), K * T, rep.data_ptr(), R * T, np.arange(K, K + R, dtype=np.uint32))
ctx.sync()
bi, ei = torch.nonzero(keep, as_tuple=True)
rb = torch.repeat_interleave(torch.arange(Z), nlost)
rq = torch.cat([torch.arange(int(x)) for x in nlost])
rows = torch.cat([bi * K + ei, Z * K + rb * R + rq])
tags = torch.cat([(bi << 24) | ei, (rb << 24) | (K + rq)])
perm = torch.randperm(len(rows), generator=g)
rows, tags = rows[perm], tags[perm]
nd = int(len(rows) * a.dup)
pick = torch.randint(0, len(rows), (nd,), generator=g)
ins = torch.randint(0, len(rows), (nd,), generator=g)
order = torch.argsort(torch.cat([torch.arange(len(rows)) * 2, ins * 2 + 1]))
rows, tags = torch.cat([rows, rows[pick]])[order], torch.cat([tags, tags[pick]])[order]
nl = int(len(rows) * a.late)
lb, le = torch.randint(0, Z, (nl,), generator=g), torch.randint(0, K, (nl,), generator=g)
rows, tags = torch.cat([rows, lb * K + le]), torch.cat([tags, (lb << 24) | le])
n = len(rows)
flat = torch.cat([src.reshape(-1, T), rep.reshape(-1, T)])
payload = flat[rows.cuda()]
del flat
tags32 = tags.to(torch.int32).cuda()
if a.inline:
    pk = torch.empty((n, T + 4), dtype=torch.uint8, device="cuda")
    be = tags.numpy().astype(np.uint32).astype(">u4").view(np.uint8).reshape(n, 4)
    pk[:, :4] = torch.from_numpy(be).cuda()
    pk[:, 4:] = payload
torch.cuda.synchronize()
rep_cap = R + 8
payload_bytes = int(n) * T

# ---- device path ----
rx = nanorq_amd.Receiver(ctx, K, T, Z, rep_cap)
ingest_ms, dev_ms, st_dev = [], [], None
for r in range(a.reps + 1):
    rx.reset()
    ctx.sync()
    t0 = time.perf_counter()
    ctx.timer_start()
    if a.inline:
        rx.add(pk, inline=True)
    else:
        rx.add(payload, tags=tags32)
    ims = ctx.timer_stop_ms()
    st_dev, _ = rx.decode()
    ctx.sync()
    if r:  # (the first run pays first-use costs)
        ingest_ms.append(ims)
        dev_ms.append(1e3 * (time.perf_counter() - t0))
ok_dev = bool(st_dev.sum() >= Z - 4) and torch.equal(rx.source[st_dev.astype(bool)], src[torch.from_numpy(st_dev.astype(bool)).cuda()])
rx.close()

# ---- host-list path: the same packets, booked on the host ----
host = None
if not a.no_host:
    max_esi = 2 * nanorq_amd.params(K)["Kp"]
    work = torch.empty((Z, K, T), dtype=torch.uint8, device="cuda")
    drep = torch.empty((Z, rep_cap, T), dtype=torch.uint8, device="cuda")
    host_ms, book_ms = [], []
    for r in range(min(a.reps, 3) + 1):
        ctx.sync()
        t0 = time.perf_counter()
        tg = tags32.cpu().numpy().view(np.uint32)
        t1 = time.perf_counter()
        sbn, esi = (tg >> 24).astype(np.int64), (tg & 0xFFFFFF).astype(np.int64)
        key = sbn * (max_esi + 1) + esi
        _, fidx, inv = np.unique(key, return_index=True, return_inverse=True)
        first = fidx[inv] == np.arange(n)
        srcf = first & (esi < K)
        done_at = np.full(Z, n, np.int64)  # packets after the one completing a block are not needed
        cnt = np.bincount(sbn[srcf], minlength=Z)
        last = np.zeros(Z, np.int64)
        np.maximum.at(last, sbn[srcf], np.flatnonzero(srcf))
        done_at[cnt == K] = last[cnt == K]
        live = np.arange(n) <= done_at[sbn]
        added = first & live
        dst = np.zeros(n, np.uint64)
        s_add = added & (esi < K)
        dst[s_add] = np.uint64(work.data_ptr()) + (sbn[s_add] * K * T + esi[s_add] * T).astype(np.uint64)
        r_add = np.flatnonzero(added & (esi >= K))
        o = np.argsort(sbn[r_add], kind="stable")
        rb_, ridx = sbn[r_add][o], r_add[o]
        starts = np.searchsorted(rb_, np.arange(Z))
        q = np.arange(len(rb_)) - starts[rb_]
        dst[ridx] = np.uint64(drep.data_ptr()) + (rb_ * rep_cap * T + q * T).astype(np.uint64)
        resi = np.zeros((Z, rep_cap), np.uint32)
        resi[rb_, q] = esi[ridx]
        nrep_b = np.bincount(rb_, minlength=Z).astype(np.uint32)
        have = np.zeros((Z, K), bool)
        have[sbn[s_add], esi[s_add]] = True
        nl_b = (~have).sum(1).astype(np.uint32)
        lost = np.zeros((Z, max(1, int(nl_b.max()))), np.uint32)
        for b in range(Z):
            m = np.flatnonzero(~have[b])
            lost[b, :len(m)] = m
        t2 = time.perf_counter()
        ctx._chk(L.nrq_scatter_symbols(ctx._h, 0, C.c_void_p(payload.data_ptr()), n, T, dst.ctypes.data_as(C.POINTER(C.c_uint64))))
        nuse = np.where(nrep_b - nl_b > 2, nl_b + 2, nrep_b).astype(np.uint32)
        st = ctx.decode_blocks_lazy(K, T, Z, work.data_ptr(), K * T, lost, nl_b, resi, nuse, nrep_b, drep.data_ptr(), rep_cap * T)
        ctx.sync()
        if r:
            host_ms.append(1e3 * (time.perf_counter() - t0))
            book_ms.append(1e3 * (t2 - t1))
    st_host = st[0] if isinstance(st, tuple) else st
    ok_host = bool(np.array_equal(np.asarray(st_host).astype(bool), st_dev.astype(bool)))
    host = {"ingest_decode_ms": round(min(host_ms), 2), "host_books_ms": round(min(book_ms), 2), "statuses_equal": ok_host}

ing = min(ingest_ms)
print(json.dumps({"K": K, "T": T, "blocks": Z, "loss": a.loss, "packets": int(n), "inline": a.inline,
                  "payload_gb": round(payload_bytes / 1e9, 3), "ingest_ms": round(ing, 3),
                  "ingest_ms_all": [round(x, 3) for x in ingest_ms],
                  "ingest_copy_tbps": round(2 * payload_bytes / ing / 1e9, 2),
                  "device_ingest_decode_ms": round(min(dev_ms), 2), "decoded_blocks": int(st_dev.sum()), "ok": ok_dev,
                  "host_list_path": host}))
