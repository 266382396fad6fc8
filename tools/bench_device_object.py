"""Whole objects on the device (nrq_otx_* / nrq_orx_*) at the headline object: F = 256*8192*1280 - 128,077 bytes, T = 1280, Z = 256
(156 blocks of K=8192, 100 of K=8191).  One JSON line with, as best and median HIP-event times over --reps:
  layout_{N}_{to_rows,to_obj}_ms   the layout kernel alone, N = 1 (16-byte pieces), 4 (320-byte sub-symbols, 16-byte pieces) and
                                   3 (432 / 424-byte sub-symbols, 8-byte pieces), against the floor 2*F / 6.29 TB/s
  emit_all_ms vs sender_ms         ObjectSender.emit_all(911, interleaved, inline) of a 256 x 8192 object against one-class
                                   Sender.emit_range of the same blocks (equal bytes), alternated rep by rep
  emit_all_headline_ms             ObjectSender.emit_all(911, interleaved, inline) of the headline object (two classes and the
                                   last block staged apart: a table of three segments)
  orx_add_ms vs rx_add_ms          ObjectReceiver.add against one-class Receiver.add on the same packets (the 256 x 8192 object:
                                   one class, one reception inside), alternated
  orx_add_headline_ms              ObjectReceiver.add of the headline object's own emit_all(911) packets (two classes: a reception
                                   per class, each scanning every packet), against rx_add_ms (100 packets fewer), alternated
    python tools/bench_device_object.py [--reps 10] [--skip-layout] [--skip-emit] [--skip-add]"""
import argparse
import ctypes as C
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
ap.add_argument("--skip-layout", action="store_true")
ap.add_argument("--skip-emit", action="store_true")
ap.add_argument("--skip-add", action="store_true")
a = ap.parse_args()
COPY_TBPS = 6.29
T, Z, K, NREP = 1280, 256, 8192, 911
F = Z * K * T - 128077

ctx = nanorq_amd.Context(0)
L = ctx._L
res = {"tool": "bench_device_object", "F": F, "T": T, "Z": Z, "reps": a.reps}


def timed(fn):
    ctx.sync()
    ctx.timer_start()
    fn()
    return ctx.timer_stop_ms()


def stats(key, ts):
    res[key] = round(float(min(ts)), 3)
    res[key + "_median"] = round(float(np.median(ts)), 3)


g = torch.Generator(device="cuda").manual_seed(1)
obj = torch.randint(0, 256, (F,), dtype=torch.uint8, device="cuda", generator=g)
torch.cuda.synchronize()

if not a.skip_layout:
    # the layout kernel alone (nrq_obj_layout), both directions
    res["layout_floor_ms"] = round(2 * F / (COPY_TBPS * 1e9), 3)
    out = torch.empty(F, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for N in (1, 4, 3):
        flags = nanorq_amd.EXT_SUBBLOCKS if N > 1 else 0
        p = nanorq_amd.obj_params_enc(F, T, 0, Z, N, 8, flags)
        res["layout_%d_sub" % N] = [p.TL, p.TS]
        rows = torch.empty(p.Kt * T, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        to_rows, to_obj = [], []
        for _ in range(a.reps):
            to_rows.append(timed(lambda: L.nrq_obj_layout(ctx._h, C.byref(p), C.c_void_p(obj.data_ptr()), C.c_void_p(rows.data_ptr()), 0)))
            to_obj.append(timed(lambda: L.nrq_obj_layout(ctx._h, C.byref(p), C.c_void_p(out.data_ptr()), C.c_void_p(rows.data_ptr()), 1)))
        ctx.sync()
        assert torch.equal(out, obj), "layout round trip differs (N=%d)" % N
        stats("layout_%d_to_rows_ms" % N, to_rows)
        stats("layout_%d_to_obj_ms" % N, to_obj)
        del rows
    del out

if not a.skip_emit or not a.skip_add:
    # a 256 x 8192 object: one class, so Sender (one transmission) and ObjectSender emit the same packets
    F1 = Z * K * T
    obj1 = torch.cat([obj, torch.randint(0, 256, (F1 - F,), dtype=torch.uint8, device="cuda", generator=g)])
    torch.cuda.synchronize()
    otx = nanorq_amd.ObjectSender(ctx, obj1, T, Z=Z)
    assert otx.blocks == [(K, nanorq_amd.params(K)["Kp"])] * Z
    tx = nanorq_amd.Sender(ctx, K, T, Z, obj1)
    otx.encode()
    tx.encode()
    n = Z * (K + NREP)
    stride = (T + 4 + 15) // 16 * 16
    pk_o = torch.empty((n, stride), dtype=torch.uint8, device="cuda")
    pk_s = torch.empty((n, stride), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    t_o, t_s = [], []
    for _ in range(a.reps):
        t_o.append(timed(lambda: otx.emit_all(NREP, interleave=True, inline=True, out=pk_o)))
        t_s.append(timed(lambda: tx.emit_range(0, K + NREP, interleave=True, inline=True, out=pk_s)))
    ctx.sync()
    assert torch.equal(pk_o, pk_s), "emit_all and emit_range packets differ"
    res["packets"] = n
    res["packet_bytes"] = n * stride
    if not a.skip_emit:
        stats("emit_all_ms", t_o)
        stats("sender_ms", t_s)
        res["emit_all_vs_sender"] = round(float(np.median(t_o) / np.median(t_s)), 3)
        with nanorq_amd.ObjectSender(ctx, obj, T, Z=Z) as htx:
            htx.encode()
            pk_h = torch.empty((htx.count_all(NREP), stride), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            t_h = [timed(lambda: htx.emit_all(NREP, interleave=True, inline=True, out=pk_h)) for _ in range(a.reps)]
            stats("emit_all_headline_ms", t_h)
            ctx.sync()
        del pk_h
    del pk_s
    otx.close()
    tx.close()
    if not a.skip_add:
        p1 = nanorq_amd.obj_params_enc(F1, T, 0, Z, 1, 8, 0)
        with nanorq_amd.ObjectSender(ctx, obj, T, Z=Z) as htx:  # the headline object: 156 x 8192 and 100 x 8191
            htx.encode()
            pk_h = htx.emit_all(NREP, interleave=True, inline=True)
            ctx.sync()
            hcommon, hspecific = htx.oti
        res["headline_packets"] = int(pk_h.shape[0])
        t_o, t_r, t_h = [], [], []
        for _ in range(a.reps):
            orx = nanorq_amd.ObjectReceiver(ctx, p1.oti_common, p1.oti_specific, rep_cap=NREP)
            rx = nanorq_amd.Receiver(ctx, K, T, Z, NREP)
            hrx = nanorq_amd.ObjectReceiver(ctx, hcommon, hspecific, rep_cap=NREP)
            ctx.sync()
            t_o.append(timed(lambda: orx.add(pk_o, inline=True)))
            t_r.append(timed(lambda: rx.add(pk_o, inline=True)))
            t_h.append(timed(lambda: hrx.add(pk_h, inline=True)))
            for r in (orx, rx, hrx):
                r.close()
        stats("orx_add_ms", t_o)
        stats("rx_add_ms", t_r)
        stats("orx_add_headline_ms", t_h)
        res["orx_add_vs_rx_add"] = round(float(np.median(t_o) / np.median(t_r)), 3)
        res["orx_add_headline_vs_rx_add"] = round(float(np.median(t_h) / np.median(t_r)), 3)

print(json.dumps(res))
