"""Packets of several symbols through the sets (nrq_txset_emit_syms / nrq_rxset_add_syms) against the two routes a caller had
before them.  One JSON line with best and median HIP-event times over --reps (after --warmup reps that the statistics leave out;
the first one's time is reported as *_warm), the routes of a comparison alternated rep by rep in one process.  8 members of 8
blocks (member m: key m + 1, SBNs 8m .. 8m+7), K = 1024, ESIs 0 .. K + 10 % of every block, key and FEC Payload ID inline, at
(T, G) = (64, 16), (256, 5), (1280, 1):
  set_emit_syms_ms    ONE SenderSet.emit_syms of all members' packets into one buffer
  members_repack_ms   8 x Sender.emit_syms into 8 buffers, then a torch repack into the one buffer with the keys written by torch
  set_one_gather_ms   SenderSet.emit (one symbol per packet) into [symbols, T], then a torch gather by a prebuilt index into the
                      packets and the 8-byte headers written by torch
  set_add_syms_ms     ONE ReceiverSet.add_syms of that buffer (counts given)
  members_scan_ms     8 x Receiver.add_syms over the one buffer (behind the key; each member takes its SBNs)
  split_set_add_ms    a torch gather of the packets' symbols into [symbols, T], then ReceiverSet.add with prebuilt keys and tags
  G = 1 only: set_emit_one_ms / set_add_one_ms, the one-symbol set calls (key and tag inline) on the same work.
The emit routes' packets are compared byte for byte, the receptions' lists entry for entry.
    python tools/bench_device_syms_set.py [--reps 10] [--warmup 2]"""
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
K, NMEM, NBLK = 1024, 8, 8
NESI = K + (K + 9) // 10

ctx = nanorq_amd.Context(0)  # (the null stream, as torch's default: the events below bracket torch's work too)
res = {"tool": "bench_device_syms_set", "K": K, "members": NMEM, "blocks_per_member": NBLK, "esis_per_block": NESI, "reps": a.reps,
       "warmup": a.warmup}
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


def ratio(key, x, y):
    res[key] = round(float(np.median(x[a.warmup:]) / np.median(y[a.warmup:])), 3)


def be_bytes(v):
    return torch.stack([(v >> s) & 0xFF for s in (24, 16, 8, 0)], 1).to(torch.uint8)


def shape(T, G):
    lab = "T%d_G%d" % (T, G)
    sset = nanorq_amd.SenderSet(ctx, T)
    txs, m_tags, m_ns, m_buf = [], [], [], []
    for m in range(NMEM):
        src = torch.randint(0, 256, (NBLK, K, T), dtype=torch.uint8, device="cuda", generator=g)
        torch.cuda.synchronize()
        tx = nanorq_amd.Sender(ctx, K, T, NBLK, src, sbn0=NBLK * m)
        tx.encode()
        buf, tg, ns = tx.emit_range_syms(0, NESI, G, interleave=True, inline=True)  # (the member's packet list, and its own buffer)
        ctx.sync()
        sset.attach(m + 1, tx)
        txs.append(tx)
        m_tags.append(tg)
        m_ns.append(ns)
        m_buf.append(buf)
    pm = int(m_tags[0].numel())  # packets per member
    npkt = pm * NMEM
    # the set's list: the members' packets in turn (packet p of member 0, of member 1, ...)
    tags = torch.stack(m_tags, 1).reshape(-1).contiguous()
    ns = torch.stack(m_ns, 1).reshape(-1).contiguous()
    keys = (torch.arange(NMEM, device="cuda", dtype=torch.int32) + 1).repeat(pm).contiguous()
    stride = sset.stride_syms(G, True, True)
    mstride = txs[0].stride_syms(G, True)
    t64, c64 = tags.to(torch.int64) & 0xFFFFFFFF, ns.to(torch.int64)
    hdr8 = torch.cat([be_bytes(keys.to(torch.int64)), be_bytes(t64)], 1)
    # the one-symbol list (the expansion in slot order) and, per slot, its row there
    i = torch.arange(G, device="cuda", dtype=torch.int64)[None, :]
    valid = (i < c64[:, None]).reshape(-1)
    sel = torch.nonzero(valid).flatten()
    p, s = sel // G, sel % G
    one_tags = (t64[p] + s).to(torch.int32).contiguous()
    one_keys = keys[p].contiguous()
    first = torch.cumsum(c64, 0) - c64
    idx = (first[:, None] + torch.minimum(i, c64[:, None] - 1)).reshape(-1)
    nsym_all = int(sel.numel())
    out_a = torch.zeros((npkt, stride), dtype=torch.uint8, device="cuda")
    out_b = torch.zeros((npkt, stride), dtype=torch.uint8, device="cuda")
    out_c = torch.zeros((npkt, stride), dtype=torch.uint8, device="cuda")
    one = torch.zeros((nsym_all, T), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def emit_set():
        sset.emit_syms(keys, tags, G, nsym=ns, out=out_a, inline=True, key_inline=True)

    def emit_members():
        for m in range(NMEM):
            txs[m].emit_syms(m_tags[m], G, nsym=m_ns[m], out=m_buf[m], inline=True)
        ctx.sync()  # (the library's stream and torch's are not ordered: a caller of this route waits here too)
        v = out_b.view(pm, NMEM, stride)
        for m in range(NMEM):
            v[:, m, 4:4 + 4 + G * T] = m_buf[m][:, :4 + G * T]
        out_b[:, :4] = hdr8[:, :4]
        torch.cuda.synchronize()

    def emit_one_gather():
        sset.emit(one_keys, one_tags, out=one)
        ctx.sync()
        out_c[:, 8:8 + G * T] = one[idx].view(npkt, G * T)
        out_c[:, :8] = hdr8
        torch.cuda.synchronize()

    t_a, t_b, t_c = [], [], []
    for _ in range(a.warmup + a.reps):
        t_a.append(timed(emit_set))
        t_b.append(timed(emit_members))
        t_c.append(timed(emit_one_gather))
    torch.cuda.synchronize()
    ctx.sync()
    keep = torch.zeros((npkt, stride), dtype=torch.bool, device="cuda")
    keep[:, :8] = True
    keep[:, 8:8 + G * T] = valid.view(npkt, G).repeat_interleave(T, 1)
    assert torch.equal(out_a[keep], out_b[keep]) and torch.equal(out_a[keep], out_c[keep]), "the emit routes wrote different packets"
    res["packets_" + lab] = npkt
    stats("set_emit_syms_%s_ms" % lab, t_a)
    stats("members_repack_%s_ms" % lab, t_b)
    stats("set_one_gather_%s_ms" % lab, t_c)
    ratio("set_emit_syms_vs_members_" + lab, t_a, t_b)
    ratio("set_emit_syms_vs_one_gather_" + lab, t_a, t_c)

    # ingest: three groups of receivers, one per route
    rep_cap = NESI - K + 8
    groups = [[nanorq_amd.Receiver(ctx, K, T, NBLK, rep_cap, sbn0=NBLK * m) for m in range(NMEM)] for _ in range(3)]
    rset_a, rset_c = nanorq_amd.ReceiverSet(ctx, T), nanorq_amd.ReceiverSet(ctx, T)
    for m in range(NMEM):
        rset_a.attach(m + 1, groups[0][m])
        rset_c.attach(m + 1, groups[2][m])
    torch.cuda.synchronize()

    def add_set():
        rset_a.add_syms(out_a, G, nsym=ns, inline=True, key_inline=True)

    def add_members():
        for rx in groups[1]:
            rx.add_syms(out_a.data_ptr() + 4, G, nsym=ns, inline=True, n=npkt, stride=stride)

    def add_split():
        syms = out_a[:, 8:8 + G * T].reshape(npkt * G, T)[sel]
        torch.cuda.synchronize()
        rset_c.add(syms, keys=one_keys, tags=one_tags)

    t_a, t_b, t_c = [], [], []
    for _ in range(a.warmup + a.reps):
        for grp in groups:
            for rx in grp:
                rx.reset()
        t_a.append(timed(add_set))
        t_b.append(timed(add_members))
        t_c.append(timed(add_split))
    for m in range(NMEM):
        la, lb, lc = (groups[r][m].lists() for r in range(3))
        assert all(np.array_equal(x, y) and np.array_equal(x, z) for x, y, z in zip(la[0] + la[1], lb[0] + lb[1], lc[0] + lc[1])), \
            "the ingest routes left different books"
    stats("set_add_syms_%s_ms" % lab, t_a)
    stats("members_scan_%s_ms" % lab, t_b)
    stats("split_set_add_%s_ms" % lab, t_c)
    ratio("set_add_syms_vs_members_" + lab, t_a, t_b)
    ratio("set_add_syms_vs_split_" + lab, t_a, t_c)

    if G == 1:  # the new calls against the one-symbol set calls themselves
        out_1 = torch.zeros((npkt, stride), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        t_n, t_o, u_n, u_o = [], [], [], []
        for _ in range(a.warmup + a.reps):
            t_n.append(timed(emit_set))
            t_o.append(timed(lambda: sset.emit(keys, tags, out=out_1, inline=True, key_inline=True)))
            for grp in (groups[0], groups[2]):
                for rx in grp:
                    rx.reset()
            u_n.append(timed(add_set))
            u_o.append(timed(lambda: rset_c.add(out_1, inline=True, key_inline=True)))
        ctx.sync()
        assert torch.equal(out_1[:, :T + 8], out_a[:, :T + 8])
        stats("set_emit_syms_g1_ms", t_n)
        stats("set_emit_one_ms", t_o)
        stats("set_add_syms_g1_ms", u_n)
        stats("set_add_one_ms", u_o)
        ratio("set_emit_syms_vs_one", t_n, t_o)
        ratio("set_add_syms_vs_one", u_n, u_o)
    for h in [rset_a, rset_c, sset] + [rx for grp in groups for rx in grp] + txs:
        h.close()
    torch.cuda.empty_cache()


for T, G in ((64, 16), (256, 5), (1280, 1)):
    shape(T, G)
print(json.dumps(res))
