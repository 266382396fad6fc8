"""The range mode of a sender set (nrq_txset_emit_all) against the list emit it stands in for.  One JSON line with best and median
times over --reps, the routes alternated rep by rep in one process, at the two shapes of tools/bench_device_txset.py: every source
ESI plus 911 repair ESIs of every block, interleaved over all blocks of the set (round j: packet j of every block, in the set's
block order), each packet key | FEC Payload ID | payload at a stride of T + 8 rounded up to 16.
    range_<m>_ms   (a) ONE SenderSet.emit_all(key_inline=True, inline=True): the map pass, then the payload kernels (HIP events)
    list_<m>_ms    (b) SenderSet.emit over the same keys and tags already on the device: the three bucketing passes, then the same
                       payload kernels -- the payload floor; (a) - (b) is the map pass against the bucketing passes (HIP events)
    host_<m>_ms    (c) the route a caller has without the range mode: the numpy build of the interleaved keys and tags, their
                       upload, and the emit -- host wall time around a ctx.sync()
  <m> = obj8: 8 objects of 32 blocks of K = 8192 (2.33 M packets); tx64: 64 senders of 4 blocks of K = 1000.  The packets of the
  three routes are compared byte for byte.
    python tools/bench_device_txset_range.py [--reps 10] [--only obj8|tx64]"""
import argparse
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
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--only", choices=("obj8", "tx64"))
a = ap.parse_args()
T, NREP = 1280, 911
KSTRIDE = (T + 8 + 15) // 16 * 16

ctx = nanorq_amd.Context(0)  # (the null stream, as torch's default)
res = {"tool": "bench_device_txset_range", "T": T, "nrep": NREP, "reps": a.reps}
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


def host_lists(bkeys, bsbn, bK):
    """the interleaved (keys, tags) of all source and NREP repair ESIs of every block, built as a caller would: numpy on the host"""
    lens = bK.astype(np.int64) + NREP
    blk = np.repeat(np.arange(len(lens)), lens)
    j = np.arange(int(lens.sum())) - np.repeat(np.cumsum(lens) - lens, lens)
    perm = np.lexsort((blk, j))
    blk, j = blk[perm], j[perm]
    return bkeys[blk].astype(np.uint32), ((bsbn[blk].astype(np.uint32) << 24) | j.astype(np.uint32))


def many(label, nmem, K, nblk, make, blocks_K):
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
    bkeys, bsbn = st.blocks()
    bK = np.concatenate([blocks_K(tx) for tx in txs]).astype(np.uint32)  # (keys 0 .. nmem-1 in attach order: the set's block order)
    n = st.count_all(NREP)
    out_a, out_b, out_c = (torch.zeros((n, KSTRIDE), dtype=torch.uint8, device="cuda") for _ in range(3))
    keys = torch.zeros(n, dtype=torch.int32, device="cuda")
    tags = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    st.emit_all(NREP, inline=True, key_inline=True, out=out_a, keys_out=keys, tags_out=tags)  # (the lists of route (b); warm-up)
    ctx.sync()

    def route_a():
        st.emit_all(NREP, inline=True, key_inline=True, out=out_a)

    def route_b():
        st.emit(keys, tags, out=out_b, inline=True, key_inline=True)

    def route_c():
        t0 = time.perf_counter()
        hk, ht = host_lists(bkeys, bsbn, bK)
        dk, dt = torch.from_numpy(hk.view(np.int32)).cuda(), torch.from_numpy(ht.view(np.int32)).cuda()
        torch.cuda.synchronize()
        st.emit(dk, dt, out=out_c, inline=True, key_inline=True)
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3

    route_b()
    ctx.sync()
    t_a, t_b, t_c = [], [], []
    for _ in range(a.reps):
        t_a.append(timed(route_a))
        t_b.append(timed(route_b))
        torch.cuda.synchronize()
        ctx.sync()
        t_c.append(route_c())
    torch.cuda.synchronize()
    assert torch.equal(out_a, out_b) and torch.equal(out_a, out_c), "the routes wrote different packets"
    assert bool((out_a[:, 8:T + 8] != 0).any())
    res["packets_" + label] = n
    stats("range_%s_ms" % label, t_a)
    stats("list_%s_ms" % label, t_b)
    stats("host_%s_ms" % label, t_c)
    res["range_minus_list_%s_ms" % label] = round(float(np.median(t_a) - np.median(t_b)), 3)
    st.close()
    for tx in txs:
        tx.close()


if a.only in (None, "obj8"):
    many("obj8", 8, 8192, 32, lambda src: nanorq_amd.ObjectSender(ctx, src, T, Z=32), lambda tx: np.array([K for K, _ in tx.blocks]))
    torch.cuda.empty_cache()
if a.only in (None, "tx64"):
    many("tx64", 64, 1000, 4, lambda src: nanorq_amd.Sender(ctx, 1000, T, 4, src), lambda tx: np.full(4, 1000))

print(json.dumps(res))
