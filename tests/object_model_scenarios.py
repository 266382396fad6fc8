"""Groups e and f of tests/host_model_worker.py: the object layer (nanorq_amd/csrc/nanorq_api.c) under fault injection, over the
model HIP runtime.  The scenarios are those of tests/test_gpu_faults.py -- the same objects, the same `fail_after` sweeps, the
same floors for how many runs must have met their injected failure -- re-stated for a runtime whose kernels move no bytes: what
is compared byte for byte is what travels by copies alone (the received source symbols, into the output), and the packets are
made without an encoder (source symbols are slices of the object, a repair symbol's bytes do not matter to the host layer)."""
import ctypes as C

import numpy as np

from util import payload

SYM_ADDED, SYM_ERR = 0, -1


def groups(W):
    """W: the worker module (its model(), hazards(), brief(), fuzz0(), counters())"""
    import capi

    def opt(name, value):
        L = capi.api()
        L.nanorq_hip_option.restype = C.c_int
        L.nanorq_hip_option.argtypes = [C.c_size_t, C.c_char_p, C.c_longlong]
        return L.nanorq_hip_option(0, name.encode(), value)

    def faults():
        return opt("faults_injected", 0)

    def packets(F, T, K, loss, oh, seed):
        """encode_object's packets (capi.py: the same draws decide what is lost) without an encoder: (data, common, specific,
        [(tag, bytes)], {tag of a source symbol: (offset, bytes of the object it holds)})"""
        L = capi.api()
        data = payload(F, seed=seed)
        rq = L.nanorq_encoder_new_ex(F, T, K, 0, 8)
        assert rq
        rng = np.random.default_rng(seed)
        pk, where = [], {}
        off = 0
        for sbn in range(L.nanorq_blocks(rq)):
            nk = L.nanorq_block_symbols(rq, sbn)
            dropped = 0
            for esi in range(nk):
                o = off + esi * T
                if rng.random() < loss:
                    dropped += 1
                    continue
                sym = np.zeros(T, np.uint8)
                n = max(0, min(T, F - o))
                sym[:n] = data[o:o + n]
                tag = L.nanorq_tag(sbn, esi)
                pk.append((tag, sym.tobytes()))
                where[tag] = (o, n)
            for esi in range(nk, nk + dropped + oh):
                pk.append((L.nanorq_tag(sbn, esi), payload(T, seed=seed + 1000, block=sbn * 65536 + esi).tobytes()))
            off += nk * T
        c, s = L.nanorq_oti_common(rq), L.nanorq_oti_scheme_specific(rq)
        L.nanorq_free(rq)
        return data, c, s, pk, where

    def feed_pinned(L, dq, pk, T, oio, asynchronous=False):
        addr, view = capi.pinned_array(len(pk) * T)
        view[:] = np.frombuffer(b"".join(p for _, p in pk), np.uint8)
        tags = np.array([t for t, _ in pk], np.uint32)
        res = np.full(len(pk), 77, np.int32)
        fn = L.nanorq_decoder_add_symbols_async if asynchronous else L.nanorq_decoder_add_symbols
        n = fn(dq, C.c_void_p(addr), tags.ctypes.data_as(C.POINTER(C.c_uint32)), len(pk), res.ctypes.data_as(C.POINTER(C.c_int)), oio)
        return n, res, addr

    class Report:
        def __init__(self):
            self.failures, self.hz, self.hit, self.rolled_back, self.runs = [], [], 0, 0, 0

        def check(self, cond, *what):
            if not cond and len(self.failures) < 40:
                self.failures.append(" ".join(str(w) for w in what))
            return cond

        def collect(self, n):
            hz = W.hazards()
            if hz and len(self.hz) < 40:
                self.hz += ["n=%s %s" % (n, t) for t in W.brief(hz)[:4]]
            self.runs += 1

        def result(self):
            return dict(failures=self.failures, hazards=self.hz, hit=self.hit, rolled_back=self.rolled_back, runs=self.runs)

    def books_match(R, L, dq, pk, res, K, n):
        for b in range(L.nanorq_blocks(dq)):
            nsrc = sum(1 for (t, _), r in zip(pk, res) if r == SYM_ADDED and t >> 24 == b and (t & 0xFFFFFF) < K)
            nrep = sum(1 for (t, _), r in zip(pk, res) if r == SYM_ADDED and t >> 24 == b and (t & 0xFFFFFF) >= K)
            R.check(L.nanorq_num_repair(dq, b) == nrep, "n", n, "block", b, "repair count", L.nanorq_num_repair(dq, b), "booked", nrep)
            R.check(L.nanorq_num_missing(dq, b) == L.nanorq_block_symbols(dq, b) - nsrc, "n", n, "block", b, "gaps do not match the results")

    def received_right(R, out, data, pk, where, n, blocks=None):
        """every received source symbol is in the output where it belongs (it got there by copies alone)"""
        bad = 0
        for t, _ in pk:
            if t in where and (blocks is None or t >> 24 in blocks):
                o, m = where[t]
                bad += not np.array_equal(out[o:o + m], data[o:o + m])
        R.check(bad == 0, "n", n, bad, "received source symbols are not in the output")

    def batch(asynchronous):
        L = capi.api()
        R = Report()
        T, K = 256, 120
        data, c, s, pk, where = packets(5 * K * T - 9, T, K, 0.1, 3, seed=5)
        for n in list(range(1, 40)) + [48, 64, 96]:
            dq = L.nanorq_decoder_new(c, s)
            oio, out = capi.pinned_io(len(data))
            out[:] = 0
            before = faults()
            R.check(opt("fail_after", n) == 0, "fail_after is not an option")
            added, res, addr = feed_pinned(L, dq, pk, T, oio, asynchronous)
            opt("fail_after", 0)
            R.hit += faults() > before
            R.check(added == int((res == SYM_ADDED).sum()) and set(np.unique(res)) <= {SYM_ADDED, SYM_ERR}, "n", n, "results", np.unique(res), "added", added)
            books_match(R, L, dq, pk, res, K, n)
            addr2 = None
            if added != len(pk):
                R.rolled_back += added == 0
                again = [x for x, r in zip(pk, res) if r == SYM_ERR]
                if n % 2:
                    a2, r2, addr2 = feed_pinned(L, dq, again, T, oio, asynchronous)
                    R.check(a2 == len(again) and (r2 == SYM_ADDED).all(), "n", n, "the retry stored", a2, "of", len(again))
                else:
                    for t, p in again:
                        R.check(L.nanorq_decoder_add_symbol(dq, (C.c_uint8 * T).from_buffer_copy(p), t, oio) == SYM_ADDED, "n", n, "retry per symbol")
            R.check(L.nanorq_repair_all(dq, oio) == L.nanorq_blocks(dq), "n", n, "repair_all after the retry")
            received_right(R, out, data, pk, where, n)
            L.nanorq_free(dq)
            L.nanorq_pinned_free(addr)
            if addr2:
                L.nanorq_pinned_free(addr2)
            oio.contents.destroy(oio)
            R.collect(n)
        return R.result()

    def repair_all(resident):
        L = capi.api()
        R = Report()
        T, K = 512, 300
        data, c, s, pk, where = packets(6 * K * T, T, K, 0.08, 2, seed=9)
        for n in list(range(1, 60, 2)) + [80, 120, 200]:
            dq = L.nanorq_decoder_new(c, s)
            oio, out = capi.pinned_io(len(data))
            out[:] = 0
            addr = None
            if resident == "device":
                added, res, addr = feed_pinned(L, dq, pk, T, oio)
                R.check(added == len(pk), "n", n, "feed")
            else:
                for t, p in pk:
                    R.check(L.nanorq_decoder_add_symbol(dq, (C.c_uint8 * T).from_buffer_copy(p), t, oio) == SYM_ADDED, "n", n, "feed")
            before = faults()
            opt("fail_after", n)
            done = L.nanorq_repair_all(dq, oio)
            opt("fail_after", 0)
            R.hit += faults() > before
            R.check(done <= L.nanorq_blocks(dq), "n", n, "done", done)
            complete = {b for b in range(L.nanorq_blocks(dq)) if L.nanorq_num_missing(dq, b) == 0}
            received_right(R, out, data, pk, where, n, blocks=complete)
            R.check(L.nanorq_repair_all(dq, oio) == L.nanorq_blocks(dq), "n", n, "the second repair_all")
            received_right(R, out, data, pk, where, n)
            L.nanorq_free(dq)
            if addr:
                L.nanorq_pinned_free(addr)
            oio.contents.destroy(oio)
            R.collect(n)
        return R.result()

    def per_block():
        L = capi.api()
        R = Report()
        T, K = 128, 200
        data, c, s, pk, where = packets(3 * K * T, T, K, 0.1, 2, seed=31)
        for n in range(1, 30):
            rq = L.nanorq_encoder_new_ex(len(data), T, K, 0, 8)
            io = capi.mem_io(data)
            before = faults()
            opt("fail_after", n)
            ok = L.nanorq_generate_symbols(rq, 1, io)
            buf = (C.c_uint8 * T)()
            got = L.nanorq_encode(rq, buf, K + 1, 1, io) if ok else 0
            opt("fail_after", 0)
            R.hit += faults() > before
            if not ok or got != T:
                R.check(got in (0, T), "n", n, "nanorq_encode gave", got)
                R.check(L.nanorq_encode(rq, buf, K + 1, 1, io) == T, "n", n, "the retry of nanorq_encode")
            # a source symbol of the solved block comes back by copies alone
            R.check(L.nanorq_encode(rq, buf, 3, 1, io) == T and bytes(buf) == data[(K + 3) * T:(K + 4) * T].tobytes(), "n", n, "source symbol")
            L.nanorq_free(rq)
            io.contents.destroy(io)
            dq = L.nanorq_decoder_new(c, s)
            out = np.zeros(len(data), np.uint8)
            oio = capi.mem_io(out)
            for t, p in pk:
                L.nanorq_decoder_add_symbol(dq, (C.c_uint8 * T).from_buffer_copy(p), t, oio)
            before = faults()
            opt("fail_after", n)
            ok0 = L.nanorq_repair_block(dq, oio, 0)
            opt("fail_after", 0)
            R.hit += faults() > before
            if not ok0:
                R.check(L.nanorq_num_missing(dq, 0) > 0, "n", n, "a failed repair_block left no gaps")
            for b in range(3):
                R.check(L.nanorq_repair_block(dq, oio, b), "n", n, "block", b, "the retry of repair_block")
            received_right(R, out, data, pk, where, n)
            L.nanorq_free(dq)
            oio.contents.destroy(oio)
            R.collect(n)
        return R.result()

    def repair_rows():
        L = capi.api()
        R = Report()
        T, K = 64, 400
        data, c, s, pk, where = packets(K * T, T, K, 0.5, 4, seed=7)
        src = [(t, p) for t, p in pk if (t & 0xFFFFFF) < K]
        rep = [(t, p) for t, p in pk if (t & 0xFFFFFF) >= K]
        for n in range(1, 24):
            dq = L.nanorq_decoder_new(c, s)
            oio, out = capi.pinned_io(len(data))
            out[:] = 0
            a1, r1, addr1 = feed_pinned(L, dq, src + rep[:40], T, oio)
            R.check(a1 == len(src) + 40, "n", n, "first batch")
            before = faults()
            opt("fail_after", n)
            a2, r2, addr2 = feed_pinned(L, dq, rep[40:], T, oio)
            opt("fail_after", 0)
            R.hit += faults() > before
            if a2 != len(rep) - 40:
                R.check(a2 == 0 and (r2 == SYM_ERR).all() and L.nanorq_num_repair(dq, 0) == 40, "n", n, "a failed batch counted", a2)
                R.rolled_back += 1
                L.nanorq_pinned_free(addr2)
                a2, r2, addr2 = feed_pinned(L, dq, rep[40:], T, oio)
                R.check(a2 == len(rep) - 40, "n", n, "the retry stored", a2)
            R.check(L.nanorq_repair_all(dq, oio) == 1, "n", n, "repair_all")
            received_right(R, out, data, pk, where, n)
            L.nanorq_free(dq)
            L.nanorq_pinned_free(addr1)
            L.nanorq_pinned_free(addr2)
            oio.contents.destroy(oio)
            R.collect(n)
        return R.result()

    def host_block_in_a_deferred_chunk():
        L = capi.api()
        R = Report()
        T, K, Z = 1280, 500, 6
        data, c, s, pk, where = packets(Z * K * T, T, K, 0.1, 2, seed=15)
        for it in range(3):
            dq = L.nanorq_decoder_new(c, s)
            oio, out = capi.pinned_io(len(data))
            out[:] = 0
            for t, p in [x for x in pk if x[0] >> 24 == 0]:
                R.check(L.nanorq_decoder_add_symbol(dq, (C.c_uint8 * T).from_buffer_copy(p), t, oio) == SYM_ADDED, "feed")
            rest = [x for x in pk if x[0] >> 24 != 0]
            n, res, addr = feed_pinned(L, dq, rest, T, oio, asynchronous=True)
            R.check(n == len(rest), "async batch stored", n)
            R.check(L.nanorq_repair_all(dq, oio) == Z, "repair_all")
            received_right(R, out, data, pk, where, it)
            L.nanorq_free(dq)
            L.nanorq_pinned_free(addr)
            oio.contents.destroy(oio)
            R.collect(it)
        return R.result()

    def rows_grown_under_a_deferred_batch():
        L = capi.api()
        R = Report()
        T, K = 1280, 2000
        data, c, s, pk, where = packets(2 * K * T, T, K, 0.3, 3, seed=4)
        for it in range(3):
            dq = L.nanorq_decoder_new(c, s)
            oio, out = capi.pinned_io(len(data))
            out[:] = 0
            rep = [x for x in pk if (x[0] & 0xFFFFFF) >= K]
            src = [x for x in pk if (x[0] & 0xFFFFFF) < K]
            first = src + [x for i, x in enumerate(rep) if i % 3 == 0]
            second = [x for i, x in enumerate(rep) if i % 3 != 0]
            n1, _, a1 = feed_pinned(L, dq, first, T, oio, asynchronous=True)
            n2, _, a2 = feed_pinned(L, dq, second, T, oio, asynchronous=True)
            R.check(n1 == len(first) and n2 == len(second), "async batches stored", n1, n2)
            R.check(L.nanorq_repair_all(dq, oio) == 2, "repair_all")
            received_right(R, out, data, pk, where, it)
            L.nanorq_free(dq)
            L.nanorq_pinned_free(a1)
            L.nanorq_pinned_free(a2)
            oio.contents.destroy(oio)
            R.collect(it)
        return R.result()

    SCENARIOS = {
        "batch_sync": lambda: batch(False),
        "batch_async": lambda: batch(True),
        "repair_all_device": lambda: repair_all("device"),
        "repair_all_host": lambda: repair_all("host"),
        "per_block": per_block,
        "repair_rows": repair_rows,
        "host_block_in_a_deferred_chunk": host_block_in_a_deferred_chunk,
        "rows_grown_under_a_deferred_batch": rows_grown_under_a_deferred_batch,
    }

    def group_faults(names=None):
        W.model()
        W.hazards()
        out = {k: f() for k, f in SCENARIOS.items() if names is None or k in names}
        out["pending_at_end"] = W.model().hm_pending_total()
        out["counters"] = W.counters()
        return out

    def group_process():
        """the process that faulted: the object layer's fault sweeps, then the fuzz calls on fresh contexts in the same process"""
        out = {"faults": group_faults()}
        import gpu_support
        gpu_support._CTXS.clear()
        out["fuzz0"] = W.fuzz0()
        out["hazards"] = W.brief(W.hazards())
        out["counters"] = W.counters()
        return out

    g = {"faults": group_faults, "process": group_process}
    for k in SCENARIOS:
        g["faults:" + k] = (lambda k=k: group_faults((k,)))
    return g
