"""ctypes binding of libnanorq_hip.so (include/nanorq_hip.h)."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class NrqError(RuntimeError):
    pass


class ObjParams(C.Structure):
    """nrq_obj_params (include/nanorq_hip.h): an object's partition into blocks and sub-blocks, K' per class, max_esi, OTI"""
    _fields_ = [("F", C.c_uint64)] + [(n, C.c_uint32) for n in
                                       ("T", "Al", "Z", "N", "Kt", "ZL", "KL", "KpL", "ZS", "KS", "KpS", "NL", "TL", "NS", "TS",
                                        "flags", "max_esi")] + [("oti_common", C.c_uint64), ("oti_specific", C.c_uint32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class CallStats(C.Structure):
    _fields_ = [("plan_ms", C.c_double), ("host_ms", C.c_double), ("strip_bytes", C.c_uint32),
                ("lds_bytes", C.c_uint32), ("grid", C.c_uint32), ("planner", C.c_uint32),
                ("plan_bytes", C.c_uint64), ("xor_ops", C.c_uint64), ("npiv", C.c_uint32), ("u", C.c_uint32),
                ("nlev", C.c_uint32), ("nfree", C.c_uint32), ("wg_threads", C.c_uint32), ("strips_per_slot", C.c_uint32),
                ("wg_waves_per_simd", C.c_uint32), ("host_planned", C.c_uint32), ("movers_aligned", C.c_uint32),
                ("plan_ahead", C.c_uint32), ("strip_bytes_b", C.c_uint32), ("blocks_b", C.c_uint32),
                ("plan_wg_threads", C.c_uint32), ("plan_compact_state", C.c_uint32), ("plan_segmented", C.c_uint32),
                ("backsub_strip", C.c_uint32), ("encplan_device", C.c_uint32), ("out_view", C.c_uint32),
                ("need_view", C.c_uint32), ("nneed", C.c_uint32), ("plan_scan_lists", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def lib_path():
    return os.path.join(_HERE, "libnanorq_hip.so")


def lib():
    """Load the native library (building it first if the sources are newer). No fallback."""
    global _LIB
    if _LIB is not None:
        return _LIB
    from . import build
    path = os.environ.get("NANORQ_HIP_LIB") or build.build_lib()  # the override loads a tuning variant of the same library
    L = C.CDLL(path)
    vp, u32p, ip = C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_int)
    sz = C.c_size_t
    L.nrq_ctx_create.argtypes = [C.c_int, vp, C.POINTER(vp)]
    L.nrq_ctx_destroy.argtypes = [vp]
    L.nrq_ctx_destroy.restype = None
    L.nrq_ctx_set_stream.argtypes = [vp, vp]
    L.nrq_ctx_error.argtypes = [vp]
    L.nrq_ctx_error.restype = C.c_char_p
    L.nrq_ctx_sync.argtypes = [vp]
    L.nrq_ctx_last_stats.argtypes = [vp, C.POINTER(CallStats)]
    L.nrq_ctx_last_stats.restype = None
    L.nrq_ctx_set_threads.argtypes = [vp, C.c_int]
    L.nrq_ctx_set_planner.argtypes = [vp, C.c_int]
    L.nrq_ctx_set_option.argtypes = [vp, C.c_char_p, C.c_longlong]
    L.nrq_params.argtypes = [C.c_uint32, u32p]
    L.nrq_precalculate.argtypes = [vp, C.c_uint32, C.c_uint32]
    L.nrq_plan_cache_clear.argtypes = [vp]
    L.nrq_plan_cache_clear.restype = None
    L.nrq_encode_blocks.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, sz, vp, sz, C.c_uint32, u32p, vp, sz]
    L.nrq_decode_blocks.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, sz, u32p, u32p, C.c_uint32, u32p,
                                    u32p, C.c_uint32, vp, sz, vp, sz, ip]
    L.nrq_decode_blocks_lazy.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, sz, u32p, u32p, C.c_uint32,
                                         u32p, u32p, u32p, C.c_uint32, vp, sz, vp, sz, ip, u32p]
    L.nrq_decode_plan_ahead.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, sz, u32p, u32p, C.c_uint32,
                                        u32p, u32p, u32p, C.c_uint32, vp, sz, vp, sz]
    L.nrq_gen_symbols.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, sz, C.c_uint32, u32p, vp, sz]
    L.nrq_dev_alloc.argtypes = [vp, sz, C.POINTER(vp)]
    L.nrq_dev_free.argtypes = [vp, vp]
    if hasattr(L, "nrq_dev_pool_books"):  # (NANORQ_HIP_LIB may name a build from before the pool's books were readable)
        L.nrq_dev_pool_books.argtypes = [vp, C.POINTER(sz)]
    L.nrq_dev_trim.argtypes = [vp]
    L.nrq_dev_upload.argtypes = [vp, vp, vp, sz]
    L.nrq_dev_download.argtypes = [vp, vp, vp, sz]
    L.nrq_dev_memset.argtypes = [vp, vp, C.c_int, sz]
    L.nrq_ktime_enable.argtypes = [vp, C.c_int]
    L.nrq_ktime_read.argtypes = [vp, C.POINTER(C.c_float), C.c_uint32, u32p]
    L.nrq_ptime_read.argtypes = [vp, C.POINTER(C.c_float), C.c_uint32, u32p]
    L.nrq_ktime_read_intervals.argtypes = [vp, vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_uint32, u32p]
    L.nrq_timer_start.argtypes = [vp]
    L.nrq_timer_stop_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.nrq_rx_create.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, sz, vp, sz,
                                C.POINTER(vp)]
    L.nrq_rx_destroy.argtypes = [vp]
    L.nrq_rx_destroy.restype = None
    L.nrq_rx_add.argtypes = [vp, vp, sz, vp, C.c_uint32, C.c_uint32, vp]
    L.nrq_rx_counts.argtypes = [vp, u32p, u32p]
    L.nrq_rx_lists.argtypes = [vp, u32p, u32p, u32p, u32p]
    L.nrq_rx_decode.argtypes = [vp, ip, u32p]
    L.nrq_rx_src.argtypes = [vp]
    L.nrq_rx_src.restype = vp
    L.nrq_rx_rep.argtypes = [vp]
    L.nrq_rx_rep.restype = vp
    L.nrq_rx_reset.argtypes = [vp]
    L.nrq_tx_create.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, sz, C.POINTER(vp)]
    L.nrq_tx_destroy.argtypes = [vp]
    L.nrq_tx_destroy.restype = None
    L.nrq_tx_encode.argtypes = [vp]
    L.nrq_tx_emit.argtypes = [vp, vp, C.c_uint32, vp, sz, C.c_uint32, vp]
    L.nrq_tx_emit_range.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_int, vp, sz, C.c_uint32, vp]
    L.nrq_tx_inter.argtypes = [vp]
    L.nrq_tx_inter.restype = vp
    opp = C.POINTER(ObjParams)
    L.nrq_obj_params_enc.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, opp]
    L.nrq_obj_params_oti.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, opp]
    L.nrq_obj_layout.argtypes = [vp, opp, vp, vp, C.c_int]
    L.nrq_otx_create.argtypes = [vp, opp, vp, C.POINTER(vp)]
    L.nrq_otx_destroy.argtypes = [vp]
    L.nrq_otx_destroy.restype = None
    L.nrq_otx_encode.argtypes = [vp]
    L.nrq_otx_emit.argtypes = [vp, vp, C.c_uint32, vp, sz, C.c_uint32, vp]
    L.nrq_otx_emit_all.argtypes = [vp, C.c_uint32, C.c_int, vp, sz, C.c_uint32, vp]
    L.nrq_otx_oti.argtypes = [vp, C.POINTER(C.c_uint64), u32p]
    L.nrq_orx_create.argtypes = [vp, opp, C.c_uint32, C.POINTER(vp)]
    L.nrq_orx_destroy.argtypes = [vp]
    L.nrq_orx_destroy.restype = None
    L.nrq_orx_add.argtypes = [vp, vp, sz, vp, C.c_uint32, C.c_uint32, vp]
    L.nrq_orx_counts.argtypes = [vp, u32p, u32p]
    L.nrq_orx_decode.argtypes = [vp, ip, u32p]
    L.nrq_orx_write.argtypes = [vp, vp]
    if hasattr(L, "nrq_rx_relay"):  # (NANORQ_HIP_LIB may name a build from before the relays: A/B runs against it; relay() then raises)
        L.nrq_tx_ready.argtypes = [vp, u32p]
        L.nrq_rx_relay.argtypes = [vp, C.POINTER(vp)]
        L.nrq_otx_ready.argtypes = [vp, u32p]
        L.nrq_orx_relay.argtypes = [vp, C.POINTER(vp)]
    if hasattr(L, "nrq_rx_held"):  # (likewise a build from before the held symbols: held() then raises, held=True is refused)
        L.nrq_rx_held.argtypes = [vp, vp, C.c_uint32, u32p]
        L.nrq_orx_held.argtypes = [vp, vp, C.c_uint32, u32p]
    if hasattr(L, "nrq_rx_want"):  # (likewise a build from before the want listing: want() then raises)
        L.nrq_rx_want.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_uint32, u32p]
        L.nrq_orx_want.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_uint32, u32p]
    if hasattr(L, "nrq_rxset_create"):  # (likewise a build from before the reception sets: ReceiverSet then raises)
        L.nrq_rxset_create.argtypes = [vp, C.c_uint32, C.POINTER(vp)]
        L.nrq_rxset_destroy.argtypes = [vp]
        L.nrq_rxset_destroy.restype = None
        L.nrq_rxset_attach.argtypes = [vp, C.c_uint32, vp]
        L.nrq_rxset_attach_obj.argtypes = [vp, C.c_uint32, vp]
        L.nrq_rxset_detach.argtypes = [vp, C.c_uint32]
        L.nrq_rxset_add.argtypes = [vp, vp, sz, vp, vp, C.c_uint32, C.c_uint32, vp]
    if hasattr(L, "nrq_rxset_decode"):  # (likewise a build from before the set-wide counts, lists and decode: those methods then raise)
        L.nrq_rxset_blocks.argtypes = [vp, u32p, u32p, C.c_uint32, u32p]
        L.nrq_rxset_counts.argtypes = [vp, u32p, u32p]
        L.nrq_rxset_lists.argtypes = [vp, u32p, u32p, u32p, sz, C.POINTER(sz)]
        L.nrq_rxset_decode.argtypes = [vp, ip, u32p]
    if hasattr(L, "nrq_rxset_want"):  # (likewise a build from before the set-wide want and held listings: those methods then raise)
        L.nrq_rxset_want.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, C.c_uint32, u32p, u32p]
        L.nrq_rxset_held.argtypes = [vp, vp, vp, C.c_uint32, u32p, u32p]
    if hasattr(L, "nrq_txset_create"):  # (likewise a build from before the sender sets: SenderSet then raises)
        L.nrq_txset_create.argtypes = [vp, C.c_uint32, C.POINTER(vp)]
        L.nrq_txset_destroy.argtypes = [vp]
        L.nrq_txset_destroy.restype = None
        L.nrq_txset_attach.argtypes = [vp, C.c_uint32, vp]
        L.nrq_txset_attach_obj.argtypes = [vp, C.c_uint32, vp]
        L.nrq_txset_detach.argtypes = [vp, C.c_uint32]
        L.nrq_txset_blocks.argtypes = [vp, u32p, u32p, C.c_uint32, u32p]
        L.nrq_txset_emit.argtypes = [vp, vp, vp, C.c_uint32, vp, sz, C.c_uint32, vp]
    if hasattr(L, "nrq_rx_add_syms"):  # (likewise a build from before the packets of several symbols: the *_syms methods then raise)
        u32 = C.c_uint32
        L.nrq_pkt_count.argtypes = [u32, u32, u32, u32]
        L.nrq_pkt_count.restype = u32
        L.nrq_rx_add_syms.argtypes = [vp, vp, sz, vp, u32, u32, vp, u32, vp]
        L.nrq_orx_add_syms.argtypes = [vp, vp, sz, vp, u32, u32, vp, u32, vp]
        L.nrq_tx_emit_syms.argtypes = [vp, vp, u32, u32, vp, vp, sz, u32, vp]
        L.nrq_otx_emit_syms.argtypes = [vp, vp, u32, u32, vp, vp, sz, u32, vp]
        L.nrq_tx_emit_range_syms.argtypes = [vp, u32, u32, u32, C.c_int, vp, sz, u32, vp, vp, u32p]
        L.nrq_otx_emit_all_syms.argtypes = [vp, u32, u32, C.c_int, vp, sz, u32, vp, vp, u32p]
    if hasattr(L, "nrq_rxset_add_syms"):  # (likewise a build from before the sets' packets of several symbols: those methods then raise)
        u32 = C.c_uint32
        L.nrq_rxset_add_syms.argtypes = [vp, vp, sz, vp, vp, u32, u32, vp, u32, vp]
        L.nrq_txset_emit_syms.argtypes = [vp, vp, vp, u32, u32, vp, vp, sz, u32, vp]
    if hasattr(L, "nrq_txset_emit_all"):  # (likewise a build from before the sets' range mode: count_all / emit_all then raise)
        u32 = C.c_uint32
        L.nrq_txset_count_all.argtypes = [vp, u32, u32, u32, u32p, u32p]
        L.nrq_txset_emit_all.argtypes = [vp, u32, u32, u32, C.c_int, vp, sz, u32, vp, vp, u32p]
        L.nrq_txset_emit_all_syms.argtypes = [vp, u32, u32, u32, u32, C.c_int, vp, sz, u32, vp, vp, vp, u32p]
    if hasattr(L, "nrq_rx_want_syms"):  # (likewise a build from before the listings as runs: want_syms / held_syms then raise)
        u32 = C.c_uint32
        L.nrq_rx_want_syms.argtypes = [vp, u32, u32, u32, u32, vp, vp, u32, u32p, u32p]
        L.nrq_orx_want_syms.argtypes = [vp, u32, u32, u32, u32, vp, vp, u32, u32p, u32p]
        L.nrq_rx_held_syms.argtypes = [vp, u32, vp, vp, u32, u32p, u32p]
        L.nrq_orx_held_syms.argtypes = [vp, u32, vp, vp, u32, u32p, u32p]
    if hasattr(L, "nrq_rxset_want_syms"):  # (likewise a build from before the sets' listings as runs: those methods then raise)
        u32 = C.c_uint32
        L.nrq_rxset_want_syms.argtypes = [vp, u32, u32, u32, u32, vp, vp, vp, u32, u32p, u32p, u32p]
        L.nrq_rxset_held_syms.argtypes = [vp, u32, vp, vp, vp, u32, u32p, u32p, u32p]
    u8pp = C.POINTER(C.POINTER(C.c_uint8))
    L.nrq_host_kconst_build.argtypes = [C.c_uint32, u8pp, u32p]
    L.nrq_host_plan_build.argtypes = [C.c_uint32, C.c_uint32, u32p, C.POINTER(C.c_uint8), u8pp, u32p]
    L.nrq_host_plan_build_forced.argtypes = [C.c_uint32, C.c_uint32, u32p, C.POINTER(C.c_uint8), u8pp, u32p, C.c_uint32]
    L.nrq_host_free.argtypes = [vp]
    L.nrq_host_free.restype = None
    _LIB = L
    return L


PARAM_NAMES = ("Kp", "J", "S", "H", "W", "L", "P", "P1", "U", "B")
PLAN_FIELDS = ("magic status K Kp J S H W L P P1 B M npiv u nlow r2 nfree nlev nrows pipe wpr "
               "npiv_pad n_xor_ops off_ops off_pivslot off_pivcol off_wt off_lowslot off_pivx off_fbits "
               "off_mh off_freex off_hinv off_colslot off_pivof off_uslot total_bytes reserved0 reserved1 fail_site "
               "off_augt lpr aug_stride nneed need_pad off_needslot off_wneed off_wout out_pad out_n off_out_cptr "
               "off_out_slots scan_lists").split()


def params(K):
    out = (C.c_uint32 * 10)()
    if lib().nrq_params(K, out) != 0:
        raise ValueError("K out of range: %r" % (K,))
    return dict(zip(PARAM_NAMES, (int(x) for x in out)))


def _u32(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def host_kconst(K):
    """Per-K' HDPC constants arena (bytes)."""
    out = C.POINTER(C.c_uint8)()
    n = C.c_uint32()
    if lib().nrq_host_kconst_build(K, C.byref(out), C.byref(n)) != 0:
        raise NrqError("kconst build failed")
    buf = bytes(C.string_at(out, n.value))
    lib().nrq_host_free(out)
    return buf


def host_plan(K, isis, kconst, extra_inact=0):
    """Host planner: returns the plan arena as bytes (header status tells solvable/singular).  extra_inact (tests): that many
    columns more are inactive before peeling begins -- the same system and solution at a chosen number of inactive columns."""
    isis = np.ascontiguousarray(isis, dtype=np.uint32)
    kc = (C.c_uint8 * len(kconst)).from_buffer_copy(kconst)
    out = C.POINTER(C.c_uint8)()
    n = C.c_uint32()
    rc = lib().nrq_host_plan_build_forced(K, len(isis), _u32(isis), kc, C.byref(out), C.byref(n), int(extra_inact))
    if rc != 0:
        raise NrqError("plan build failed: %d" % rc)
    buf = bytes(C.string_at(out, n.value))
    lib().nrq_host_free(out)
    return buf


def plan_header(plan):
    h = np.frombuffer(plan, dtype=np.uint32, count=len(PLAN_FIELDS))
    return dict(zip(PLAN_FIELDS, (int(x) for x in h)))


class Context:
    """One per GPU.  Device buffers are plain integers (device addresses): pass torch tensor
    data_ptr()s, or use alloc()/upload()/download()."""

    def __init__(self, device=0, stream=None):
        self._L = lib()
        h = C.c_void_p()
        rc = self._L.nrq_ctx_create(device, C.c_void_p(stream or 0), C.byref(h))
        if rc != 0:
            raise NrqError("nrq_ctx_create failed (%d): no usable HIP device -- the HIP path has no CPU fallback" % rc)
        self._h = h
        self.device = device
        self._stream = int(stream or 0)
        self._tstream = None

    def close(self):
        if getattr(self, "_h", None):
            self._L.nrq_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise NrqError("%s (rc=%d)" % (self._L.nrq_ctx_error(self._h).decode(), rc))

    def set_stream(self, stream):
        self._chk(self._L.nrq_ctx_set_stream(self._h, C.c_void_p(stream or 0)))
        self._stream = int(stream or 0)
        self._tstream = None

    def torch_stream(self):
        """The context's stream as a torch stream (0: torch's default stream, which is the null stream)."""
        if self._tstream is None:
            import torch
            self._tstream = (torch.cuda.ExternalStream(self._stream, device=self.device) if self._stream
                             else torch.cuda.default_stream(self.device))
        return self._tstream

    def new_tensor(self, shape, dtype, zero=False):
        """A device tensor of the binding's own, allocated (and zeroed) ON THE CONTEXT'S STREAM whatever torch's current stream
        is: the library's next write to it on that stream comes after the allocator's last use of the block and after the fill."""
        import torch
        with torch.cuda.stream(self.torch_stream()):
            return (torch.zeros if zero else torch.empty)(shape, dtype=dtype, device="cuda:%d" % self.device)

    def set_planner(self, device=True):
        self._chk(self._L.nrq_ctx_set_planner(self._h, int(bool(device))))

    def set_option(self, name, value):
        self._chk(self._L.nrq_ctx_set_option(self._h, name.encode(), int(value)))

    def set_threads(self, n):
        self._chk(self._L.nrq_ctx_set_threads(self._h, n))

    def sync(self):
        self._chk(self._L.nrq_ctx_sync(self._h))

    def stats(self):
        s = CallStats()
        self._L.nrq_ctx_last_stats(self._h, C.byref(s))
        return s.as_dict()

    def precalculate(self, K, Kp=0):
        self._chk(self._L.nrq_precalculate(self._h, K, Kp))

    def clear_plan_cache(self):
        self._L.nrq_plan_cache_clear(self._h)

    # -- raw device memory -------------------------------------------------------------------
    def alloc(self, nbytes):
        p = C.c_void_p()
        self._chk(self._L.nrq_dev_alloc(self._h, nbytes, C.byref(p)))
        return p.value

    def free(self, ptr):
        self._chk(self._L.nrq_dev_free(self._h, C.c_void_p(ptr)))

    def upload(self, dptr, arr):
        arr = np.ascontiguousarray(arr)
        self._chk(self._L.nrq_dev_upload(self._h, C.c_void_p(dptr), arr.ctypes.data_as(C.c_void_p), arr.nbytes))

    def download(self, dptr, nbytes):
        out = np.empty(nbytes, np.uint8)
        self._chk(self._L.nrq_dev_download(self._h, out.ctypes.data_as(C.c_void_p), C.c_void_p(dptr), nbytes))
        return out

    def memset(self, dptr, value, nbytes):
        self._chk(self._L.nrq_dev_memset(self._h, C.c_void_p(dptr), value, nbytes))

    # -- hot path ----------------------------------------------------------------------------
    def encode_blocks(self, K, T, nblk, d_src, src_stride, d_rep, rep_stride, esis, d_inter=0, inter_stride=0, Kp=0):
        esis = np.ascontiguousarray(esis, dtype=np.uint32)
        self._chk(self._L.nrq_encode_blocks(self._h, K, Kp, T, nblk, C.c_void_p(d_src), src_stride,
                                            C.c_void_p(d_inter or 0), inter_stride, len(esis),
                                            _u32(esis) if len(esis) else None, C.c_void_p(d_rep or 0), rep_stride))

    def decode_blocks(self, K, T, nblk, d_src, src_stride, lost, nlost, rep_esi, nrep, d_rep, rep_stride,
                      d_inter=0, inter_stride=0, Kp=0):
        """lost: [nblk, lost_cap] uint32, rep_esi: [nblk, rep_cap] uint32. Returns status int array."""
        lost = np.ascontiguousarray(lost, dtype=np.uint32).reshape(nblk, -1)
        rep_esi = np.ascontiguousarray(rep_esi, dtype=np.uint32).reshape(nblk, -1)
        nlost = np.ascontiguousarray(nlost, dtype=np.uint32)
        nrep = np.ascontiguousarray(nrep, dtype=np.uint32)
        status = np.zeros(nblk, dtype=np.int32)
        self._chk(self._L.nrq_decode_blocks(self._h, K, Kp, T, nblk, C.c_void_p(d_src), src_stride, _u32(lost),
                                            _u32(nlost), lost.shape[1], _u32(rep_esi), _u32(nrep), rep_esi.shape[1],
                                            C.c_void_p(d_rep or 0), rep_stride, C.c_void_p(d_inter or 0),
                                            inter_stride, status.ctypes.data_as(C.POINTER(C.c_int))))
        return status

    def decode_blocks_lazy(self, K, T, nblk, d_src, src_stride, lost, nlost, rep_esi, nrep, nrep_avail, d_rep, rep_stride,
                           d_inter=0, inter_stride=0, Kp=0):
        """Like decode_blocks, but block b starts from its first nrep[b] repair symbols and takes more (up to
        nrep_avail[b]) only if its system is rank deficient.  Returns (status, used)."""
        lost = np.ascontiguousarray(lost, dtype=np.uint32).reshape(nblk, -1)
        rep_esi = np.ascontiguousarray(rep_esi, dtype=np.uint32).reshape(nblk, -1)
        nlost = np.ascontiguousarray(nlost, dtype=np.uint32)
        nrep = np.ascontiguousarray(nrep, dtype=np.uint32)
        nrep_avail = np.ascontiguousarray(nrep_avail, dtype=np.uint32)
        status = np.zeros(nblk, dtype=np.int32)
        used = np.zeros(nblk, dtype=np.uint32)
        self._chk(self._L.nrq_decode_blocks_lazy(self._h, K, Kp, T, nblk, C.c_void_p(d_src), src_stride, _u32(lost),
                                                 _u32(nlost), lost.shape[1], _u32(rep_esi), _u32(nrep), _u32(nrep_avail),
                                                 rep_esi.shape[1], C.c_void_p(d_rep or 0), rep_stride,
                                                 C.c_void_p(d_inter or 0), inter_stride,
                                                 status.ctypes.data_as(C.POINTER(C.c_int)), _u32(used)))
        return status, used

    def decode_plan_ahead(self, K, T, nblk, d_src, src_stride, lost, nlost, rep_esi, nrep, nrep_avail, d_rep, rep_stride,
                          d_inter=0, inter_stride=0, Kp=0):
        """Issue the planner run of the decode_blocks_lazy (nrep_avail given) / decode_blocks (None) call with the same
        arguments now; that call then only waits for it."""
        lost = np.ascontiguousarray(lost, dtype=np.uint32).reshape(nblk, -1)
        rep_esi = np.ascontiguousarray(rep_esi, dtype=np.uint32).reshape(nblk, -1)
        nlost = np.ascontiguousarray(nlost, dtype=np.uint32)
        nrep = np.ascontiguousarray(nrep, dtype=np.uint32)
        av = None if nrep_avail is None else np.ascontiguousarray(nrep_avail, dtype=np.uint32)
        self._chk(self._L.nrq_decode_plan_ahead(self._h, K, Kp, T, nblk, C.c_void_p(d_src), src_stride, _u32(lost), _u32(nlost),
                                                lost.shape[1], _u32(rep_esi), _u32(nrep), None if av is None else _u32(av),
                                                rep_esi.shape[1], C.c_void_p(d_rep or 0), rep_stride, C.c_void_p(d_inter or 0),
                                                inter_stride))

    def gen_symbols(self, K, T, nblk, d_inter, inter_stride, isis, d_out, out_stride, Kp=0):
        isis = np.ascontiguousarray(isis, dtype=np.uint32)
        self._chk(self._L.nrq_gen_symbols(self._h, K, Kp, T, nblk, C.c_void_p(d_inter), inter_stride, len(isis),
                                          _u32(isis), C.c_void_p(d_out), out_stride))

    def ktime_enable(self, on=True):
        self._chk(self._L.nrq_ktime_enable(self._h, int(on)))

    def ktime_read(self, cap=65536):
        buf = (C.c_float * cap)()
        n = C.c_uint32()
        self._chk(self._L.nrq_ktime_read(self._h, buf, cap, C.byref(n)))
        return [float(buf[k]) for k in range(min(cap, n.value))]

    def ptime_read(self, cap=65536):
        """durations (ms) of the decode planner runs since ktime_enable"""
        buf = (C.c_float * cap)()
        n = C.c_uint32()
        self._chk(self._L.nrq_ptime_read(self._h, buf, cap, C.byref(n)))
        return [float(buf[k]) for k in range(min(cap, n.value))]

    def ktime_read_intervals(self, ref=None, cap=65536):
        """[(start_ms, dur_ms)] of the solve-kernel launches since ktime_enable, on `ref`'s time axis."""
        a = (C.c_float * cap)()
        b = (C.c_float * cap)()
        n = C.c_uint32()
        self._chk(self._L.nrq_ktime_read_intervals(self._h, (ref or self)._h, a, b, cap, C.byref(n)))
        return [(float(a[k]), float(b[k])) for k in range(min(cap, n.value))]

    def timer_start(self):
        self._chk(self._L.nrq_timer_start(self._h))

    def timer_stop_ms(self):
        ms = C.c_float()
        self._chk(self._L.nrq_timer_stop_ms(self._h, C.byref(ms)))
        return float(ms.value)


RX_TAG_INLINE = 1   # NRQ_RX_TAG_INLINE
RX_FULL = 3         # NRQ_RX_FULL
RX_KEY_INLINE = 2   # NRQ_RX_KEY_INLINE
RXSET_MAX_MEMBERS = 64   # NRQ_RXSET_MAX_MEMBERS
RXSET_MAX_BLOCKS = 1024  # NRQ_RXSET_MAX_BLOCKS
TX_KEY_INLINE = 4        # NRQ_TX_KEY_INLINE
TXSET_MAX_SEGS = 64      # NRQ_TXSET_MAX_SEGS
TXSET_MAX_BLOCKS = 1024  # NRQ_TXSET_MAX_BLOCKS


def _dptr(x):
    """device address of a torch tensor (data_ptr()) or of a raw integer address; None -> 0"""
    if x is None:
        return 0
    return int(x.data_ptr()) if hasattr(x, "data_ptr") else int(x)


class _Handle:
    """The lifecycle of a device handle: close() (also by `with` and on collection) calls the library's <_api>_destroy once."""
    _api = None
    _h = None

    def close(self):
        if self._h and getattr(self.ctx, "_h", None):
            getattr(self._L, self._api + "_destroy")(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Receiver(_Handle):
    """A device-resident reception (nrq_rx, include/nanorq_hip.h): nblk blocks of equal (K, K', T), SBNs sbn0 .. sbn0+nblk-1,
    fed with packets that are already in device memory.  Buffers are torch HIP tensors or raw device addresses.  src None: the
    source rows are a torch tensor of the reception's own (`source`, [nblk, K, T] uint8); rep None: the repair rows come from the
    context's pool."""
    _api = "nrq_rx"

    def __init__(self, ctx, K, T, nblk, rep_cap, sbn0=0, max_esi=0, Kp=0, src=None, src_stride=0, rep=None, rep_stride=0):
        self.ctx = ctx
        self._L = ctx._L
        self.K, self.T, self.nblk, self.rep_cap, self.sbn0 = K, T, nblk, rep_cap, sbn0
        self._source = None
        if src is None:
            import torch
            self._source = ctx.new_tensor((nblk, K, T), torch.uint8)
            src, src_stride = self._source, K * T
        self._keep = (src, rep)  # the tensors stay alive as long as the reception
        h = C.c_void_p()
        ctx._chk(self._L.nrq_rx_create(ctx._h, K, Kp, T, nblk, sbn0, max_esi, rep_cap, C.c_void_p(_dptr(src)), src_stride,
                                       C.c_void_p(_dptr(rep)), rep_stride, C.byref(h)))
        self._h = h

    @property
    def src_ptr(self):
        return self._L.nrq_rx_src(self._h) or 0

    @property
    def rep_ptr(self):
        return self._L.nrq_rx_rep(self._h) or 0

    @property
    def source(self):
        """[nblk, K, T] uint8 tensor of the source rows when the reception was created without `src` (None otherwise)."""
        return self._source

    def add(self, payload, tags=None, inline=False, results=None, n=None, stride=None):
        """Ingest packets (enqueue only).  payload: [n, stride] uint8 tensor (or an address with n and stride); tags: [n] int32 /
        uint32 tensor in nanorq_tag() form, or inline=True when each packet starts with the 4-byte FEC Payload ID; results:
        optional [n] int32 device tensor for the NANORQ_SYM_* / RX_FULL codes."""
        if hasattr(payload, "data_ptr"):
            n = payload.shape[0] if n is None else n
            stride = payload.stride(0) * payload.element_size() if stride is None else stride
        if n is None or stride is None:
            raise ValueError("a raw payload address needs n and stride")
        if inline == (tags is not None):
            raise ValueError("give either tags or inline=True")
        self.ctx._chk(self._L.nrq_rx_add(self._h, C.c_void_p(_dptr(payload)), stride, C.c_void_p(_dptr(tags)), n,
                                         RX_TAG_INLINE if inline else 0, C.c_void_p(_dptr(results))))

    def add_syms(self, payload, G, tags=None, nsym=None, inline=False, results=None, n=None, stride=None):
        """Ingest packets of up to G symbols each (nrq_rx_add_syms; enqueue only): tags / the inline FEC Payload ID name each
        packet's FIRST symbol, nsym ([n] uint8 device tensor, or None for the sender's rule) its count; symbol i of packet k lies
        at hdr + i * T and reports into results[k * G + i] ([n * G] int32 device tensor, optional).  The reception ends in the
        state add() leaves after the one-symbol packets in slot order."""
        _add_syms(self, payload, G, tags, nsym, inline, results, n, stride)

    def counts(self):
        """(missing source symbols, repair rows used) per block, as numpy arrays (waits)."""
        nl = np.zeros(self.nblk, np.uint32)
        nr = np.zeros(self.nblk, np.uint32)
        self.ctx._chk(self._L.nrq_rx_counts(self._h, _u32(nl), _u32(nr)))
        return nl, nr

    def lists(self):
        """(lost, rep_esi): per block the ascending missing source ESIs and the repair ESIs in arrival order (waits)."""
        nl = np.zeros(self.nblk, np.uint32)
        nr = np.zeros(self.nblk, np.uint32)
        lost = np.zeros((self.nblk, self.K), np.uint32)
        resi = np.zeros((self.nblk, self.rep_cap), np.uint32)
        self.ctx._chk(self._L.nrq_rx_lists(self._h, _u32(nl), _u32(nr), _u32(lost), _u32(resi)))
        return [lost[b, :nl[b]].copy() for b in range(self.nblk)], [resi[b, :nr[b]].copy() for b in range(self.nblk)]

    def decode(self):
        """Decode in place; returns (status, used) numpy arrays (1 = block complete; 0 = ingest more and decode again)."""
        st = np.zeros(self.nblk, np.int32)
        used = np.zeros(self.nblk, np.uint32)
        self.ctx._chk(self._L.nrq_rx_decode(self._h, st.ctypes.data_as(C.POINTER(C.c_int)), _u32(used)))
        return st, used

    def reset(self):
        self.ctx._chk(self._L.nrq_rx_reset(self._h))

    def held(self):
        """The tags (nanorq_tag() form) of every symbol the reception holds, as an [n] int32 device tensor listed on the device:
        block-major, per block the seen source ESIs ascending, then the repair ESIs in arrival order (waits).  It is the list
        relay().emit(tags, held=True) writes in full."""
        return _held(self)

    def want(self, extra=0, source=False, esi_from=0):
        """The tags (nanorq_tag() form) the reception asks upstream for, as an [n] int32 device tensor listed on the device,
        block-major and ascending within a block (waits).  Default: per incomplete block the lowest unseen repair ESIs from
        max(K, esi_from), as many as it lacks plus `extra`, less the repair rows it has, at most its free repair rows.
        source=True (WANT_SOURCE): its missing source ESIs -- what parent.emit(tags, held=True) of a relay that is not ready can
        still answer.  A complete block wants nothing.  A block a decode left at status 0 with enough symbols (rank deficient)
        wants nothing until extra exceeds its surplus."""
        return _want(self, extra, source, esi_from)

    def want_syms(self, G, extra=0, source=False, esi_from=0):
        """want() as packets of up to G symbols (nrq_rx_want_syms): (tags int32 [n], nsym uint8 [n]) device tensors, packet k the
        first tag tags[k] and its count nsym[k] -- every run of consecutive ESIs of want()'s list cut into packets of G from its
        start, the last one short.  The form parent.emit_syms(tags, G, nsym, held=...) and add_syms(..., nsym=nsym) take; its
        expansion is want()'s list word for word (waits)."""
        return _list_syms(self, "_want_syms", (WANT_SOURCE if source else 0, extra, esi_from, G))

    def held_syms(self, G):
        """held() as packets of up to G symbols (nrq_rx_held_syms), as want_syms: per block the runs of its seen source ESIs, then
        those of its repair ESIs in arrival order (a run lies in consecutive repair rows).  It is the list
        relay().emit_syms(tags, G, nsym, held=True) writes in full (waits)."""
        return _list_syms(self, "_held_syms", (G,))

    def relay(self):
        """A Sender over this reception's own rows (nrq_rx_relay): it emits any (SBN, ESI) of every block that is ready -- decoded
        while the relay was attached, or complete and made ready by its encode().  One per reception."""
        return RelaySender(self)


PKT_SYMS_MAX = 64  # NRQ_PKT_SYMS_MAX


def _syms_fn(obj, name):
    fn = getattr(obj._L, obj._api + name, None)
    if fn is None or not hasattr(obj._L, "nrq_rx_add_syms"):
        raise NrqError("this build of the library has no packets of several symbols (%s%s)" % (obj._api, name))
    return fn


def _add_syms(rx, payload, G, tags, nsym, inline, results, n, stride):
    if hasattr(payload, "data_ptr"):
        n = payload.shape[0] if n is None else n
        stride = payload.stride(0) * payload.element_size() if stride is None else stride
    if n is None or stride is None:
        raise ValueError("a raw payload address needs n and stride")
    rx.ctx._chk(_syms_fn(rx, "_add_syms")(rx._h, C.c_void_p(_dptr(payload)), stride, C.c_void_p(_dptr(tags)), n, G,
                                          C.c_void_p(_dptr(nsym)), RX_TAG_INLINE if inline else 0, C.c_void_p(_dptr(results))))


def pkt_count(K, esi0, n, G):
    """packets that carry ESIs esi0 .. esi0+n-1 of a block of K source symbols, G symbols a packet (nrq_pkt_count)"""
    return int(lib().nrq_pkt_count(K, esi0, n, G))


def _held(rx):
    """<_api>_held: the count first, then the tags into a tensor of that size"""
    import torch
    n = C.c_uint32(0)
    fn = getattr(rx._L, rx._api + "_held")
    rx.ctx._chk(fn(rx._h, None, 0, C.byref(n)))
    out = rx.ctx.new_tensor(n.value, torch.int32)
    if n.value:
        rx.ctx._chk(fn(rx._h, C.c_void_p(_dptr(out)), n.value, C.byref(n)))
        rx.ctx.sync()  # (torch's stream and the library's are not ordered: the list is complete on return)
    return out


WANT_SOURCE = 1     # NRQ_WANT_SOURCE


def _want(rx, extra, source, esi_from):
    """<_api>_want: the count first, then the tags into a tensor of that size"""
    import torch
    n = C.c_uint32(0)
    fn = getattr(rx._L, rx._api + "_want")
    args = (WANT_SOURCE if source else 0, extra, esi_from)
    rx.ctx._chk(fn(rx._h, *args, None, 0, C.byref(n)))
    out = rx.ctx.new_tensor(n.value, torch.int32)
    if n.value:
        rx.ctx._chk(fn(rx._h, *args, C.c_void_p(_dptr(out)), n.value, C.byref(n)))
        rx.ctx.sync()  # (torch's stream and the library's are not ordered: the list is complete on return)
    return out


def _list_syms(rx, name, args):
    """<_api>_want_syms / <_api>_held_syms: the counts first, then the packets into two tensors of that size"""
    import torch
    fn = getattr(rx._L, rx._api + name, None)
    if fn is None:
        raise NrqError("this build of the library has no listings in packets of several symbols (%s%s)" % (rx._api, name))
    npkt = C.c_uint32(0)
    rx.ctx._chk(fn(rx._h, *args, None, None, 0, C.byref(npkt), None))
    tags = rx.ctx.new_tensor(npkt.value, torch.int32)
    nsym = rx.ctx.new_tensor(npkt.value, torch.uint8)
    if npkt.value:
        rx.ctx._chk(fn(rx._h, *args, C.c_void_p(_dptr(tags)), C.c_void_p(_dptr(nsym)), npkt.value, C.byref(npkt), None))
        rx.ctx.sync()  # (torch's stream and the library's are not ordered: the list is complete on return)
    return tags, nsym


TX_TAG_INLINE = 1   # NRQ_TX_TAG_INLINE
TX_HELD = 2         # NRQ_TX_HELD
TX_NOT_READY = -2   # NRQ_TX_NOT_READY
TX_BAD_RANGE = -3   # NRQ_TX_BAD_RANGE


def _tx_flags(inline, held):
    return (TX_TAG_INLINE if inline else 0) | (TX_HELD if held else 0)


class _Emitter(_Handle):
    """What Sender and ObjectSender share: the packet buffers, encode and the tag-list emit (<_api>_encode, <_api>_emit)."""

    def stride(self, inline=False):
        """the packet stride of out=None: T, or T + 4 rounded up to 16 with the inline header"""
        return (self.T + 4 + 15) // 16 * 16 if inline else self.T

    def _out(self, n, inline, out):
        if out is not None:
            return out, out.stride(0) * out.element_size()
        import torch
        out = self.ctx.new_tensor((n, self.stride(inline)), torch.uint8)
        return out, out.shape[1]

    def encode(self):
        """solve every block (the intermediate symbols stay in device memory); needed before any emit"""
        self.ctx._chk(getattr(self._L, self._api + "_encode")(self._h))

    def emit(self, tags, out=None, inline=False, results=None, held=False):
        """Packet k for tags[k] ([n] int32 / uint32 device tensor, nanorq_tag() form) in row k of out ([n, stride] uint8 device
        tensor; None: a new one).  results: optional [n] int32 device tensor (0 written, -1 SBN outside the transmission or the
        object, whose packet is left untouched; a relay: TX_NOT_READY for a block that is not ready, likewise untouched).
        held (relays only; a sender refuses it): a block that is not ready still gives the symbols its reception holds
        (TX_HELD), as copies of the rows they were ingested into.  Returns out."""
        n = int(tags.shape[0])
        out, stride = self._out(n, inline, out)
        self.ctx._chk(getattr(self._L, self._api + "_emit")(self._h, C.c_void_p(_dptr(tags)), n, C.c_void_p(_dptr(out)), stride,
                                                            _tx_flags(inline, held), C.c_void_p(_dptr(results))))
        return out

    def stride_syms(self, G, inline=False):
        """the packet stride of out=None for packets of G symbols: G * T, or G * T + 4 rounded up to 16 with the inline header"""
        return (G * self.T + 4 + 15) // 16 * 16 if inline else G * self.T

    def _out_syms(self, n, G, inline, out):
        if out is not None:
            return out, out.stride(0) * out.element_size()
        import torch
        out = self.ctx.new_tensor((n, self.stride_syms(G, inline)), torch.uint8)
        return out, out.shape[1]

    def emit_syms(self, tags, G, nsym=None, out=None, inline=False, results=None, held=False):
        """Packet k of up to G symbols for the first tag tags[k] in row k of out (<_api>_emit_syms): nsym[k] symbols ([n] uint8
        device tensor), or by the sender's rule with nsym None -- G, but a packet of source symbols ends with the block's last
        one.  results: optional [n] int32 device tensor (0, -1, TX_NOT_READY, TX_BAD_RANGE; only a 0 packet is written, and
        whole).  held (relays only; a sender refuses it): a packet of a block that is not ready is still written when its
        reception holds EVERY one of its symbols (TX_HELD) -- all or nothing, else TX_NOT_READY; what Receiver.held_syms lists is
        written in full.  Returns out."""
        n = int(tags.shape[0])
        out, stride = self._out_syms(n, G, inline, out)
        self.ctx._chk(_syms_fn(self, "_emit_syms")(self._h, C.c_void_p(_dptr(tags)), n, G, C.c_void_p(_dptr(nsym)), C.c_void_p(_dptr(out)),
                                                   stride, _tx_flags(inline, held), C.c_void_p(_dptr(results))))
        return out

    def _range_syms(self, fn, head, npkt, G, interleave, inline, out):
        import torch
        out, stride = self._out_syms(npkt, G, inline, out)
        # (no fill: the call writes the first tag and the count of every one of its npkt packets, and a fill on torch's current
        # stream would not be ordered against that write on the context's)
        tags = self.ctx.new_tensor(npkt, torch.int32)
        nsym = self.ctx.new_tensor(npkt, torch.uint8)
        got = C.c_uint32()
        self.ctx._chk(fn(self._h, *head, G, 1 if interleave else 0, C.c_void_p(_dptr(out)), stride, _tx_flags(inline, False),
                         C.c_void_p(_dptr(tags)), C.c_void_p(_dptr(nsym)), C.byref(got)))
        assert got.value == npkt, (got.value, npkt)
        return out, tags, nsym


class Sender(_Emitter):
    """A device-resident transmission (nrq_tx, include/nanorq_hip.h): nblk blocks of equal (K, K', T), SBNs sbn0 .. sbn0+nblk-1,
    whose packets are written straight into device memory.  src: the source rows (a torch HIP tensor or a raw device address),
    block b at src + b*src_stride (0 = K*T); they are read by encode() and by every emit, so they must not change until the last
    emit has completed.  Every call is enqueue-only on the context's stream."""
    _api = "nrq_tx"

    def __init__(self, ctx, K, T, nblk, src, src_stride=0, sbn0=0, Kp=0):
        self.ctx = ctx
        self._L = ctx._L
        self.K, self.T, self.nblk, self.sbn0 = K, T, nblk, sbn0
        self._keep = src  # the tensor stays alive as long as the transmission
        h = C.c_void_p()
        ctx._chk(self._L.nrq_tx_create(ctx._h, K, Kp, T, nblk, sbn0, C.c_void_p(_dptr(src)), src_stride, C.byref(h)))
        self._h = h

    @property
    def inter_ptr(self):
        """device address of the intermediate symbols (block b's L rows at + b*L*T)"""
        return self._L.nrq_tx_inter(self._h) or 0

    def emit_range(self, esi0, n, interleave=True, inline=False, out=None, tags_out=None, held=False):
        """ESIs esi0 .. esi0+n-1 of every block: n * nblk packets, interleaved (packet k: block k % nblk, ESI esi0 + k // nblk) or
        block-major (block k // n, ESI esi0 + k % n).  tags_out: optional [n * nblk] int32 device tensor for each packet's tag.
        held: refused (the range maps are analytic over all blocks; the flag is passed on so that the library says so).
        Returns out ([n * nblk, stride] uint8)."""
        out, stride = self._out(n * self.nblk, inline, out)
        self.ctx._chk(self._L.nrq_tx_emit_range(self._h, esi0, n, 1 if interleave else 0, C.c_void_p(_dptr(out)), stride,
                                                _tx_flags(inline, held), C.c_void_p(_dptr(tags_out))))
        return out

    def emit_range_syms(self, esi0, n, G, interleave=True, inline=False, out=None):
        """ESIs esi0 .. esi0+n-1 of every block in packets of G symbols (nrq_tx_emit_range_syms): per block the source run, then
        the repair run, each cut into packets of G from its start; interleaved (round j: packet j of every block) or
        block-major.  Returns (out [packets, stride] uint8, first tags [packets] int32, counts [packets] uint8)."""
        return self._range_syms(_syms_fn(self, "_emit_range_syms"), (esi0, n), pkt_count(self.K, esi0, n, G) * self.nblk, G, interleave,
                                inline, out)


class _Relay:
    """What the two relays add to their sender class: made from a receiver (which they keep alive, so that Python tears the relay
    down first), encode() = "make ready every complete block that is not", ready()."""

    def _attach(self, rx):
        self.ctx = rx.ctx
        self._L = rx._L
        self.receiver = rx
        h = C.c_void_p()
        self.ctx._chk(getattr(self._L, rx._api + "_relay")(rx._h, C.byref(h)))
        self._h = h

    def ready(self):
        """numpy bool per block: its packets can be emitted"""
        r = np.zeros(self._nblocks, np.uint32)
        self.ctx._chk(getattr(self._L, self._api + "_ready")(self._h, _u32(r)))
        return r.astype(bool)


class RelaySender(_Relay, Sender):
    """Receiver.relay(): a Sender (emit, emit_range, inter_ptr) over the reception's rows, in place."""

    def __init__(self, rx):
        self.K, self.T, self.nblk, self.sbn0 = rx.K, rx.T, rx.nblk, rx.sbn0
        self._nblocks = rx.nblk
        self._attach(rx)


EXT_RFC_OTI = 1       # NANORQ_EXT_RFC_OTI (include/nanorq_ext.h)
EXT_PER_BLOCK_KP = 2  # NANORQ_EXT_PER_BLOCK_KP
EXT_SUBBLOCKS = 4     # NANORQ_EXT_SUBBLOCKS


def obj_params_enc(F, T, K=0, Z=0, N=1, Al=8, flags=0):
    """the object parameters nanorq_encoder_new_ext(F, T, K, Z, N, Al, flags) derives (ObjParams), or None where it refuses"""
    p = ObjParams()
    return p if lib().nrq_obj_params_enc(F, T, K, Z, N, Al, flags, C.byref(p)) == 0 else None


def obj_params_oti(common, specific, flags=0):
    """the object parameters nanorq_decoder_new_ext(common, specific, flags) derives (ObjParams), or None where it refuses"""
    p = ObjParams()
    return p if lib().nrq_obj_params_oti(common, specific, flags, C.byref(p)) == 0 else None


def _blocks(p):
    return [(p.KL, p.KpL)] * p.ZL + [(p.KS, p.KpS)] * p.ZS


class ObjectSender(_Emitter):
    """A whole object sent from device memory (nrq_otx, include/nanorq_hip.h): obj is a 1-D uint8 HIP tensor of F bytes, partitioned
    as nanorq_encoder_new_ext(F, T, K, Z, N, Al, flags) does.  The object must not change until the last emit has completed.
    Every call but the constructor is enqueue-only on the context's stream."""
    _api = "nrq_otx"

    def __init__(self, ctx, obj, T, K=0, Z=0, N=1, Al=8, flags=0):
        if obj.dim() != 1 or obj.element_size() != 1 or not obj.is_contiguous():
            raise ValueError("obj must be a contiguous 1-D uint8 device tensor")
        self.ctx = ctx
        self._L = ctx._L
        self.params = obj_params_enc(obj.shape[0], T, K, Z, N, Al, flags)
        if self.params is None:
            raise NrqError("the object parameters are refused (as nanorq_encoder_new_ext would)")
        self.T = self.params.T
        self._keep = obj
        h = C.c_void_p()
        ctx._chk(self._L.nrq_otx_create(ctx._h, C.byref(self.params), C.c_void_p(_dptr(obj)), C.byref(h)))
        self._h = h

    @property
    def oti(self):
        """(common, scheme-specific) OTI words for the receiver"""
        c, s = C.c_uint64(), C.c_uint32()
        self.ctx._chk(self._L.nrq_otx_oti(self._h, C.byref(c), C.byref(s)))
        return c.value, s.value

    @property
    def blocks(self):
        """(K, K') of every block, SBN 0 .. Z-1"""
        return _blocks(self.params)

    def count_all(self, nrep):
        p = self.params
        return p.ZL * (p.KL + nrep) + p.ZS * (p.KS + nrep)

    def emit_all(self, nrep, interleave=True, inline=False, out=None, tags_out=None, held=False):
        """ESIs 0 .. K_b + nrep - 1 of every block b, block-major or interleaved (sorted by (ESI, SBN)); held: refused, as
        Sender.emit_range.  Returns out."""
        out, stride = self._out(self.count_all(nrep), inline, out)
        self.ctx._chk(self._L.nrq_otx_emit_all(self._h, nrep, 1 if interleave else 0, C.c_void_p(_dptr(out)), stride,
                                               _tx_flags(inline, held), C.c_void_p(_dptr(tags_out))))
        return out

    def count_all_syms(self, nrep, G):
        p = self.params
        return ((p.ZL * pkt_count(p.KL, 0, p.KL + nrep, G) if p.ZL else 0) +
                (p.ZS * pkt_count(p.KS, 0, p.KS + nrep, G) if p.ZS else 0))

    def emit_all_syms(self, nrep, G, interleave=True, inline=False, out=None):
        """ESIs 0 .. K_b + nrep - 1 of every block b in packets of G symbols (nrq_otx_emit_all_syms), each block class cut by
        its own K; returns (out, first tags, counts) as Sender.emit_range_syms."""
        return self._range_syms(_syms_fn(self, "_emit_all_syms"), (nrep,), self.count_all_syms(nrep, G), G, interleave, inline, out)


class RelayObjectSender(_Relay, ObjectSender):
    """ObjectReceiver.relay(): an ObjectSender (emit, emit_all, oti, blocks) over the receiver's row images, in place."""

    def __init__(self, rx):
        self.params = rx.params
        self.T = rx.params.T
        self._nblocks = rx.Z
        self._attach(rx)


class ObjectReceiver(_Handle):
    """A whole object received into device memory (nrq_orx, include/nanorq_hip.h), from its OTI words and the flags of
    nanorq_decoder_new_ext.  rep_cap: repair rows per block (default: 10 % of the larger K, at least 16)."""
    _api = "nrq_orx"

    def __init__(self, ctx, common, specific, flags=0, rep_cap=None):
        self.ctx = ctx
        self._L = ctx._L
        self.params = obj_params_oti(common, specific, flags)
        if self.params is None:
            raise NrqError("the OTI is refused (as nanorq_decoder_new_ext would)")
        p = self.params
        self.F, self.Z = p.F, p.Z
        self.rep_cap = max(16, max(p.KL, p.KS) // 10) if rep_cap is None else rep_cap
        h = C.c_void_p()
        ctx._chk(self._L.nrq_orx_create(ctx._h, C.byref(p), self.rep_cap, C.byref(h)))
        self._h = h

    @property
    def blocks(self):
        return _blocks(self.params)

    def add(self, payload, tags=None, inline=False, results=None, n=None, stride=None):
        """as Receiver.add, over every block of the object (SBN >= Z: the host decoder's codes, ERR above max_esi, else IGN)"""
        if hasattr(payload, "data_ptr"):
            n = payload.shape[0] if n is None else n
            stride = payload.stride(0) * payload.element_size() if stride is None else stride
        if n is None or stride is None:
            raise ValueError("a raw payload address needs n and stride")
        if inline == (tags is not None):
            raise ValueError("give either tags or inline=True")
        self.ctx._chk(self._L.nrq_orx_add(self._h, C.c_void_p(_dptr(payload)), stride, C.c_void_p(_dptr(tags)), n,
                                          RX_TAG_INLINE if inline else 0, C.c_void_p(_dptr(results))))

    def add_syms(self, payload, G, tags=None, nsym=None, inline=False, results=None, n=None, stride=None):
        """as Receiver.add_syms, over every block of the object (the sender's rule with each block class's own K)"""
        _add_syms(self, payload, G, tags, nsym, inline, results, n, stride)

    def counts(self):
        nl = np.zeros(self.Z, np.uint32)
        nr = np.zeros(self.Z, np.uint32)
        self.ctx._chk(self._L.nrq_orx_counts(self._h, _u32(nl), _u32(nr)))
        return nl, nr

    def decode(self):
        st = np.zeros(self.Z, np.int32)
        used = np.zeros(self.Z, np.uint32)
        self.ctx._chk(self._L.nrq_orx_decode(self._h, st.ctypes.data_as(C.POINTER(C.c_int)), _u32(used)))
        return st, used

    def held(self):
        """as Receiver.held, over both block classes in SBN order"""
        return _held(self)

    def want_syms(self, G, extra=0, source=False, esi_from=0):
        """as Receiver.want_syms, over both block classes in SBN order, each with its own K"""
        return _list_syms(self, "_want_syms", (WANT_SOURCE if source else 0, extra, esi_from, G))

    def held_syms(self, G):
        """as Receiver.held_syms, over both block classes in SBN order, each with its own K"""
        return _list_syms(self, "_held_syms", (G,))

    def want(self, extra=0, source=False, esi_from=0):
        """as Receiver.want, over both block classes in SBN order (each class with its own K)"""
        return _want(self, extra, source, esi_from)

    def relay(self):
        """An ObjectSender over this receiver's row images (nrq_orx_relay): it emits any (SBN, ESI) of every block that is ready,
        bit-exact with an ObjectSender of the original object.  One per receiver."""
        return RelayObjectSender(self)

    def write(self, out=None):
        """Every complete block into out (a uint8 device tensor of at least F bytes; None: a new one of F bytes, zeroed) in the
        object's layout; bytes past F and incomplete blocks are left untouched.  Returns (out, blocks still incomplete)."""
        if out is None:
            import torch
            out = self.ctx.new_tensor(self.F, torch.uint8, zero=True)  # (zeroed on the context's stream, ahead of the write)
        elif out.numel() * out.element_size() < self.F:
            raise ValueError("out is shorter than the object")
        rc = self._L.nrq_orx_write(self._h, C.c_void_p(_dptr(out)))
        self.ctx._chk(min(rc, 0))
        return out, rc


class ReceiverSet(_Handle):
    """A set of device-resident receptions of one T (nrq_rxset, include/nanorq_hip.h): Receivers and ObjectReceivers attached
    under 32-bit keys, fed from ONE packet buffer in one pass.  Members stay ordinary receptions; closing one detaches it, closing
    the set leaves its members usable."""
    _api = "nrq_rxset"

    def __init__(self, ctx, T):
        self.ctx = ctx
        self._L = ctx._L
        self.T = T
        self._members = {}  # key -> the attached receivers (kept alive as long as they are attached)
        if not hasattr(self._L, "nrq_rxset_create"):
            raise NrqError("this library build has no reception sets")
        h = C.c_void_p()
        ctx._chk(self._L.nrq_rxset_create(ctx._h, T, C.byref(h)))
        self._h = h

    def attach(self, key, rx):
        """rx: a Receiver, or an ObjectReceiver (both block classes; it owns its key).  May wait for the context's stream."""
        fn = self._L.nrq_rxset_attach_obj if isinstance(rx, ObjectReceiver) else self._L.nrq_rxset_attach
        self.ctx._chk(fn(self._h, key, rx._h))
        self._members.setdefault(key, []).append(rx)

    def detach(self, key):
        """every member under key (an unknown key raises).  May wait for the context's stream."""
        self.ctx._chk(self._L.nrq_rxset_detach(self._h, key))
        self._members.pop(key, None)

    def add(self, payload, keys=None, tags=None, inline=False, key_inline=False, results=None, n=None, stride=None):
        """Ingest the packets of all members (enqueue only).  payload, tags, inline, results, n, stride as in Receiver.add; keys:
        [n] int32 / uint32 device tensor of each packet's key, or key_inline=True (with inline=True) when each packet starts with
        its key in front of the FEC Payload ID, or neither: every packet has key 0.  Packets that belong to no member keep their
        results entry."""
        if hasattr(payload, "data_ptr"):
            n = payload.shape[0] if n is None else n
            stride = payload.stride(0) * payload.element_size() if stride is None else stride
        if n is None or stride is None:
            raise ValueError("a raw payload address needs n and stride")
        if inline == (tags is not None):
            raise ValueError("give either tags or inline=True")
        if key_inline and (not inline or keys is not None):
            raise ValueError("key_inline=True goes with inline=True and without keys")
        flags = (RX_TAG_INLINE if inline else 0) | (RX_KEY_INLINE if key_inline else 0)
        self.ctx._chk(self._L.nrq_rxset_add(self._h, C.c_void_p(_dptr(payload)), stride, C.c_void_p(_dptr(keys)), C.c_void_p(_dptr(tags)),
                                            n, flags, C.c_void_p(_dptr(results))))

    def add_syms(self, payload, G, keys=None, tags=None, nsym=None, inline=False, key_inline=False, results=None, n=None, stride=None):
        """Ingest packets of up to G symbols each of all members (nrq_rxset_add_syms; enqueue only): payload, keys, tags, inline,
        key_inline, n, stride as in add(), with the first tag of each packet; G, nsym and results ([n * G] int32 device tensor, one
        entry per slot) as in Receiver.add_syms.  Symbol i of a packet lies at hdr + i * T, hdr = 0, 4 (inline) or 8 (key_inline).
        Every member ends as its own add_syms over the packets of its key would leave it."""
        if hasattr(payload, "data_ptr"):
            n = payload.shape[0] if n is None else n
            stride = payload.stride(0) * payload.element_size() if stride is None else stride
        if n is None or stride is None:
            raise ValueError("a raw payload address needs n and stride")
        if inline == (tags is not None):
            raise ValueError("give either tags or inline=True")
        if key_inline and (not inline or keys is not None):
            raise ValueError("key_inline=True goes with inline=True and without keys")
        flags = (RX_TAG_INLINE if inline else 0) | (RX_KEY_INLINE if key_inline else 0)
        self.ctx._chk(self._fn("nrq_rxset_add_syms")(self._h, C.c_void_p(_dptr(payload)), stride, C.c_void_p(_dptr(keys)),
                                                     C.c_void_p(_dptr(tags)), n, G, C.c_void_p(_dptr(nsym)), flags,
                                                     C.c_void_p(_dptr(results))))

    def _fn(self, name):
        if not hasattr(self._L, name):
            raise NrqError("this library build has no %s" % name)
        return getattr(self._L, name)

    def blocks(self):
        """(keys, sbns) of the set's blocks as uint32 arrays, in the set's block order: members sorted by (key, first SBN), a
        member's blocks in SBN order.  Every per-block array of counts(), lists() and decode() is in this order (host state only)."""
        fn = self._fn("nrq_rxset_blocks")
        n = C.c_uint32(0)
        self.ctx._chk(fn(self._h, None, None, 0, C.byref(n)))
        keys, sbns = np.zeros(n.value, np.uint32), np.zeros(n.value, np.uint32)
        if n.value:
            self.ctx._chk(fn(self._h, _u32(keys), _u32(sbns), n.value, C.byref(n)))
        return keys, sbns

    def counts(self):
        """(missing source symbols, repair rows used) per block of all members, in block order (one kernel, one download; waits)."""
        n = len(self.blocks()[0])
        nl, nr = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        self.ctx._chk(self._fn("nrq_rxset_counts")(self._h, _u32(nl), _u32(nr)))
        return nl, nr

    def lists(self):
        """(nlost, nrep, lists): the counts per block and, in one uint32 array, block by block its repair ESIs in arrival order
        followed by its missing source ESIs ascending (block j's words start at sum(nlost[:j] + nrep[:j]); waits)."""
        fn = self._fn("nrq_rxset_lists")
        n = len(self.blocks()[0])
        nl, nr = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        total = C.c_size_t(0)
        self.ctx._chk(fn(self._h, _u32(nl), _u32(nr), None, 0, C.byref(total)))
        lists = np.zeros(total.value, np.uint32)
        if total.value:
            self.ctx._chk(fn(self._h, _u32(nl), _u32(nr), _u32(lists), total.value, C.byref(total)))
        return nl, nr, lists

    def decode(self):
        """Decode every member in place with one listing pass, the decodable blocks of all members grouped by code parameters
        into as few decode calls as possible, and one marking launch; returns (status, used) per block in block order, with
        Receiver.decode's meaning.  Every member is left as its own decode() would have left it."""
        fn = self._fn("nrq_rxset_decode")
        n = len(self.blocks()[0])
        st, used = np.zeros(n, np.int32), np.zeros(n, np.uint32)
        self.ctx._chk(fn(self._h, st.ctypes.data_as(C.POINTER(C.c_int)), _u32(used)))
        return st, used

    def _listing(self, fn, args, per_block):
        """a set-wide listing with keys, as _want / _held: the count call, two tensors of that size, the fill call"""
        import torch
        n = C.c_uint32(0)
        cnt = np.zeros(len(self.blocks()[0]), np.uint32)
        self.ctx._chk(fn(self._h, *args, None, None, 0, _u32(cnt) if per_block else None, C.byref(n)))
        keys = self.ctx.new_tensor(n.value, torch.int32)
        tags = self.ctx.new_tensor(n.value, torch.int32)
        if n.value:
            self.ctx._chk(fn(self._h, *args, C.c_void_p(_dptr(keys)), C.c_void_p(_dptr(tags)), n.value, None, C.byref(n)))
            self.ctx.sync()  # (torch's stream and the library's are not ordered: the lists are complete on return)
        return (keys, tags, cnt) if per_block else (keys, tags)

    def want(self, extra=0, source=False, esi_from=0, per_block=False):
        """(keys, tags): what every member's own want(extra, source, esi_from) lists, one behind the other in block order, and
        beside each tag the key of its member -- [n] int32 device tensors listed on the device in one pass (three launches, one
        wait for the whole set), the form SenderSet.emit(keys, tags, ...) takes.  Each member is asked with its own K, max_esi
        and repair rows.  per_block=True: also the number of tags per block, a uint32 array in blocks() order."""
        return self._listing(self._fn("nrq_rxset_want"), (WANT_SOURCE if source else 0, extra, esi_from), per_block)

    def held(self, per_block=False):
        """(keys, tags): what every member's own held() lists, one behind the other in block order, with each tag's key, as
        want() -- the list SenderSet.emit(keys, tags, held=True) over the members' relays writes in full."""
        return self._listing(self._fn("nrq_rxset_held"), (), per_block)

    def _listing_syms(self, fn, args, per_block):
        """a set-wide listing in packets with keys, as _listing: the count call, three tensors of that size, the fill call"""
        import torch
        npkt = C.c_uint32(0)
        cnt = np.zeros(len(self.blocks()[0]), np.uint32)
        self.ctx._chk(fn(self._h, *args, None, None, None, 0, _u32(cnt) if per_block else None, C.byref(npkt), None))
        keys = self.ctx.new_tensor(npkt.value, torch.int32)
        tags = self.ctx.new_tensor(npkt.value, torch.int32)
        nsym = self.ctx.new_tensor(npkt.value, torch.uint8)
        if npkt.value:
            self.ctx._chk(fn(self._h, *args, C.c_void_p(_dptr(keys)), C.c_void_p(_dptr(tags)), C.c_void_p(_dptr(nsym)), npkt.value, None,
                             C.byref(npkt), None))
            self.ctx.sync()  # (torch's stream and the library's are not ordered: the lists are complete on return)
        return (keys, tags, nsym, cnt) if per_block else (keys, tags, nsym)

    def want_syms(self, G, extra=0, source=False, esi_from=0, per_block=False):
        """(keys, tags, nsym): want() as packets of up to G symbols (nrq_rxset_want_syms) -- what every member's own
        want_syms(G, extra, source, esi_from) lists, one behind the other in block order, with each packet's key: int32 / int32 /
        uint8 [n] device tensors, the form SenderSet.emit_syms(keys, tags, G, nsym=nsym, ...) takes.  Each member's list is cut with
        its own K.  per_block=True: also the number of PACKETS per block, a uint32 array in blocks() order."""
        return self._listing_syms(self._fn("nrq_rxset_want_syms"), (WANT_SOURCE if source else 0, extra, esi_from, G), per_block)

    def held_syms(self, G, per_block=False):
        """(keys, tags, nsym): held() as packets of up to G symbols (nrq_rxset_held_syms), as want_syms -- the list
        SenderSet.emit_syms(keys, tags, G, nsym=nsym, held=True) over the members' relays writes in full."""
        return self._listing_syms(self._fn("nrq_rxset_held_syms"), (G,), per_block)


class SenderSet(_Handle):
    """A set of device-resident transmissions of one T (nrq_txset, include/nanorq_hip.h): Senders, RelaySenders, ObjectSenders and
    RelayObjectSenders attached under 32-bit keys, whose packets ONE emit writes into one buffer.  Members stay ordinary
    transmissions; closing one detaches it, closing the set leaves its members usable."""
    _api = "nrq_txset"

    def __init__(self, ctx, T):
        self.ctx = ctx
        self._L = ctx._L
        self.T = T
        self._members = {}  # key -> the attached senders (kept alive as long as they are attached)
        if not hasattr(self._L, "nrq_txset_create"):
            raise NrqError("this library build has no sender sets")
        h = C.c_void_p()
        ctx._chk(self._L.nrq_txset_create(ctx._h, T, C.byref(h)))
        self._h = h

    def attach(self, key, tx):
        """tx: a Sender or RelaySender, or an ObjectSender or RelayObjectSender (it owns its key).  May wait for the context's
        stream."""
        fn = self._L.nrq_txset_attach_obj if isinstance(tx, ObjectSender) else self._L.nrq_txset_attach
        self.ctx._chk(fn(self._h, key, tx._h))
        self._members.setdefault(key, []).append(tx)

    def detach(self, key):
        """every member under key (an unknown key raises).  May wait for the context's stream."""
        self.ctx._chk(self._L.nrq_txset_detach(self._h, key))
        self._members.pop(key, None)

    def blocks(self):
        """(keys, sbns) of the set's blocks as uint32 arrays, in the set's block order, as ReceiverSet.blocks()"""
        n = C.c_uint32(0)
        self.ctx._chk(self._L.nrq_txset_blocks(self._h, None, None, 0, C.byref(n)))
        keys, sbns = np.zeros(n.value, np.uint32), np.zeros(n.value, np.uint32)
        if n.value:
            self.ctx._chk(self._L.nrq_txset_blocks(self._h, _u32(keys), _u32(sbns), n.value, C.byref(n)))
        return keys, sbns

    def stride(self, inline=False, key_inline=False):
        """the packet stride of out=None: T, or T + 4 (inline) or T + 8 (key_inline) rounded up to 16"""
        hdr = 8 if key_inline else 4 if inline else 0
        return (self.T + hdr + 15) // 16 * 16 if hdr else self.T

    def emit(self, keys, tags, out=None, inline=False, key_inline=False, results=None, held=False):
        """Packet k for (keys[k], tags[k]) ([n] int32 / uint32 device tensors; keys None: every key 0) in row k of out
        ([n, stride] uint8 device tensor; None: a new one).  inline: the FEC Payload ID in front of the payload; key_inline (with
        inline): the key in front of that, the form ReceiverSet.add(key_inline=True) reads.  results: optional [n] int32 device
        tensor, with _Emitter.emit's codes; a packet of no member is left untouched with -1.  held: as _Emitter.emit, on the relay
        members (plain senders answer as without it).  Enqueue only.  Returns out."""
        n = int(tags.shape[0])
        if out is None:
            import torch
            out = self.ctx.new_tensor((n, self.stride(inline, key_inline)), torch.uint8)
            stride = out.shape[1]
        else:
            stride = out.stride(0) * out.element_size()
        flags = _tx_flags(inline, held) | (TX_KEY_INLINE if key_inline else 0)
        self.ctx._chk(self._L.nrq_txset_emit(self._h, C.c_void_p(_dptr(keys)), C.c_void_p(_dptr(tags)), n, C.c_void_p(_dptr(out)), stride,
                                             flags, C.c_void_p(_dptr(results))))
        return out

    def stride_syms(self, G, inline=False, key_inline=False):
        """the packet stride of out=None for packets of G symbols: G * T, or G * T + 4 (inline) or + 8 (key_inline) rounded up to 16"""
        hdr = 8 if key_inline else 4 if inline else 0
        return (G * self.T + hdr + 15) // 16 * 16 if hdr else G * self.T

    def emit_syms(self, keys, tags, G, nsym=None, out=None, inline=False, key_inline=False, results=None, held=False):
        """Packet k of up to G symbols for (keys[k], first tag tags[k]) in row k of out (nrq_txset_emit_syms): keys, tags, out,
        inline, key_inline as in emit(); G, nsym and results (0, -1, TX_NOT_READY, TX_BAD_RANGE; only a 0 packet is written, and
        whole) as in _Emitter.emit_syms, each member with its own K.  held: as _Emitter.emit_syms on the relay members -- a packet
        of a block that is not ready is written iff the member's reception holds EVERY one of its symbols; plain senders answer as
        without it, and a set with no relay member refuses it.  Enqueue only.  Returns out."""
        if not hasattr(self._L, "nrq_txset_emit_syms"):
            raise NrqError("this library build has no nrq_txset_emit_syms")
        n = int(tags.shape[0])
        if out is None:
            import torch
            out = self.ctx.new_tensor((n, self.stride_syms(G, inline, key_inline)), torch.uint8)
            stride = out.shape[1]
        else:
            stride = out.stride(0) * out.element_size()
        flags = _tx_flags(inline, held) | (TX_KEY_INLINE if key_inline else 0)
        self.ctx._chk(self._L.nrq_txset_emit_syms(self._h, C.c_void_p(_dptr(keys)), C.c_void_p(_dptr(tags)), n, G, C.c_void_p(_dptr(nsym)),
                                                  C.c_void_p(_dptr(out)), stride, flags, C.c_void_p(_dptr(results))))
        return out

    def _range_fn(self, name):
        fn = getattr(self._L, name, None)
        if fn is None:
            raise NrqError("this library build has no range mode of a sender set (%s)" % name)
        return fn

    def count_all(self, nrep, G=1, source=True, per_block=False):
        """packets of emit_all(nrep, source=source) / emit_all_syms(nrep, G, source=source) (nrq_txset_count_all); per_block: (total,
        uint32 array of the packets of every block in the set's block order).  Host state only."""
        n = C.c_uint32(0)
        cnt = np.zeros(len(self.blocks()[0]), np.uint32) if per_block else None
        self.ctx._chk(self._range_fn("nrq_txset_count_all")(self._h, 1 if source else 0, nrep, G, None if cnt is None else _u32(cnt), C.byref(n)))
        return (n.value, cnt) if per_block else n.value

    def _range(self, syms, nrep, G, interleave, inline, key_inline, out, rep0, source, keys_out, tags_out, nsym_out, held):
        npkt = self.count_all(nrep, G, source)
        if out is None:
            import torch
            out = self.ctx.new_tensor((npkt, self.stride_syms(G, inline, key_inline)), torch.uint8)
            stride = out.shape[1]
        else:
            stride = out.stride(0) * out.element_size()
        flags = _tx_flags(inline, held) | (TX_KEY_INLINE if key_inline else 0)
        head = (self._h, 1 if source else 0, rep0, nrep) + ((G,) if syms else ())
        tail = (C.c_void_p(_dptr(keys_out)), C.c_void_p(_dptr(tags_out))) + ((C.c_void_p(_dptr(nsym_out)),) if syms else ())
        got = C.c_uint32()
        fn = self._range_fn("nrq_txset_emit_all_syms" if syms else "nrq_txset_emit_all")
        self.ctx._chk(fn(*head, 1 if interleave else 0, C.c_void_p(_dptr(out)), stride, flags, *tail, C.byref(got)))
        assert got.value == npkt, (got.value, npkt)
        return out

    def emit_all(self, nrep, interleave=True, inline=False, key_inline=False, out=None, rep0=0, source=True, keys_out=None, tags_out=None,
                 held=False):
        """The range mode (nrq_txset_emit_all): of every block of every member the K source symbols (source) and the repair ESIs
        K + rep0 .. K + rep0 + nrep - 1, each block with its own K -- count_all(nrep, source=source) packets, block-major in the
        set's block order or interleaved (round j: packet j of every block that has one, in block order), with no list from the
        host.  inline / key_inline as in emit(); keys_out / tags_out: optional [packets] int32 device tensors for each packet's
        key and tag; held: refused, as Sender.emit_range.  out None: a new [packets, stride] tensor.  Enqueue only.  Returns out."""
        return self._range(False, nrep, 1, interleave, inline, key_inline, out, rep0, source, keys_out, tags_out, None, held)

    def emit_all_syms(self, nrep, G, interleave=True, inline=False, key_inline=False, out=None, rep0=0, source=True, keys_out=None,
                      tags_out=None, nsym_out=None, held=False):
        """emit_all in packets of G symbols (nrq_txset_emit_all_syms): per block the source run, then the repair run, each cut into
        packets of G from its start, the last one short -- count_all(nrep, G, source) packets; nsym_out: optional [packets] uint8
        device tensor for each packet's count.  Returns out."""
        return self._range(True, nrep, G, interleave, inline, key_inline, out, rep0, source, keys_out, tags_out, nsym_out, held)


def plan_ops(plan, header=None):
    """The op stream of a plan as an array [row, lane] (a copy).  plan.h: the stream is stored quad-interleaved -- the words
    of rows 4g..4g+3 of a lane lie next to each other (NRQ_OP_INDEX)."""
    import numpy as np
    h = header or plan_header(bytes(plan))
    rows = (h["nrows"] + 3) & ~3
    a = np.frombuffer(bytes(plan), dtype=np.uint32, offset=h["off_ops"], count=rows * 64)
    return a.reshape(rows // 4, 64, 4).transpose(0, 2, 1).reshape(rows, 64)[:h["nrows"]].copy()


def plan_ops_store(plan, ops, header=None):
    """Write an array [row, lane] (all nrows rows) back into the bytearray `plan` (tests that tamper with a stream)."""
    import numpy as np
    h = header or plan_header(bytes(plan))
    rows = (h["nrows"] + 3) & ~3
    assert ops.shape == (h["nrows"], 64)
    full = np.frombuffer(plan, dtype=np.uint32, offset=h["off_ops"], count=rows * 64).reshape(rows // 4, 64, 4)
    for r in range(h["nrows"]):
        full[r // 4, :, r % 4] = ops[r]
