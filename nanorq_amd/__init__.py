"""nanorq_amd -- MI355X-native RaptorQ precode solve / symbol generation (nanorq-compatible).

The product is the native library nanorq_amd/libnanorq_hip.so (gfx950 HIP kernels behind the C ABI
of include/nanorq_hip.h, plus the drop-in nanorq.h / io.h layer).  This package only loads it and
offers a thin ctypes mirror for tests and bench.py; there is no Python or CPU implementation of
the hot path, and every entry point raises when the HIP library or a GPU is missing.
"""
from .binding import (NrqError, Context, Receiver, ReceiverSet, SenderSet, RX_TAG_INLINE, RX_KEY_INLINE, RX_FULL, RXSET_MAX_MEMBERS, RXSET_MAX_BLOCKS, Sender, TX_TAG_INLINE, TX_HELD, TX_NOT_READY, TX_BAD_RANGE, PKT_SYMS_MAX, pkt_count, TX_KEY_INLINE, TXSET_MAX_SEGS, TXSET_MAX_BLOCKS, WANT_SOURCE, ObjParams, ObjectSender, ObjectReceiver,
                      obj_params_enc, obj_params_oti, EXT_RFC_OTI, EXT_PER_BLOCK_KP, EXT_SUBBLOCKS, lib, lib_path, params, host_plan, host_kconst, PLAN_FIELDS,
                      plan_header, plan_ops, plan_ops_store)

__all__ = ["NrqError", "Context", "Receiver", "ReceiverSet", "SenderSet", "RX_TAG_INLINE", "RX_KEY_INLINE", "RX_FULL", "RXSET_MAX_MEMBERS", "RXSET_MAX_BLOCKS", "Sender", "TX_TAG_INLINE", "TX_HELD", "TX_NOT_READY", "TX_BAD_RANGE", "PKT_SYMS_MAX", "pkt_count", "TX_KEY_INLINE", "TXSET_MAX_SEGS", "TXSET_MAX_BLOCKS", "WANT_SOURCE", "ObjParams", "ObjectSender", "ObjectReceiver",
           "obj_params_enc", "obj_params_oti", "EXT_RFC_OTI", "EXT_PER_BLOCK_KP", "EXT_SUBBLOCKS", "lib", "lib_path", "params", "host_plan", "host_kconst", "PLAN_FIELDS",
           "plan_header", "plan_ops", "plan_ops_store"]
