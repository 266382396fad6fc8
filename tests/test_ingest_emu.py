"""CPU tier of the device-resident receiver (nrq_rx_*): the emulated ingest kernels (tests/emu/ingest_emu.cpp running the bodies of
nanorq_amd/csrc/ingest_body.h) on randomised packet streams, against nanorq_decoder_add_symbol on a decoder object fed the same
tags in the same order, and against a plain Python model of the same rules (rows, repair lists, missing lists, counts)."""
import ctypes as C

import numpy as np
import pytest

import nanorq_amd
from capi import api
from rx_support import (ADDED, DUP, ERR, FULL, IGN, UNTOUCHED, EmuRx, ModelRx, inline_packets, payloads_for, random_stream, tag)


def _pkts(tags, T, inline, stride_pad=0, salt=0):
    pl = payloads_for(tags, T, salt)
    if inline:
        return inline_packets(pl, tags, T + 4 + stride_pad), pl
    return np.concatenate([pl, np.zeros((len(tags), stride_pad), np.uint8)], axis=1), pl


def _check_same(emu, model):
    assert list(emu.gaps) == [len(m) for m in model.missing]
    assert list(emu.nrep) == [len(r) for r in model.reps]
    for b in range(emu.nblk):
        assert np.array_equal(emu.lost(b), model.lost(b)), b
        assert np.array_equal(emu.rep_list(b), np.array(model.reps[b], np.uint32)), b
    assert np.array_equal(emu.src, model.src)
    assert np.array_equal(emu.rep, model.rep)
    assert (emu.first == 0xFFFFFFFF).all(), "the first-arrival table is reset after every call"


@pytest.mark.parametrize("K,T,nblk,sbn0,rep_cap,n,calls,inline,seed", [
    (10, 8, 1, 0, 64, 40, 1, False, 1),
    (10, 8, 3, 2, 4, 300, 3, True, 2),           # rep_cap overflow, other blocks' SBNs, inline headers
    (100, 16, 4, 1, 12, 700, 2, False, 3),
    (100, 12, 5, 0, 200, 1500, 4, True, 4),      # 4-byte payload alignment under an inline header
    (300, 5, 2, 7, 40, 1200, 3, False, 5),       # T not a multiple of 4
    (1000, 16, 3, 0, 150, 5000, 2, False, 6),    # many tiles per call
    (1000, 16, 2, 250, 3000, 4000, 1, True, 7),  # SBNs up to 255
])
def test_emulated_ingest_matches_model(K, T, nblk, sbn0, rep_cap, n, calls, inline, seed):
    Kp = nanorq_amd.params(K)["Kp"]
    rng = np.random.default_rng(seed)
    emu, model = EmuRx(K, T, nblk, rep_cap, sbn0, Kp=Kp), ModelRx(K, T, nblk, rep_cap, sbn0, Kp=Kp)
    seen_codes = set()
    for call in range(calls):
        tags = random_stream(rng, K, nblk, sbn0, 2 * Kp, n, sbn_span=2)
        pk, pl = _pkts(tags, T, inline, stride_pad=int(rng.integers(0, 5)), salt=call)
        r_emu = emu.add(pk, None if inline else tags)
        r_mod = model.add(pl, tags)
        assert np.array_equal(r_emu, r_mod), np.flatnonzero(r_emu != r_mod)[:10]
        seen_codes |= set(int(x) for x in r_emu)
        _check_same(emu, model)
        if call == 0:  # a block recovered by a decode: later packets for it are IGN
            emu.mark_complete(0)
            model.mark_complete(0)
    assert {ADDED, DUP}.issubset(seen_codes)
    if rep_cap <= 40:
        assert FULL in seen_codes


def _decoder(K, T, nblk):
    L = api()
    enc = L.nanorq_encoder_new_ex(nblk * K * T, T, K, nblk, 8)
    assert enc and L.nanorq_blocks(enc) == nblk
    assert all(L.nanorq_block_symbols(enc, b) == K for b in range(nblk))
    dq = L.nanorq_decoder_new(L.nanorq_oti_common(enc), L.nanorq_oti_scheme_specific(enc))
    L.nanorq_free(enc)
    return L, dq


@pytest.mark.parametrize("K,T,nblk,sbn0,n,calls,inline,seed", [
    (20, 8, 4, 1, 300, 3, False, 11),
    (100, 16, 5, 0, 1200, 2, True, 12),
    (1000, 8, 3, 2, 3000, 2, False, 13),
])
def test_emulated_codes_match_decoder_add_symbol(K, T, nblk, sbn0, n, calls, inline, seed):
    """the per-packet result codes are those of nanorq_decoder_add_symbol on an object of the same blocks (rep_cap large enough
    that NRQ_RX_FULL cannot happen: the object layer has no such limit); packets of the object's other blocks are untouched"""
    Z = sbn0 + nblk + 2
    L, dq = _decoder(K, T, Z)
    Kp = nanorq_amd.params(K)["Kp"]
    emu = EmuRx(K, T, nblk, 2 * Kp - K + 1, sbn0, Kp=Kp)
    rng = np.random.default_rng(seed)
    sym = (C.c_uint8 * T)()
    for call in range(calls):
        tags = random_stream(rng, K, nblk, sbn0, 2 * Kp, n, sbn_span=2)
        tags = tags[(tags >> 24) < Z]
        pk, _ = _pkts(tags, T, inline)
        res = emu.add(pk, None if inline else tags)
        ref = np.array([L.nanorq_decoder_add_symbol(dq, sym, int(t), None) for t in tags], np.int32)
        inside = ((tags >> 24) >= sbn0) & ((tags >> 24) < sbn0 + nblk)
        assert np.array_equal(res[inside], ref[inside]), np.flatnonzero(res[inside] != ref[inside])[:10]
        assert (res[~inside] == UNTOUCHED).all()
        for b in range(nblk):
            assert emu.gaps[b] == L.nanorq_num_missing(dq, sbn0 + b)
            assert emu.nrep[b] == L.nanorq_num_repair(dq, sbn0 + b)
    L.nanorq_free(dq)


def test_emulated_completion_and_order():
    """hand-made stream: the packet that completes a block is added, later ones (also repair and duplicates) are IGN; repair rows
    go in arrival order; a duplicate of a repair ESI that found the rows full is full as well"""
    K, T = 10, 4
    Kp = nanorq_amd.params(K)["Kp"]
    emu = EmuRx(K, T, 1, 2, 0, Kp=Kp)
    tags = [tag(0, e) for e in (3, 15, 12, 3, 14, 14, 2 * Kp + 1, 15)] + [tag(0, e) for e in range(K) if e != 3] + [tag(0, 16), tag(0, 5)]
    tags = np.array(tags, np.uint32)
    pl = payloads_for(tags, T)
    res = emu.add(pl, tags)
    assert list(res[:8]) == [ADDED, ADDED, ADDED, DUP, FULL, FULL, ERR, DUP]
    assert list(res[8:-2]) == [ADDED] * (K - 1)
    assert list(res[-2:]) == [IGN, IGN]
    assert list(emu.rep_list(0)) == [15, 12] and emu.gaps[0] == 0
    assert np.array_equal(emu.rep[0, 0], pl[1]) and np.array_equal(emu.rep[0, 1], pl[2])
    res2 = emu.add(pl[:3], tags[:3])
    assert list(res2) == [IGN] * 3
