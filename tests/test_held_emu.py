"""CPU tier of the held symbols: the emulated ingest (ingest_body.h) fills receptions, then the emulated held emit (tx_admit_held
and the repair row lookup of emit_body.h, through held_emu.cpp) answers tag lists over them.  Expected results follow the table
of include/nanorq_hip.h, from a plain Python model of the reception (rx_support.ModelRx):
  SBN outside the span: untouched, -1;  block ready: the plain emit's packet, 0;  block not ready and the symbol held: the
  ingested bytes, 0;  block not ready and the symbol not held: untouched, -2.
Symbols of every kind are asked for: delivered, dropped, never sent, duplicated, FULL (a small rep_cap), above max_esi (whose
seen bit would lie behind the bitmap: the emulation is handed a bitmap with all-ones words behind it, so a read past it would show
as "held") and foreign.  The listing (held_body.h) is checked for content, order and bounds, and fed back into the held emit."""
import numpy as np
import pytest

import nanorq_amd
from held_support import emu_emit_held, emu_rx_held, host_held
from relay_support import FOREIGN, NOT_READY, emu_emit_table_ready
from rx_support import ADDED, FULL, EmuRx, ModelRx, payloads_for, tag
from tx_support import FILL

# (T, inline, stride): the shapes that select the kernel's four payload paths -- 16-byte, 16-byte under an inline header, 4-byte,
# bytes (an odd stride)
PATHS = [(1280, False, 1280), (1280, True, 1296), (20, False, 20), (7, True, 13)]


def _fill(rng, K, T, nblk, sbn0, rep_cap, nsent_rep, loss, batches=2, salt=0):
    """an emulated reception and its model, fed the same lossy, shuffled, partly duplicated stream in `batches` calls -> (emu,
    model, {tag: payload} of everything that was sent, result codes per sent packet)"""
    Kp = nanorq_amd.params(K)["Kp"]
    emu = EmuRx(K, T, nblk, rep_cap, sbn0=sbn0, Kp=Kp)
    mod = ModelRx(K, T, nblk, rep_cap, sbn0=sbn0, Kp=Kp)
    sent = np.array([tag(sbn0 + b, e) for b in range(nblk) for e in range(K + nsent_rep)], np.uint32)
    deliv = sent[rng.random(len(sent)) >= loss]
    deliv = np.concatenate([deliv, deliv[rng.integers(0, len(deliv), max(1, len(deliv) // 10))],        # duplicates
                            [tag(sbn0, emu.max_esi + 1), tag(sbn0 + nblk - 1, emu.max_esi + 7)]]).astype(np.uint32)  # ERR
    rng.shuffle(deliv)
    codes = []
    for part in np.array_split(deliv, batches):
        pay = payloads_for(part, T, salt)
        a, m = emu.add(pay, tags=part), mod.add(pay, part)
        assert np.array_equal(a, m)
        codes.append(a)
    return emu, mod, Kp, sent, deliv, np.concatenate(codes)


def _asked(rng, rxs, span, sent_lists):
    """the tags to ask for: everything sent, ESIs never sent, ESIs above max_esi (up to 2^24 - 1), foreign SBNs; shuffled"""
    sbn0, Z, _ = span
    extra = []
    for r in rxs:
        for b in range(r.nblk):
            sbn = r.sbn0 + b
            extra += [tag(sbn, r.max_esi), tag(sbn, r.max_esi + 1), tag(sbn, r.max_esi + 33), tag(sbn, r.bm_words * 32),
                      tag(sbn, r.bm_words * 32 + 31), tag(sbn, (1 << 24) - 1), tag(sbn, r.K + 60)]
    for sbn in (sbn0 - 1, sbn0 + Z, sbn0 + Z + 1):
        if 0 <= sbn < 256:
            extra += [tag(sbn, 0), tag(sbn, 5)]
    tags = np.concatenate(list(sent_lists) + [np.array(extra, np.uint32)]).astype(np.uint32)
    rng.shuffle(tags)
    return tags


def _check(pk, res, tags, rxs, mods, span, ready, ref_pk, T, inline, salt=0):
    """every packet against the rule table; mods: the models (what is held); ref_pk: the plain emit with every block ready"""
    sbn0, Z, _ = span
    off = 4 if inline else 0
    seen_kinds = set()
    for k, t in enumerate(tags):
        sbn, esi = int(t) >> 24, int(t) & 0xFFFFFF
        if not sbn0 <= sbn < sbn0 + Z:
            assert res[k] == FOREIGN and (pk[k] == FILL).all(), k
            seen_kinds.add("foreign")
            continue
        g = next(i for i, r in enumerate(rxs) if r.sbn0 <= sbn < r.sbn0 + r.nblk)
        b = sbn - rxs[g].sbn0
        if ready[sbn - sbn0]:
            assert res[k] == 0 and np.array_equal(pk[k], ref_pk[k]), k
            seen_kinds.add("ready")
        elif esi in mods[g].seen[b]:
            assert res[k] == 0, (k, sbn, esi)
            want = mods[g].src[b, esi] if esi < rxs[g].K else mods[g].rep[b, mods[g].reps[b].index(esi)]
            assert np.array_equal(pk[k, off:off + T], want), (k, sbn, esi)
            if inline:
                assert bytes(pk[k, :4]) == int(t).to_bytes(4, "big"), k
            assert (pk[k, off + T:] == FILL).all(), k
            seen_kinds.add("src" if esi < rxs[g].K else "rep")
        else:
            assert res[k] == NOT_READY and (pk[k] == FILL).all(), (k, sbn, esi)
            seen_kinds.add("absent")
    return seen_kinds


@pytest.mark.parametrize("T,inline,stride", PATHS)
@pytest.mark.parametrize("K", [10, 100, 257])
def test_held_emit_one_reception(K, T, inline, stride):
    rng = np.random.default_rng(K * 7 + T)
    nblk, sbn0 = 4, 3
    rep_cap = max(2, K // 8)  # (small enough for FULL: about K/4 repair symbols are sent, most arrive)
    emu, mod, Kp, sent, deliv, codes = _fill(rng, K, T, nblk, sbn0, rep_cap, K // 4 + 4, 0.2)
    assert (codes == FULL).any() and (codes == ADDED).any()
    # a held payload is the ingested one (the model's rows are the packets' bytes)
    assert np.array_equal(emu.src, mod.src) and np.array_equal(emu.rep, mod.rep)
    # block 0 ready; block 1 short; block 2 complete but not ready (decoded before the relay was attached); block 3 short
    lost2 = emu.lost(2)
    fixed = rng.integers(0, 256, (len(lost2), T), dtype=np.uint8)
    emu.src[2, lost2] = fixed
    mod.src[2, lost2] = fixed
    emu.mark_complete(2)
    mod.mark_complete(2)
    ready = np.array([True, False, False, False])
    L = nanorq_amd.params(Kp)["L"]
    inter = rng.integers(0, 256, (nblk, L, T), dtype=np.uint8)
    span = (sbn0, nblk, nblk)
    tags = _asked(rng, [emu], span, [sent])
    seg = [(K, Kp, sbn0, emu.src.reshape(nblk, -1), inter)]
    ref_pk, _ = emu_emit_table_ready(seg, span, T, inline, stride, np.ones(nblk, bool), tags=tags)
    pk, res = emu_emit_held([emu], [Kp], [inter], span, ready, tags, inline, stride)
    kinds = _check(pk, res, tags, [emu], [mod], span, ready, ref_pk, T, inline)
    assert kinds == {"foreign", "ready", "src", "rep", "absent"}
    # FULL symbols and ESIs above max_esi are not held; a duplicated symbol is held once
    blk = (deliv >> 24).astype(int) - sbn0
    full = np.isin(tags, deliv[(codes == FULL) & (blk != 0)])
    assert full.any() and (res[full] == NOT_READY).all()
    # the complete, not ready block: every source ESI, its received repair ESIs, no fresh ones
    is2 = (tags >> 24) == sbn0 + 2
    e2 = tags & 0xFFFFFF
    assert (res[is2 & (e2 < K)] == 0).all()
    assert (res[is2 & (e2 >= K) & ~np.isin(e2, mod.reps[2])] == NOT_READY).all()
    # without the flag (the plain emit with the same mask): nothing of a block that is not ready
    pk0, res0 = emu_emit_table_ready(seg, span, T, inline, stride, ready, tags=tags)
    nr = ((tags >> 24) > sbn0) & ((tags >> 24) < sbn0 + nblk)
    assert (res0[nr] == NOT_READY).all() and (pk0[nr] == FILL).all()
    # with every block ready the held emit is the plain emit
    pk1, res1 = emu_emit_held([emu], [Kp], [inter], span, np.ones(nblk, bool), tags, inline, stride)
    assert np.array_equal(pk1, ref_pk) and np.array_equal(res1 == 0, ((tags >> 24) >= sbn0) & ((tags >> 24) < sbn0 + nblk))


@pytest.mark.parametrize("T,inline,stride", [(20, False, 23), (16, True, 32)])
def test_held_emit_two_classes(T, inline, stride):
    """an object's relay: two receptions of different K (and K') side by side, one of them ahead of the other"""
    rng = np.random.default_rng(T)
    eL, mL, KpL, sentL, _, _ = _fill(rng, 31, T, 2, 0, 6, 10, 0.15, salt=1)
    eS, mS, KpS, sentS, _, _ = _fill(rng, 30, T, 3, 2, 40, 10, 0.3, batches=3, salt=1)
    span = (0, 5, 2)
    ready = np.array([False, True, False, False, False])
    inters = [rng.integers(0, 256, (r.nblk, nanorq_amd.params(Kp)["L"], T), dtype=np.uint8) for r, Kp in ((eL, KpL), (eS, KpS))]
    tags = _asked(rng, [eL, eS], span, [sentL, sentS])
    segs = [(r.K, Kp, r.sbn0, r.src.reshape(r.nblk, -1), it) for r, Kp, it in ((eL, KpL, inters[0]), (eS, KpS, inters[1]))]
    ref_pk, _ = emu_emit_table_ready(segs, span, T, inline, stride, np.ones(5, bool), tags=tags)
    pk, res = emu_emit_held([eL, eS], [KpL, KpS], inters, span, ready, tags, inline, stride)
    kinds = _check(pk, res, tags, [eL, eS], [mL, mS], span, ready, ref_pk, T, inline)
    assert kinds == {"foreign", "ready", "src", "rep", "absent"}


def test_nothing_is_held_after_a_reset():
    rng = np.random.default_rng(5)
    K, T, nblk = 40, 16, 3
    emu, mod, Kp, sent, _, _ = _fill(rng, K, T, nblk, 0, 8, 6, 0.1)
    assert emu_rx_held(emu)[1] > 0
    fresh = EmuRx(K, T, nblk, 8, Kp=Kp)  # what nrq_rx_reset leaves: the books cleared, the rows as they were
    fresh.src[:], fresh.rep[:] = emu.src, emu.rep
    inter = np.zeros((nblk, nanorq_amd.params(Kp)["L"], T), np.uint8)
    pk, res = emu_emit_held([fresh], [Kp], [inter], (0, nblk, nblk), np.zeros(nblk, bool), sent, False, T)
    assert (res == NOT_READY).all() and (pk == FILL).all()
    assert emu_rx_held(fresh)[1] == 0


@pytest.mark.parametrize("K", [10, 32, 100, 257])
def test_listing(K):
    rng = np.random.default_rng(K)
    T, nblk, sbn0 = 8, 5, 250
    emu, mod, Kp, sent, _, _ = _fill(rng, K, T, nblk, sbn0, K // 6 + 1, K // 3 + 2, 0.25, batches=3)
    emu.mark_complete(1)
    mod.mark_complete(1)
    rc, n, lst = emu_rx_held(emu)
    want = host_held(sbn0, K, [emu.seen_bits(b) for b in range(nblk)], [emu.rep_list(b) for b in range(nblk)])
    assert rc == 0 and n == len(want) == sum(K - len(mod.lost(b)) + len(mod.reps[b]) for b in range(nblk))
    assert np.array_equal(lst, want)
    # the model agrees on content and order
    assert np.array_equal(lst, host_held(sbn0, K, [[e in mod.seen[b] for e in range(K)] for b in range(nblk)], mod.reps))
    # too small a buffer: refused, the count still given, nothing written
    rc, n2, small = emu_rx_held(emu, cap=n - 1)
    assert rc == -1 and n2 == n and (small == 0xDEADBEEF).all()
    # a larger one: the list, nothing behind it
    rc, n3, big = emu_rx_held(emu, cap=n + 3)
    assert rc == 0 and n3 == n and np.array_equal(big[:n], want) and (big[n:] == 0xDEADBEEF).all()
    # the list, emitted with held symbols from blocks that are not ready: every packet written, with the ingested bytes
    inter = np.zeros((nblk, nanorq_amd.params(Kp)["L"], T), np.uint8)
    pk, res = emu_emit_held([emu], [Kp], [inter], (sbn0, nblk, nblk), np.zeros(nblk, bool), lst, True, T + 4)
    assert (res == 0).all()
    for k, t in enumerate(lst):
        b, esi = (int(t) >> 24) - sbn0, int(t) & 0xFFFFFF
        want_row = emu.src[b, esi] if esi < K else emu.rep[b, list(emu.rep_list(b)).index(esi)]
        assert np.array_equal(pk[k, 4:], want_row) and bytes(pk[k, :4]) == int(t).to_bytes(4, "big")
