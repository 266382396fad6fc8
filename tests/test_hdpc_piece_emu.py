"""CPU tier: the piece form of the HDPC phase (solve_body.h hdpc_chunks<.., PB>) on every branch of its chunking rule.

In the piece form GP = WB / PB adjacent lanes share one chunk of columns and carry PB bytes of the strip each, so a phase of `hnt`
threads has C = hnt / GP chunks and the rule that deals the n = K' + S columns out -- groups of 2, 4 or 8 columns, `base` groups a
chunk and `extra` chunks with one more -- sees C where it saw hnt.  The launch emulation (tests/launch_emu_support.py) runs the
kernel's own phase code at the HDPC thread counts the kernel uses (512 in the 768-thread workgroup, 256, 64), so every case below is
an encode with intermediate symbols and a decode against the oracle, byte for byte, at a K chosen for one branch:

    g2      n <= 2C: groups of 2
    g4      2C < n <= 4C: groups of 4
    sparse  just above 4C: groups of 8, fewer groups than chunks (base == 0, empty chunks)
    extra   groups of 8, every chunk has one (base >= 1) and some have one more (extra != 0) -- where a K <= 1100 gets there
    h11     K' = 1050 (K = 1033), the first with H = 11 HDPC rows (RFC 6330 table 2; rfc6330_tables.h: K' = 1032 still has 10)
    and n not a multiple of 8 with groups of 8 (the last column, MT's alpha^h one, in a partial group) in `sparse` or `extra`

Symbol sizes leave a partial last strip (fewer bytes than the strip width inside T), so some lanes of a chunk own bytes beyond T.
"""
import pytest

import nanorq_amd

# the variants that ship pieces (solve_body.h hdpc_piece: 16-byte strips; 12- and 8-byte strips keep whole-strip chunks):
# strip bytes, workgroup threads, threads of its HDPC phase, piece bytes, options that reach the variant, symbol sizes
VARIANTS = {
    "w16-768": dict(wb=16, NT=768, hnt=512, pb=8, opts={"big_wg": 1}, Ts=(40, 20)),
    "w16-256": dict(wb=16, NT=256, hnt=256, pb=4, opts={}, Ts=(40, 20)),
    # (single waves are taken while seven images share a CU's LDS: 16-byte strips up to K of about 900, so no H = 11 there)
    "w16-64": dict(wb=16, NT=64, hnt=64, pb=4, opts={"tiny_any": 1}, Ts=(40, 20), kmax=800),
}
KMAX = 1100
_N = {}


def columns(K):
    """n = K' + S and H of block size K"""
    if K not in _N:
        p = nanorq_amd.params(K)
        _N[K] = (p["Kp"] + p["S"], p["H"])
    return _N[K]


def chunking(n, C):
    """the rule of hdpc_chunks over C chunks: (columns a group, groups, groups every chunk has, chunks with one more)"""
    gsz = 2 if (n + 1) // 2 <= C else 4 if (n + 3) // 4 <= C else 8
    groups = (n + gsz - 1) // gsz
    return gsz, groups, groups // C, groups % C


BRANCHES = {
    "g2": lambda n, H, C: chunking(n, C)[0] == 2 and n > C,
    "g4": lambda n, H, C: chunking(n, C)[0] == 4,
    "sparse": lambda n, H, C: chunking(n, C)[0] == 8 and chunking(n, C)[2] == 0 and n % 8 != 0,
    "extra": lambda n, H, C: chunking(n, C)[0] == 8 and chunking(n, C)[2] >= 1 and chunking(n, C)[3] != 0 and n % 8 != 0,
    "h11": lambda n, H, C: H == 11,
}


def pick(C, branch, kmax=KMAX):
    """the smallest K <= kmax on that branch with C chunks (None: no such K)"""
    for K in range(6, kmax + 1):
        n, H = columns(K)
        if BRANCHES[branch](n, H, C):
            return K
    return None


# variant -> {branch: K}: what pick() gives, written out (a test module must not call into the library while pytest collects: in a
# run of the whole suite torch has to bring the GPU runtime up first, tests/conftest.py); test_the_branches_are_the_rule_s holds
# the table against pick()
PICKS = {
    "w16-768": {"g2": 226, "g4": 467, "sparse": 964, "h11": 1033},
    "w16-256": {"g2": 50, "g4": 102, "sparse": 226, "extra": 467, "h11": 1033},
    "w16-64": {"g2": 6, "g4": 21, "sparse": 50, "extra": 102},
}


def cases():
    return [pytest.param(name, branch, K, T, id="%s-%s-K%d-T%d" % (name, branch, K, T))
            for name, ks in PICKS.items() for branch, K in ks.items() for T in VARIANTS[name]["Ts"]]


def test_the_branches_are_the_rule_s():
    """the K chosen for a branch lands on it, and every variant has all the branches a K <= 1100 can reach"""
    assert columns(1033) == (1050 + 59, 11) and columns(1032)[1] == 10
    for name, v in VARIANTS.items():
        C = v["hnt"] // (v["wb"] // v["pb"])
        kmax = v.get("kmax", KMAX)
        have = {b for b in BRANCHES if pick(C, b, kmax) is not None}
        # (every chunk has a group of 8 from n = 8C - 7 columns on: beyond K = 1100 for more than 128 chunks)
        must = {"g2", "g4", "sparse"} | ({"extra"} if 8 * C - 7 + 8 < columns(kmax)[0] else set()) | ({"h11"} if kmax >= 1033 else set())
        assert have >= must, (name, have)
        assert PICKS[name] == {b: pick(C, b, kmax) for b in have}, name
        n, _ = columns(pick(C, "sparse"))
        assert 4 * C < n <= 4 * C + 24 and chunking(n, C)[1] < C


@pytest.mark.parametrize("name,branch,K,T", cases())
def test_piece_form_matches_oracle(name, branch, K, T):
    import launch_emu_support as S
    import oracle
    oracle.lib()
    v = VARIANTS[name]
    expect = dict(wb=v["wb"], NT=v["NT"])
    nblk = 1 if v["NT"] != 256 else 8
    S.run_encode(oracle, K, T, nblk, 3, v["opts"], want_inter=True, expect=expect)
    d = S.run_decode(oracle, K, T, nblk, 0.1, 2, v["opts"], want_inter=False, expect=expect)
    assert d["solved"] == nblk
