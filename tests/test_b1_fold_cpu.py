"""pointsB1 folded into pointsA1, on the CPU.

A1 and B1 are multiplied by the same scalars, so with D_i = B1_i - A1_i the sum MSM(w, B1) equals MSM(w, A1) + MSM(w, D);
a key keeps D (or nothing at all) in place of pointsB1 where few enough of the D_i are live.  Held here, without a GPU:
  * the rule (b1_fold_form, nim_groth16_amd/csrc/key_plan.hpp) against a restatement in Python integers, exhaustively
    over small counts and at every boundary of its three forms, keys with 5 .. 50 % linear wires (whose B1 runs
    compacted, and which the fold must leave alone), the switch G16_B1_FOLD=0, and why the counts must be the whole
    key's and not a shard's;
  * what the form changes in a proof's launch plan: the arrangement the B1 run reads, and nothing else;
  * the device's point difference (nim_groth16_amd/csrc/b1_fold.cuh, built with g++) and a restatement of it on the
    oracle's curve, case by case, and the identity of the sums on random small sets."""
import ctypes
import os
import subprocess

import pytest

from oracle import bn254_ref as o

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpu_kernels")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN, EMPTY, DELTA = 0, 1, 2
SORT_W, SORT_WB = 0, 3


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("b1_fold") / "libb1_fold_shim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(HERE, "b1_fold_shim.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    lib.shim_b1_fold_form.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, ctypes.c_int]
    lib.shim_b1_plan.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32] + [ctypes.c_int] * 5 + \
        [ctypes.POINTER(ctypes.c_int)]
    lib.shim_g1_difference.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p]
    lib.shim_g1_difference.restype = None
    return lib


# ---- the rule ------------------------------------------------------------------------------------------------------------
def sparse(n_inf, n, pct):
    """points_sparse: a set with this many points at infinity runs on a compacted arrangement of its own"""
    return n_inf > 0 and n_inf * 100 >= pct * n


def form(live_b1, live_delta, n=None, pct=10, fold=1):
    """the rule in Python integers: the issue's threshold, and -- because the differences ride the arrangement of all n
    pairs, where only a wave of 64 entries that are all at infinity is skipped -- against a B1 that runs compacted
    (live_b1 entries) the differences must leave most waves empty.  n = None: a key whose B1 has no point at infinity."""
    n = live_b1 if n is None else n
    if not fold:
        return PLAIN
    if live_delta == 0:
        return EMPTY
    if live_delta * 100 > live_b1 * (100 - pct):
        return PLAIN
    if n >= live_b1 and sparse(n - live_b1, n, pct) and live_delta * 64 > live_b1:
        return PLAIN
    return DELTA


def issue_form(live_b1, live_delta, pct=10):
    """the three forms as the issue states them: what the rule answers for every key whose B1 does not run compacted"""
    if live_delta == 0:
        return EMPTY
    return DELTA if live_delta * 100 <= live_b1 * (100 - pct) else PLAIN


PCTS = (0, 1, 10, 33, 50, 99, 100, 101)


def test_rule_exhaustively_over_small_counts(shim):
    for pct in PCTS:
        for live_b1 in range(0, 41):
            for live_delta in range(0, 61):
                # B1 without a point at infinity: never compacted, the issue's rule to the letter
                assert shim.shim_b1_fold_form(live_b1, live_delta, live_b1, pct, 1) == issue_form(live_b1, live_delta, pct), \
                    (pct, live_b1, live_delta)
                for n in (live_b1 + 1, live_b1 * 10 // 9, live_b1 * 10 // 9 + 1, 2 * live_b1 + 3, 70 * live_b1):
                    got = shim.shim_b1_fold_form(live_b1, live_delta, n, pct, 1)
                    assert got == form(live_b1, live_delta, n, pct), (pct, live_b1, live_delta, n)
                    # the second condition only ever turns DELTA into PLAIN
                    assert got == issue_form(live_b1, live_delta, pct) or \
                        (got == PLAIN and issue_form(live_b1, live_delta, pct) == DELTA)


def test_rule_at_the_boundaries_of_its_forms(shim):
    top = (1 << 26) - 1                                     # the largest point set the library registers
    for pct in PCTS:
        for live_b1 in (1, 2, 9, 10, 11, 99, 100, 101, 1000, 1 << 20, (1 << 20) + 1, top):
            n = live_b1                                     # B1 not compacted: the issue's three forms
            edge = max(live_b1 * (100 - pct) // 100, 0)     # the largest live_delta that is still DELTA (if positive)
            for live_delta in {0, 1, 2, max(edge - 1, 0), edge, edge + 1, live_b1 - 1, live_b1, live_b1 + 1, top}:
                got = shim.shim_b1_fold_form(live_b1, live_delta, n, pct, 1)
                assert got == issue_form(live_b1, live_delta, pct) == form(live_b1, live_delta, n, pct), \
                    (pct, live_b1, live_delta)
            if pct <= 100 and edge >= 1:
                assert shim.shim_b1_fold_form(live_b1, edge, n, pct, 1) == DELTA
            assert shim.shim_b1_fold_form(live_b1, edge + 1, n, pct, 1) == PLAIN
            assert shim.shim_b1_fold_form(live_b1, 0, n, pct, 1) == EMPTY
            # B1 compacted (a key twice as long, the other half absent from B): DELTA up to live_b1 / 64 differences
            n2 = 2 * live_b1
            wave_edge = live_b1 // 64
            for live_delta in {1, max(wave_edge - 1, 1), max(wave_edge, 1), wave_edge + 1, edge, edge + 1}:
                assert shim.shim_b1_fold_form(live_b1, live_delta, n2, pct, 1) == form(live_b1, live_delta, n2, pct)
            if 1 <= pct <= 50 and 1 <= wave_edge <= edge:
                assert shim.shim_b1_fold_form(live_b1, wave_edge, n2, pct, 1) == DELTA
                assert shim.shim_b1_fold_form(live_b1, wave_edge + 1, n2, pct, 1) == PLAIN
            assert shim.shim_b1_fold_form(live_b1, 0, n2, pct, 1) == EMPTY
    # the defaults at a glance: 10 % of B1's live points must go
    assert shim.shim_b1_fold_form(1000, 900, 1000, 10, 1) == DELTA and shim.shim_b1_fold_form(1000, 901, 1000, 10, 1) == PLAIN
    # ... and compaction of B1 starts at 10 % of its points at infinity: one wire short of it the issue's rule alone
    assert shim.shim_b1_fold_form(901, 800, 1000, 10, 1) == DELTA and shim.shim_b1_fold_form(900, 800, 1000, 10, 1) == PLAIN
    # no live point in B1 and none in the difference: both sets are infinity throughout
    assert shim.shim_b1_fold_form(0, 0, 10, 10, 1) == EMPTY
    # B1 empty, A1 not: the difference is -A1, more live points than B1 has
    assert shim.shim_b1_fold_form(0, 5, 10, 10, 1) == PLAIN
    # the Poseidon shape: a third of the wires absent from B, so the difference is live on more wires than B1 is
    assert shim.shim_b1_fold_form(2000, 3000, 3000, 10, 1) == PLAIN
    # G16_INF_COMPACT=101 ("never") leaves only the EMPTY form
    assert shim.shim_b1_fold_form(1000, 1, 1000, 101, 1) == PLAIN and shim.shim_b1_fold_form(1000, 0, 1000, 101, 1) == EMPTY


@pytest.mark.parametrize("lin_pct", [5, 9, 10, 20, 30, 50])
def test_keys_with_linear_wires_keep_b1_once_it_runs_compacted(shim, lin_pct):
    """mixedCircuit(lin_pct): that share of the wires is absent from B (B1 at infinity, A1 not), the others are symmetric.
    live_b1 = (100 - lin_pct) % of n and live_delta = lin_pct % of n.  Below 10 % B1 runs on the arrangement of all n
    pairs and the differences, on the same arrangement, cost what it did: DELTA, as the issue's threshold says.  From
    10 % on B1 runs compacted, at live_b1 additions; the differences would meet a live lane in nearly every wave of 64
    and cost about n: the key keeps pointsB1, although the issue's threshold alone would have let it go (up to 47 %)."""
    n = 1 << 20
    live_delta = (n * lin_pct + 99) // 100                  # rounded up: at least that share
    live_b1 = n - live_delta
    want = DELTA if lin_pct < 10 else PLAIN
    assert form(live_b1, live_delta, n) == want
    assert shim.shim_b1_fold_form(live_b1, live_delta, n, 10, 1) == want
    if lin_pct in (10, 20, 30):
        assert issue_form(live_b1, live_delta) == DELTA
    # what the fold is for survives compaction: a handful of live differences leaves nearly every wave empty
    assert shim.shim_b1_fold_form(live_b1, 2, n, 10, 1) == DELTA
    assert shim.shim_b1_fold_form(live_b1, live_b1 // 64, n, 10, 1) == DELTA


def test_switch_forces_plain(shim):
    for pct in PCTS:
        for live_b1, live_delta in ((0, 0), (10, 0), (1000, 1), (1000, 900), (1000, 2000), (1 << 26, 0)):
            for n in (live_b1, 2 * live_b1 + 1):
                assert shim.shim_b1_fold_form(live_b1, live_delta, n, pct, 0) == PLAIN


def test_counts_are_the_whole_keys_not_a_shards(shim):
    """A key whose live differences all lie in its first half: by its own counts the first shard would keep pointsB1 and
    the second would drop it, and the combine kernel -- which adds the A1 slots of ALL records to the B1 slots, or of
    none -- would get a mix.  By the whole key's counts every shard reaches the same answer."""
    n = 1000
    differs = [i < 460 for i in range(n)]                   # B1_i != A1_i
    live = [True] * n                                        # B1_i != infinity
    whole = form(sum(live), sum(differs), n)
    shards = []
    for k in range(2):
        lo, hi = n * k // 2, n * (k + 1) // 2
        shards.append(form(sum(live[lo:hi]), sum(differs[lo:hi]), hi - lo))
    assert whole == DELTA and shards == [PLAIN, EMPTY]
    assert shim.shim_b1_fold_form(sum(live), sum(differs), n, 10, 1) == whole
    assert [shim.shim_b1_fold_form(500, 460, 500, 10, 1), shim.shim_b1_fold_form(500, 0, 500, 10, 1)] == shards


# ---- the plan ------------------------------------------------------------------------------------------------------------
def test_the_form_moves_nothing_in_the_plan_but_the_arrangement_b1_reads(shim):
    for nw, nh, log2n in ((254, 256, 8), (1 << 20, 1 << 20, 20), (300, 0, 10), (0, 512, 9)):
        for liveA in (0, 1):
            for liveB in (0, 1):
                for cfg_equal in (0, 1):
                    for batch in (0, 1):
                        sort_b = ctypes.c_int(-9)
                        for f in (PLAIN, EMPTY, DELTA):
                            got = shim.shim_b1_plan(nw, nh, log2n, liveA, liveB, cfg_equal, batch, f, ctypes.byref(sort_b))
                            assert sort_b.value == (SORT_WB if liveB else SORT_W)
                            # the difference set is live where A1 OR B1 is: not covered by the B1 | B2 bitmap
                            assert got == (sort_b.value if f == PLAIN else SORT_W), (nw, liveA, liveB, batch, f)


# ---- the difference ------------------------------------------------------------------------------------------------------
def delta(b, a):
    """B1_i - A1_i on the oracle's curve, case by case as key creation computes it"""
    G = o.G1
    if a == b:
        return G.inf
    if G.is_inf(a):
        return b
    if G.is_inf(b):
        return G.neg(a)
    if b == G.neg(a):
        return G.to_affine(G.jdbl(G.to_jac(b)))
    return G.add(b, G.neg(a))


def _points(seed, n):
    rng = o.SplitMix64(seed)
    gen = (1, 2)
    return [o.G1.mul(rng.fr(), gen) for _ in range(n)]


def _cases():
    p, q, r = _points(3, 3)
    G = o.G1
    return {"equal": (p, p), "both at infinity": (G.inf, G.inf), "A1 at infinity": (q, G.inf),
            "B1 at infinity": (G.inf, q), "opposite": (G.neg(r), r), "general": (p, q), "general, swapped": (q, p),
            "B1 = 2 A1": (G.add(p, p), p)}


@pytest.mark.parametrize("name", list(_cases()))
def test_difference_case_by_case(shim, name):
    b, a = _cases()[name]
    G = o.G1
    want = G.add(b, G.neg(a))                                # the definition: the oracle's own addition
    assert delta(b, a) == want and G.is_on_curve(want)
    assert G.add(a, want) == b                               # A1_i + D_i = B1_i
    out = ctypes.create_string_buffer(64)
    shim.shim_g1_difference(o.g1_to_bytes(b), o.g1_to_bytes(a), out)
    assert out.raw == o.g1_to_bytes(want), name              # the device's code: the same point in its canonical bytes
    if name in ("equal", "both at infinity"):
        assert out.raw == bytes(64)
    if name == "opposite":
        assert want == G.add(b, b) and not G.is_inf(want)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_sums_agree_on_random_small_sets(shim, seed):
    """B1sum = A1sum + Dsum with the D_i from the device's code, over sets that mix every case"""
    G = o.G1
    rng = o.SplitMix64(100 + seed)
    n = 24
    base = _points(seed, n)
    a1, b1 = [], []
    for i, p in enumerate(base):
        kind = rng.next() % 6
        other = base[(i + 7) % n]
        a, b = {0: (p, p), 1: (G.inf, p), 2: (p, G.inf), 3: (G.inf, G.inf), 4: (p, G.neg(p)), 5: (p, other)}[kind]
        a1.append(a), b1.append(b)
    d = []
    for a, b in zip(a1, b1):
        out = ctypes.create_string_buffer(64)
        shim.shim_g1_difference(o.g1_to_bytes(b), o.g1_to_bytes(a), out)
        d.append(o.g1_from_bytes(out.raw))
        assert d[-1] == delta(b, a)
    w = [rng.fr() for _ in range(n - 3)] + [0, 1, o.R - 1]
    assert G.msm_naive(w, b1) == G.add(G.msm_naive(w, a1), G.msm_naive(w, d))
    # the counts the rule takes, as the key-creation kernel counts them: 64-byte equality and 64 zero bytes
    live_b1 = sum(o.g1_to_bytes(b) != bytes(64) for b in b1)
    live_delta = sum(o.g1_to_bytes(a) != o.g1_to_bytes(b) for a, b in zip(a1, b1))
    assert live_delta == sum(not G.is_inf(x) for x in d) and live_b1 == sum(not G.is_inf(b) for b in b1)
