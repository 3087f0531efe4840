"""The circuit setup (g16_circuit_setup, g16_points_intt_g1/g2) on the CPU: the C ABI declares the calls; the launch plan
of nim_groth16_amd/csrc/circuit_setup_plan.hpp (built with g++) covers every butterfly, entry and wire exactly once; and
an integer model shows that the formulas of include/g16hip.h, applied to the logarithms of a powers of tau, give the
logarithms of the oracle's fake_circuit_setup with gamma = 1 -- every section, both flavours, the four circuits of
tests/circuit_audit_pictures.py.  The model is Python integers and the oracle's inverse NTT; nothing of the library runs."""
import ctypes
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import bn254_ref as o
from tests import circuit_audit_pictures as CA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "cpu_kernels")
CSRC = os.path.join(ROOT, "nim_groth16_amd", "csrc")
R = o.R


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
def test_header_declares_the_calls():
    text = open(os.path.join(ROOT, "include", "g16hip.h")).read()
    text = re.sub(r"\s+", " ", re.sub(r"\n \* ", " ", text))               # comment lines joined, white space collapsed
    for proto in ("int32_t g16_points_intt_g1(g16_ctx* ctx, const void* points, uint32_t log2n, void* out);",
                  "int32_t g16_points_intt_g2(g16_ctx* ctx, const void* points, uint32_t log2n, void* out);",
                  "int32_t g16_circuit_setup(g16_ctx* ctx, const g16_r1cs_desc* r1cs, const g16_ptau_desc* ptau, "
                  "const void* delta, g16_setup_points* out);"):
        assert proto in text, proto
    from nim_groth16_amd._lib import SYMBOLS
    assert {"g16_points_intt_g1", "g16_points_intt_g2", "g16_circuit_setup"} <= set(SYMBOLS)
    # what the header must say in so many words
    assert "only after a phase-2 contribution" in text and "section 10" in text and "sections 12-15" in text


# ---- the launch plan ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim():
    so, src = os.path.join(HERE, "libcircuit_setup_shim.so"), os.path.join(HERE, "circuit_setup_shim.cpp")
    deps = [src] + glob.glob(os.path.join(CSRC, "*.hpp"))
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", src, "-o", so])
    lib = ctypes.CDLL(so)
    u32, vp = ctypes.c_uint32, ctypes.c_void_p
    for name in ("shim_cs_block", "shim_cs_nbins", "shim_pintt_max_log2"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = u32, []
    for name in ("shim_bin_glog", "shim_bin_of", "shim_pintt_stages", "shim_pintt_butterflies", "shim_pintt_stage_grid",
                 "shim_pintt_twiddles"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = u32, [u32]
    lib.shim_pintt_rev.restype, lib.shim_pintt_rev.argtypes = u32, [u32, u32]
    lib.shim_pintt_stage.restype, lib.shim_pintt_stage.argtypes = None, [u32, u32, vp, vp, vp]
    lib.shim_pintt_check_stage.restype, lib.shim_pintt_check_stage.argtypes = ctypes.c_uint64, [u32, u32]
    lib.shim_cs_sum_plan.restype, lib.shim_cs_sum_plan.argtypes = None, [vp, u32, vp, vp]
    return lib


def _stage(shim, log2n, s):
    nb = shim.shim_pintt_butterflies(log2n)
    lo, hi, tw = (np.zeros(max(nb, 1), dtype=np.uint32) for _ in range(3))
    shim.shim_pintt_stage(log2n, s, lo.ctypes.data, hi.ctypes.data, tw.ctypes.data)
    return lo[:nb], hi[:nb], tw[:nb]


def test_every_butterfly_exactly_once_per_stage(shim):
    assert shim.shim_pintt_max_log2() == 24 and shim.shim_cs_block() == 64
    for log2n in range(0, 25):
        n = 1 << log2n
        assert shim.shim_pintt_stages(log2n) == log2n
        assert shim.shim_pintt_butterflies(log2n) == shim.shim_pintt_twiddles(log2n) == n // 2
        assert shim.shim_pintt_stage_grid(log2n) == (n // 2 + 63) // 64
        for s in range(log2n):
            assert shim.shim_pintt_check_stage(log2n, s) == 0, (log2n, s)
    # ... and independently of the shim's own check, in numpy, where that is quick
    for log2n in range(0, 13):
        n = 1 << log2n
        for s in range(log2n):
            lo, hi, tw = _stage(shim, log2n, s)
            assert sorted(np.concatenate([lo, hi]).tolist()) == list(range(n))
            assert ((hi - lo) == (1 << s)).all() and (tw < max(n // 2, 1)).all()
            assert (tw == (lo % (1 << s)) * (n >> (s + 1))).all() and ((lo >> s) % 2 == 0).all()
        rev = [shim.shim_pintt_rev(log2n, i) for i in range(n)]
        assert rev == [int(format(i, f"0{log2n}b")[::-1], 2) if log2n else 0 for i in range(n)]


def test_the_plan_is_the_inverse_ntt(shim):
    """the load pass and the stages, run over integers: the oracle's inverse NTT, with the factor per element the load
    pass applies (1/n for a plain transform)"""
    rng = o.SplitMix64(77)
    for log2n in range(0, 9):
        n = 1 << log2n
        D = o.Domain(n)
        xs = [rng.fr() for _ in range(n)]
        v = [0] * n
        for i, x in enumerate(xs):
            v[shim.shim_pintt_rev(log2n, i)] = x * D.invDomainSize % R
        tws = [pow(D.invDomainGen, k, R) for k in range(max(n // 2, 1))]
        for s in range(log2n):
            for lo, hi, tw in zip(*(a.tolist() for a in _stage(shim, log2n, s))):
                b = v[hi] * tws[tw] % R
                v[lo], v[hi] = (v[lo] + b) % R, (v[lo] - b) % R
        assert v == o.inverse_ntt(xs, D), log2n


def _python_bin(length):
    """spmv_params.hpp in words: 0: L <= 1, 1: L == 2, 2: L <= 4, 2 + g: 4 * 2^(g-1) < L <= 4 * 2^g (g = 1..6; the last
    bin takes every longer wire)"""
    if length <= 1:
        return 0
    if length == 2:
        return 1
    if length <= 4:
        return 2
    g = 1
    while g < 6 and length > (4 << g):
        g += 1
    return 2 + g


def test_every_wire_and_entry_in_exactly_one_bin(shim):
    nb = shim.shim_cs_nbins()
    assert nb == 9 and [shim.shim_bin_glog(b) for b in range(nb)] == [0, 0, 0, 1, 2, 3, 4, 5, 6]
    rng = np.random.default_rng(5)
    edges = [0, 1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 1000, 100003]
    lens = np.array(edges + rng.integers(0, 300, size=500).tolist() + [0] * 7, dtype=np.uint32)
    rng.shuffle(lens)
    for length in edges:
        assert shim.shim_bin_of(length) == _python_bin(length), length
    wires = np.full(len(lens), 0xffffffff, dtype=np.uint32)
    out = np.zeros(3 * nb, dtype=np.uint32)
    shim.shim_cs_sum_plan(lens.ctypes.data, len(lens), wires.ctypes.data, out.ctypes.data)
    first, count, grid = out[:nb].tolist(), out[nb:2 * nb].tolist(), out[2 * nb:].tolist()
    assert sorted(wires.tolist()) == list(range(len(lens)))                # every wire once
    assert sum(count) == len(lens) and first == [sum(count[:b]) for b in range(nb)]
    for b in range(nb):
        mine = wires[first[b]:first[b] + count[b]].tolist()
        assert mine == sorted(mine) and all(_python_bin(int(lens[w])) == b for w in mine)
        lanes = 1 << shim.shim_bin_glog(b)
        assert grid[b] == (count[b] * lanes + 63) // 64                    # enough lanes, less than a workgroup to spare
        # the lanes of a wire take its terms at a stride of `lanes`: every term exactly once
        for w in mine[:3] + mine[-3:]:
            taken = sorted(i for lane in range(lanes) for i in range(lane, int(lens[w]), lanes))
            assert taken == list(range(int(lens[w])))
    assert count[0] >= 8 and count[nb - 1] >= 4                            # empty wires, and wires beyond 128 terms


# ---- the formulas, in logarithms ---------------------------------------------------------------------------------------
def model_key(c: CA.Circuit, flavour, t: dict, delta: int, odd_of_doubled: bool) -> dict:
    """include/g16hip.h, "circuit setup", over the logarithms t of a powers of tau -> section -> [logarithms]"""
    L, nv, p = c.log2_domain, c.nvars, c.npubs
    n = 1 << L
    D = o.Domain(n)
    lag = {name: o.inverse_ntt(t[name][:n], D) for name in ("tauG1", "tauG2", "alphaTauG1", "betaTauG1")}
    A, B, C = c.triplets()
    A = A + [(c.ncons + i, i, 1) for i in range(p + 1)]

    def apply(entries, vec):
        out = [0] * nv
        for row, w, v in entries:
            out[w] = (out[w] + v * vec[row]) % R
        return out
    comb = [(x + y + z) % R for x, y, z in zip(apply(A, lag["betaTauG1"]), apply(B, lag["alphaTauG1"]), apply(C, lag["tauG1"]))]
    di = o.inv_fr(delta)
    if flavour == CA.JENSGROTH:
        h = [(t["tauG1"][i + n] - t["tauG1"][i]) % R for i in range(n)]
    elif odd_of_doubled:
        h = o.inverse_ntt(t["tauG1"][:2 * n], o.Domain(2 * n))[1::2]
    else:
        eta_inv, half = o.Domain(2 * n).invDomainGen, o.inv_fr(2)
        h = o.inverse_ntt([(t["tauG1"][j] - t["tauG1"][j + n]) * pow(eta_inv, j, R) % R * half % R for j in range(n)], D)
    return {"alpha1": [t["alphaTauG1"][0]], "beta1": [t["betaTauG1"][0]], "delta1": [delta % R], "beta2": [t["betaG2"][0]],
            "gamma2": [1], "delta2": [delta % R], "pointsIC": comb[:p + 1], "pointsA1": apply(A, lag["tauG1"]),
            "pointsB1": apply(B, lag["tauG1"]), "pointsB2": apply(B, lag["tauG2"]),
            "pointsC1": [di * x % R for x in comb[p + 1:]], "pointsH1": [di * x % R for x in h]}


@pytest.mark.parametrize("flavour", [CA.SNARKJS, CA.JENSGROTH])
@pytest.mark.parametrize("name", ["toy", "chain", "dup", "nopriv"])
def test_formulas_give_the_fake_setup_with_gamma_one(name, flavour):
    c = CA.circuits()[name]
    tw = CA.toxic(2000 + len(name))
    ident = lambda ks: [k % R for k in ks]                                   # noqa: E731  the key in log space
    t = CA.ptau_logs(tw.tau, tw.alpha, tw.beta, c.log2_domain + 1)
    for delta in (1, tw.delta):
        zk = o.fake_circuit_setup(o.R1CS(c.nvars, c.npubs, 0, c.nvars - c.npubs - 1, c.constraints),
                                  o.ToxicWaste(tw.alpha, tw.beta, 1, delta, tw.tau), CA.FLAVOUR[flavour], ident, ident)
        want = {s: [getattr(zk, s)] for s in CA.KEY_SECTIONS[:6]}
        want.update({s: list(getattr(zk, s)) for s in CA.KEY_SECTIONS[6:12]})
        for odd in (True, False):                                            # both forms of the snarkjs H points
            got = model_key(c, flavour, t, delta, odd)
            assert sorted(got) == sorted(want)
            for s in want:
                assert got[s] == want[s], (name, flavour, delta, odd, s)
    assert len(want["pointsC1"]) == c.nvars - c.npubs - 1 and len(want["pointsH1"]) == 1 << c.log2_domain
