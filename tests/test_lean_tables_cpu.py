"""Window tables at a stride (lean point sets) on the CPU: the slot function that the sort kernels index tables and
bucket sets with, held to the identity it rests on in Python integers; the plans of a stride-1 set held to the plans of
the stride-less call, field by field; the plans of a lean set held to their rule; and g16_points_plan -- a pure function
of the C ABI, called here with no device present -- held to the same choice and to the byte formula."""
import ctypes
import glob
import os
import random
import subprocess

import pytest

from tests.test_gpu_knobs import KNOBS
from tests.test_msm_plan_cpu import (BS_LOG, FR_BITS, KNOB_ORDER, NS, PART_MAX, PLAIN, parse_knobs)

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpu_kernels")
CSRC = os.path.join(HERE, "..", "..", "nim_groth16_amd", "csrc")

PARAMS = ("n", "c", "nwin", "nbuckets", "seg", "scalars_mont", "tables", "max_extra", "mtab", "tstride")
SORT = ("lo_bits", "nparts", "ptiles", "nth", "use_part", "fused", "nblk", "ntiles", "nt2", "pblk")
TAIL = ("rc", "nchunks", "nsets", "log2ks", "cps", "r2", "r2_threads", "r2_lds", "fold", "heavy1", "heavy3")
FIELDS = PARAMS + SORT + TAIL + ("sort_bytes", "job_bytes")


@pytest.fixture(scope="module")
def lean():
    so, src = os.path.join(HERE, "liblean_shim.so"), os.path.join(HERE, "lean_shim.cpp")
    deps = [src] + glob.glob(os.path.join(CSRC, "*.hpp"))
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", src, "-o", so])
    lib = ctypes.CDLL(so)
    u32p, u64p, intp = (ctypes.POINTER(t) for t in (ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int))
    lib.shim_window_slot.restype = lib.shim_table_choice.restype = lib.shim_lean_plan.restype = None
    lib.shim_window_slot.argtypes = [ctypes.c_uint32, ctypes.c_uint32, u32p]
    lib.shim_table_choice.argtypes = [ctypes.c_uint64, ctypes.c_uint32, intp, u32p]
    lib.shim_lean_plan.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32, ctypes.c_int,
                                   ctypes.c_int, intp, u64p]
    return lib


def knob_array(env):
    k = parse_knobs(env)
    return (ctypes.c_int * len(KNOB_ORDER))(*[k[name] for name in KNOB_ORDER])


def slot(lean, w, s):  # noqa: F811
    out = (ctypes.c_uint32 * 2)()
    lean.shim_window_slot(w, s, out)
    return out[0], out[1]


def plan(lean, n, mode, stride, is_g1, narrow_tail, env, flags=1):  # noqa: F811
    out = (ctypes.c_uint64 * 33)()
    lean.shim_lean_plan(n, flags, mode, stride, int(is_g1), int(narrow_tail), knob_array(env), out)
    return dict(zip(FIELDS, out))


def choice(lean, n, stride, env):  # noqa: F811
    out = (ctypes.c_uint32 * 5)()
    lean.shim_table_choice(n, stride, knob_array(env), out)
    return dict(zip(("c", "mtab", "stride", "ntables", "fits"), out))


def test_slot_function_splits_the_window_sum(lean):
    """sum_w 2^(c w) d_w == sum_r 2^(c r) sum_j 2^(c s j) d_(s j + r) over random signed digits, for every stride from 1
    to nwin; every (table, set) with s j + r < nwin is hit exactly once and the tables stay below ceil(nwin / s)"""
    rng = random.Random(20)
    for c in (5, 8, 13, 16):
        nwin = FR_BITS // c + 1
        half = 1 << (c - 1)
        d = [rng.randint(-half, half) for _ in range(nwin)]
        d[0], d[-1] = half, -half                       # the extreme digits at both ends
        want = sum(d[w] << (c * w) for w in range(nwin))
        for s in range(1, nwin + 1):
            ntables = -(-nwin // s)
            sets = [0] * s
            seen = set()
            for w in range(nwin):
                j, r = slot(lean, w, s)
                assert (j, r) == (w // s, w % s) and s * j + r == w and j < ntables and r < s, (c, s, w, j, r)
                assert (j, r) not in seen
                seen.add((j, r))
                sets[r] += d[w] << (c * s * j)          # the table holds 2^(c s j) P: bucket set r sums what it gathers
            assert seen == {(j, r) for j in range(ntables) for r in range(s) if s * j + r < nwin}, (c, s)
            assert sum(sets[r] << (c * r) for r in range(s)) == want, (c, s)
        # the two ends that divide nothing: no tables (every window its own set) and a table per window (one set)
        for w in range(nwin):
            assert slot(lean, w, 0) == (0, w) and slot(lean, w, 1) == (w, 0)


def grid():
    for env in [{}] + KNOBS:
        for n in NS:
            for is_g1 in (True, False):
                for narrow_tail in (False, True):
                    yield env, n, is_g1, narrow_tail


def test_stride_one_plans_equal_the_stride_less_plans(lean):
    """msm_params, msm_sort_plan, msm_tail_plan and both workspaces: a registered set at stride 0 and at stride 1 (written
    into table_cfg as 1 << 16) plans exactly what the stride-less table_cfg plans, on the grid of test_msm_plan_cpu"""
    for env, n, is_g1, narrow_tail in grid():
        for flags in (1, 0):
            base = plan(lean, n, 1, 0, is_g1, narrow_tail, env, flags)
            assert base["tables"] == 1 and base["tstride"] == 1, (env, n)
            for stride in (0, 1):
                got = plan(lean, n, 2, stride, is_g1, narrow_tail, env, flags)
                assert got == base, (env, n, is_g1, narrow_tail, stride, [(f, got[f], base[f]) for f in FIELDS
                                                                          if got[f] != base[f]])
        # ... and a plain MSM carries no stride
        assert plan(lean, n, 0, 0, is_g1, narrow_tail, env)["tstride"] == 0
    for env in [{}] + KNOBS:
        for n in NS:
            c0, c1 = choice(lean, n, 0, env), choice(lean, n, 1, env)
            assert c0 == c1 and c0["stride"] == 1 and c0["ntables"] == c0["mtab"] * (FR_BITS // c0["c"] + 1), (env, n)


def lean_window(n, forced, s):
    """the cost model of a lean set: the one-shot rule (cap 16, 31-bit entries, no short top window) over min(s, nwin)
    bucket sets"""
    if forced:
        return forced
    best, best_cost = 5, 1e300
    for c in range(5, 17):
        nwin = FR_BITS // c + 1
        if (nwin * n) >> 31:
            continue
        if FR_BITS - (nwin - 1) * c < min(c - 2, 6) and c > 5:
            continue
        cost = 10.0 * float(n) * nwin + 28.0 * float(min(s, nwin)) * float(1 << (c - 1))
        if cost < best_cost:
            best, best_cost = c, cost
    return best


def test_lean_plans(lean):
    for env, n, is_g1, narrow_tail in grid():
        k = parse_knobs(env)
        for s in (2, 3, 4, 5, 7, 16, 51, 58, 255):
            ch = choice(lean, n, s, env)
            p = plan(lean, n, 2, s, is_g1, narrow_tail, env)
            where = (env, n, is_g1, narrow_tail, s, ch, p)
            c, nwin = p["c"], p["nwin"]
            assert c == ch["c"] == lean_window(max(n, 1), k["table_window"], s) and nwin == FR_BITS // c + 1, where
            assert k["table_window"] or c <= 16, where                     # the one-shot cap, unless the window is forced
            s_eff = min(s, nwin)
            assert ch["stride"] == s_eff == p["tstride"] and ch["mtab"] == 1 == p["mtab"] and p["tables"] == 1, where
            assert p["nbuckets"] == s_eff << (c - 1), where
            assert ch["ntables"] == -(-nwin // s_eff), where
            assert ch["fits"] == int(nwin * n < 1 << 31) and (not ch["fits"] or ch["ntables"] * n < 1 << 31), where
            assert k["table_window"] or ch["fits"], where
            # the tail: a plain MSM of s windows
            assert (p["nsets"], p["fold"], p["log2ks"]) == (s_eff, PLAIN, 0) and p["nsets"] <= 64, where
            assert p["nchunks"] * p["rc"] == p["nbuckets"] and p["nsets"] * p["cps"] == p["nchunks"], where
            assert p["cps"] * p["rc"] == 1 << (c - 1), where
            # the sort follows nbuckets
            assert p["lo_bits"] == min(c - 1, BS_LOG) and p["nparts"] << p["lo_bits"] == p["nbuckets"], where
            assert not p["use_part"] or p["nparts"] <= PART_MAX, where
    # a stride of nwin or more is the one-shot layout with the points resident: one table, the plain MSM's buckets
    p, q = plan(lean, 1 << 20, 2, 255, True, False, {}), plan(lean, 1 << 20, 0, 0, True, False, {})
    assert (p["c"], p["tstride"], p["nbuckets"], p["nsets"]) == (16, 16, q["nbuckets"], q["nsets"])
    assert choice(lean, 1 << 20, 255, {})["ntables"] == 1
    # recorded: the 2^20 key at stride 2 and 4
    for s, c, ntab in ((2, 16, 8), (4, 16, 4)):
        ch = choice(lean, 1 << 20, s, {})
        assert (ch["c"], ch["ntables"]) == (c, ntab), (s, ch)


def test_points_plan_through_the_c_abi(lean):
    """g16_points_plan needs no device and no context: bytes == ntables * n * 64 (G1) or * 128 (G2), window and tables as
    the shim's choice under the knobs of this process"""
    from nim_groth16_amd import points_plan
    from nim_groth16_amd._lib import G16Error, load_library
    env = {k: v for k, v in os.environ.items() if k.startswith("G16_")}
    for n in NS:
        for s in (0, 1, 2, 3, 4, 5, 16, 58):
            ch = choice(lean, n, s, env)
            c, ntables = ch["c"], ch["ntables"]
            assert ch["fits"]
            for group, size in ((1, 64), (2, 128)):
                assert points_plan(group, n, s) == (c, ntables, ntables * n * size), (n, s, group)
    # a lean set shrinks by the formula: ceil(nwin / s) tables against nwin of a stride-1 set with one table per window
    c, ntables, nbytes = points_plan(1, 1 << 20, 2)
    assert (c, ntables, nbytes) == (16, 8, 8 << 26)
    # NULL out pointers are allowed; bad arguments are refused
    lib = load_library()
    assert lib.g16_points_plan(1, 1000, 2, None, None, None) == 0
    for bad in ((0, 1000), (3, 1000), (1, 1 << 26)):
        with pytest.raises(G16Error):
            points_plan(bad[0], bad[1], 2)
