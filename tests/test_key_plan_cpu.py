"""The layout of a resident proving key (nim_groth16_amd/csrc/key_plan.hpp, built with g++), on the CPU: which index
ranges a shard holds, how many of its C1 slots are the library's padding, and where the entry lists of the B sets come
from.  Each rule is held to a restatement in Python.  (The form pointsB1 takes, b1_fold_form, lives in the same header;
tests/test_b1_fold_cpu.py holds it.)"""
import ctypes
import itertools
import os
import subprocess

import pytest

from nim_groth16_amd.distributed import shardRange as chunk_range

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpu_kernels")
PLAIN, EMPTY, DELTA = 0, 1, 2
NONE, FROM_B2, UNION = 0, 1, 2


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("key_plan") / "libkey_plan_shim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC",
                           os.path.join(HERE, "key_plan_shim.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    lib.shim_shard_range.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64)]
    lib.shim_shard_range.restype = None
    lib.shim_c1_padding.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32]
    lib.shim_c1_padding.restype = ctypes.c_uint64
    lib.shim_live_b_source.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_int, ctypes.c_int]
    lib.shim_live_b_kept.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int]
    return lib


def shard_range(shim, N, i, G):
    out = (ctypes.c_uint64 * 2)()
    shim.shim_shard_range(N, i, G, out)
    return out[0], out[1]


SIZES = (0, 1, 2, 63, 64, 65, 66, 1000)


def test_shard_ranges_are_ordered_disjoint_and_cover_everything(shim):
    for N in SIZES:
        for G in list(range(1, 10)) + [N + 3]:
            got = [shard_range(shim, N, i, G) for i in range(G)]
            assert got == [chunk_range(N, i, G) for i in range(G)], (N, G)          # the rule of distributed.py
            assert got == [((N * i) // G, (N * (i + 1)) // G) for i in range(G)]    # ... which is msm.nim:107-115
            assert got[0][0] == 0 and got[-1][1] == N
            assert all(lo <= hi for lo, hi in got)
            assert all(got[i][1] == got[i + 1][0] for i in range(G - 1))            # disjoint, no gap, in order
            assert max(hi - lo for lo, hi in got) - min(hi - lo for lo, hi in got) <= 1
    # the domain of the largest key, the last shard of many: no overflow on the way
    assert shard_range(shim, 1 << 27, 1023, 1024) == ((1 << 27) // 1024 * 1023, 1 << 27)


def test_c1_padding_counts_the_public_wires_of_the_range(shim):
    for N in SIZES:
        for npubs in sorted({0, 1, 5, max(N - 1, 0)}):
            if npubs + 1 > N:                   # not a key (npubs + 1 <= nvars)
                continue
            # every shard range of the key, and ranges that start before, at and after the first private wire
            edges = sorted({0, max(npubs, 0), npubs + 1, min(npubs + 2, N), N})
            ranges = {chunk_range(N, i, G) for G in range(1, 10) for i in range(G)}
            ranges |= {(lo, hi) for lo in edges for hi in edges if lo <= hi}
            for lo, hi in sorted(ranges):
                want = sum(1 for w in range(lo, hi) if w <= npubs)
                assert shim.shim_c1_padding(lo, hi, npubs) == want, (N, npubs, lo, hi)
    # over the shards of a key the padding adds up to the npubs + 1 public wires
    for G in range(1, 10):
        assert sum(shim.shim_c1_padding(*chunk_range(66, i, G), 5) for i in range(G)) == 6


def sparse(n_inf, n, pct):
    return n_inf > 0 and n_inf * 100 >= pct * n


def live_b(form, nw, b1_bitmap, b2_bitmap, dead, pct):
    """the three-way branch of key creation restated: -> (where liveB / deadB come from, whether the bitmap is kept).
    DELTA: the registered B1 set holds differences, and B1_i = (0,0) <=> B2_i = (0,0) in a key: B2's own count and bitmap.
    Otherwise the union of the two bitmaps, computed first and dropped again if the pair is dense."""
    if nw and form == DELTA and b2_bitmap:
        return FROM_B2, sparse(dead, nw, pct)
    if nw and b1_bitmap and b2_bitmap:
        return UNION, sparse(dead, nw, pct)
    return NONE, False


def test_live_list_decision_over_its_whole_domain(shim):
    seen = set()
    for form, nw, b1, b2, pct in itertools.product((PLAIN, EMPTY, DELTA), (0, 1, 9, 10, 66, 1000), (0, 1), (0, 1),
                                                   (0, 10, 101)):
        deads = sorted({0, 1, nw // 10, max(nw // 10 - 1, 0), nw // 10 + 1, nw // 2, nw})
        for dead in deads:
            if dead > nw:
                continue
            source = shim.shim_live_b_source(form, nw, b1, b2)
            kept = shim.shim_live_b_kept(source, dead, nw, pct)
            assert (source, bool(kept)) == live_b(form, nw, b1, b2, dead, pct), (form, nw, b1, b2, dead, pct)
            seen.add((source, bool(kept)))
    # every outcome is reached, the union that is computed and then dropped as dense among them
    assert seen == {(NONE, False), (FROM_B2, False), (FROM_B2, True), (UNION, False), (UNION, True)}
    # at a glance, under the default of 10 %: 6 dead wires of 66 are dense, 7 are sparse; "never" (101) keeps nothing,
    # 0 keeps every set with at least one dead wire
    assert [shim.shim_live_b_kept(UNION, d, 66, 10) for d in (0, 6, 7, 66)] == [0, 0, 1, 1]
    assert [shim.shim_live_b_kept(FROM_B2, d, 66, 101) for d in (0, 7, 66)] == [0, 0, 0]
    assert [shim.shim_live_b_kept(FROM_B2, d, 66, 0) for d in (0, 1, 66)] == [0, 1, 1]
    # an empty shard (more shards than wires) decides nothing, whatever the sets hold
    assert shim.shim_live_b_source(DELTA, 0, 1, 1) == NONE and shim.shim_live_b_kept(NONE, 0, 0, 0) == 0
