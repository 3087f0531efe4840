"""The sparse run of the B1 differences on the CPU (nim_groth16_amd/csrc/key_plan.hpp, msm_params.hpp, built with g++):
  * when a DELTA key takes it: b1_sparse_run, a function of live_delta alone, at 0, 1, B1_SPARSE_MAX and B1_SPARSE_MAX + 1;
  * the hit list its kernel builds from a live wire's scalar -- msm_hit_list, which walks the digits with the sort's own
    msm_digit_walk and places them with the sort's own msm_entry_place -- against a restatement of the signed-digit rule
    in Python integers, hit for hit and in window order, and against the scalar itself:
        sum over the hits of  sign * 2^s * weight(bucket) * 2^(c w)  ==  scalar   (as integers)
    with (s, w) read back from the entry's table index and weight() the inverse of the bucket layout (plain set: b + 1;
    class set: 4^z (2 v + 1), or 64 (x + 1) in class X; lean set: bucket set r of window w = stride * table + r)."""
import ctypes
import os
import random
import subprocess

import pytest

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpu_kernels")
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("b1_sparse") / "libb1_sparse_shim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC",
                           os.path.join(HERE, "b1_sparse_shim.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    lib.shim_b1_sparse_max.restype = ctypes.c_uint64
    lib.shim_b1_sparse_run.argtypes = [ctypes.c_uint64]
    u32p = ctypes.POINTER(ctypes.c_uint32)
    lib.shim_hit_list.argtypes = [u32p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                  ctypes.c_uint32, u32p, u32p]
    lib.shim_hit_list.restype = ctypes.c_uint32
    return lib


def test_the_sparse_run_is_taken_up_to_sparse_max_live_differences(shim):
    smax = shim.shim_b1_sparse_max()
    assert smax == 64
    assert shim.shim_b1_sparse_run(0) == 0            # no live difference: the key is EMPTY, there is nothing to run
    assert shim.shim_b1_sparse_run(1) == 1
    assert shim.shim_b1_sparse_run(smax) == 1
    assert shim.shim_b1_sparse_run(smax + 1) == 0
    assert [shim.shim_b1_sparse_run(v) for v in range(2, smax)] == [1] * (smax - 2)


def hit_list(shim, scalar, i, n, c, mtab, stride):
    words = (ctypes.c_uint32 * 8)(*[(scalar >> (32 * j)) & 0xffffffff for j in range(8)])
    out = (ctypes.c_uint32 * 512)()
    geom = (ctypes.c_uint32 * 4)()
    k = shim.shim_hit_list(words, i, n, c, mtab, stride, out, geom)
    return [(out[2 * j], out[2 * j + 1]) for j in range(k)], tuple(geom)


def signed_digits(scalar, c, nwin):
    """digit w in (-2^(c-1), 2^(c-1)]: the c-bit value plus the carry, taken negative (with a carry out) above 2^(c-1)"""
    half, out, carry = 1 << (c - 1), [], 0
    for w in range(nwin):
        raw = ((scalar >> (c * w)) & ((1 << c) - 1)) + carry
        carry = 1 if raw > half else 0
        out.append(raw - (carry << c))
    assert carry == 0 and sum(d << (c * w) for w, d in enumerate(out)) == scalar
    return out


def class_bucket(t, c):
    """msm_class_bucket restated: t = 2^s * weight, weight = 4^z (2 v + 1) for ctz(t) < 6, else 64 x in class X"""
    h, tz = 1 << (c - 1), (t & -t).bit_length() - 1
    if tz >= 6:
        return h // 2 + h // 8 + h // 32 + (t >> 6) - 1, 0
    z, v = tz >> 1, t >> (tz + 1)
    return (0, h // 2, h // 2 + h // 8)[z] + v, tz & 1


def class_weight(b, c):
    h = 1 << (c - 1)
    for z, (lo, size) in enumerate(((0, h // 2), (h // 2, h // 8), (h // 2 + h // 8, h // 32))):
        if lo <= b < lo + size:
            return 4 ** z * (2 * (b - lo) + 1)
    return 64 * (b - (h // 2 + h // 8 + h // 32) + 1)


def expected_hits(scalar, i, n, c, nwin, mtab, tstride):
    out = []
    for w, d in enumerate(signed_digits(scalar, c, nwin)):
        if d == 0:
            continue
        neg, mag = int(d < 0), abs(d)
        if mtab == 2:
            b, sel = class_bucket(mag, c)
            out.append((b, ((w + sel * nwin) * n + i) | (neg << 31)))
        elif tstride >= 2:
            out.append((((w % tstride) << (c - 1)) + mag - 1, ((w // tstride) * n + i) | (neg << 31)))
        else:
            out.append((mag - 1, (w * n + i) | (neg << 31)))
    return out


def value_of(hits, i, n, c, nwin, mtab, tstride):
    total = 0
    for slot, entry in hits:
        sign, pidx = -1 if entry >> 31 else 1, entry & 0x7fffffff
        table, wire = divmod(pidx, n)
        assert wire == i
        if mtab == 2:
            sel, w = divmod(table, nwin)
            assert sel in (0, 1)
            total += sign * (1 << sel) * class_weight(slot, c) << (c * w)
        elif tstride >= 2:
            r, b = slot >> (c - 1), slot & ((1 << (c - 1)) - 1)
            total += sign * (b + 1) << (c * (tstride * table + r))
        else:
            total += sign * (slot + 1) << (c * table)
    return total


def edge_scalars(c, nwin):
    half, mask = 1 << (c - 1), (1 << c) - 1
    top = 254 - c * (nwin - 1)                         # bits of the top window
    v = [0, 1, 2, R - 1, R - 2, half, half + 1, half - 1, mask, mask + 1]
    # a digit exactly at +2^(c-1) (no carry) and one just above it (negative, the carry moves into the next window),
    # in the first, a middle and the last whole window
    for w in (0, nwin // 2, nwin - 2):
        v += [half << (c * w), (half + 1) << (c * w), ((half + 1) << (c * w)) | (half << (c * (w + 1))),
              ((half + 1) << (c * w)) | ((half - 1) << (c * (w + 1)))]     # the carry lifts half - 1 to exactly half
    # a carry chain through all windows: every window full, so the first digit is -1, every further one 0 with a
    # carry, and the top window takes the last carry
    chain = (1 << (c * (nwin - 1))) - 1
    v += [chain, chain | (1 << (c * (nwin - 1))), (1 << 253) - 1, (1 << 253) + chain if top > 0 else chain]
    # ... and broken after w windows
    v += [(1 << (c * w)) - 1 for w in range(1, nwin)]
    # every window at half + 1: all digits negative but the top one
    v.append(sum((half + 1) << (c * w) for w in range(nwin - 1)) % R)
    return sorted({x % R for x in v})


CONFIGS = [
    # (n, c, mtab, stride): the bench key's registered sets (class bucket set); the class set at its smallest window;
    # plain sets at small windows; lean sets (tables at a stride)
    (1 << 20, 20, 2, 0), (1 << 16, 15, 2, 0), (256, 5, 1, 0), (1000, 8, 1, 0), (66, 6, 1, 1), (4096, 11, 1, 2),
    (4096, 9, 1, 3), (1 << 20, 16, 1, 4),
]


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda t: "n%d-c%d-m%d-s%d" % t)
def test_hit_list_is_the_signed_digit_rule_and_sums_to_the_scalar(shim, cfg):
    n, c, mtab, stride = cfg
    nwin = 254 // c + 1
    rng = random.Random(1000 * c + mtab)
    scalars = edge_scalars(c, nwin) + [rng.randrange(R) for _ in range(200)]
    for scalar in scalars:
        for i in (0, n - 1, n // 3):
            got, geom = hit_list(shim, scalar, i, n, c, mtab, stride)
            g_nwin, nbuckets, g_mtab, tstride = geom
            assert g_nwin == nwin and g_mtab == mtab and tstride == (min(stride, nwin) if stride >= 2 else 1)
            assert got == expected_hits(scalar, i, n, c, nwin, mtab, tstride), hex(scalar)
            assert all(slot < nbuckets for slot, _ in got)
            assert value_of(got, i, n, c, nwin, mtab, tstride) == scalar, hex(scalar)
            assert len(got) <= nwin and (scalar != 0 or got == [])


def test_edge_scalars_reach_what_they_were_built_for():
    """the restated digits of the edge cases: +2^(c-1) occurs, a negative digit with a carry occurs, and the chain
    carries through every window"""
    c, nwin = 20, 13
    half = 1 << (c - 1)
    assert signed_digits(half, c, nwin)[0] == half
    assert signed_digits(half + 1, c, nwin)[:2] == [-(half - 1), 1]
    assert signed_digits(((half + 1) | ((half - 1) << c)), c, nwin)[:3] == [-(half - 1), half, 0]
    d = signed_digits((1 << (c * (nwin - 1))) - 1, c, nwin)
    assert d == [-1] + [0] * (nwin - 2) + [1]
    assert sum(1 for x in signed_digits(R - 1, c, nwin) if x) > 1
