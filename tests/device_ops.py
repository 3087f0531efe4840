"""Operands and expected words for the op table of tests/kernels/devops.inc: one deterministic generator (fixed seeds)
shared by tests/test_device_ops_cpu.py (g++ build of the headers: the portable branches) and
tests/test_gpu_device_ops.py (libg16devops.so: the inline-asm / builtin branches in every product configuration).

Everything expected here is computed from plain Python integers (oracle/bn254_ref.py for the group law), bit for bit.
The bounds of the lazily reduced 9x29 operands are taken from tools/ff29_model.py (imported, not restated): its loop
invariants give the value bounds, its kform() the limb bounds of the subtrahends, and every product tuple is run through
its mont() / sqr(), which assert the 64-bit column and 32-bit limb bounds the C++ relies on."""
import ctypes
import functools
import importlib.util
import math
import os
import random
import zlib

import numpy as np

from oracle import bn254_ref as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("ff29_model", os.path.join(ROOT, "tools", "ff29_model.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)

P, R = o.P, o.R
MONT = 1 << 256
B29, L29, MASK = M.B, M.L, M.MASK
R261 = M.R
NRANDOM = 4096          # random tuples per op, on top of the edge tuples
VARIANTS = ("plain", "g1acc", "serial", "g2acc", "calls")


def _rng(name):
    return random.Random(zlib.crc32(name.encode()))


def w8(x):
    """256-bit integer -> 8 little-endian 32-bit words"""
    assert 0 <= x < (1 << 256)
    return [(x >> (32 * i)) & 0xffffffff for i in range(8)]


def from_w8(ws):
    return sum(int(x) << (32 * i) for i, x in enumerate(ws))


# ---- canonical edge sets ---------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def edge_set(m):
    Rm = MONT % m
    Ri = pow(Rm, -1, m)
    s = [0, 1, 2, m - 1, m - 2, (m + 1) // 2, (m - 1) // 2, Rm, Ri]
    for k in list(range(32, 256, 32)) + list(range(29, 256, 29)):    # every limb boundary of both radices
        s += [1 << k, (1 << k) - 1]
    top32, top29 = m >> 224, m >> 232
    s += [((1 << 224) - 1) | (t << 224) for t in (1, top32 - 1, top32 >> 1)]     # limbs all ones below the top limb
    s += [((1 << 232) - 1) | (t << 232) for t in (1, top29 - 1, top29 >> 1)]
    # the inversion edge list of test_field_formulas (signed 30-bit limbs of the division-step inversion)
    s += [3, 1 << 30, (1 << 30) - 1, 1 << 60, (1 << 240) + 1, (1 << 253) % m, m // 3, 0x3fffffff << 30, (1 << 128) - 1,
          5 ** 100 % m]
    out = []
    for x in s:
        assert 0 <= x < m, hex(x)
        if x not in out:
            out.append(x)
    return tuple(out)


def pair_tuples(name, edges, arity, rand, extra=(), nrandom=None):
    """all ordered pairs of `edges` in the first two slots (the other slots walk the set with coprime strides), then
    `extra`, then NRANDOM (or `nrandom`) random tuples; one more random tuple if the count would fill the last 64-lane
    block"""
    rng = _rng(name)
    nrandom = NRANDOM if nrandom is None else nrandom
    n = len(edges)
    out = []
    for i, a in enumerate(edges):
        for j, b in enumerate(edges):
            out.append([a, b] + [edges[(i * (3 + 2 * k) + j * (5 + 2 * k) + k) % n] for k in range(arity - 2)][:arity - 2])
    if arity == 1:
        out = [[a] for a in edges]
    out += [list(t) for t in extra]
    out += [[rand(rng) for _ in range(arity)] for _ in range(nrandom)]
    if len(out) % 64 == 0:
        out.append([rand(rng) for _ in range(arity)])
    return out


class Case:
    """inp, exp: uint32 arrays [n, words]; slots: (name, first word, words) of the output; post: optional extra check
    of one output row (raises AssertionError)"""

    def __init__(self, op, inp, exp, slots, post=None):
        self.op, self.slots, self.post = op, slots, post
        self.inp = np.ascontiguousarray(np.array(inp, dtype=np.uint64).astype(np.uint32))
        self.exp = np.ascontiguousarray(np.array(exp, dtype=np.uint64).astype(np.uint32))
        assert self.inp.shape[0] == self.exp.shape[0] and self.inp.shape[0] % 64 != 0, (op, self.inp.shape)


# ---- Field<Fp>, Field<Fr> --------------------------------------------------------------------------------------------
def _field(prefix):
    return P if prefix == "fp" else R


def case_field_all(prefix):
    m = _field(prefix)
    Rm = MONT % m
    Ri = pow(Rm, -1, m)
    i2 = pow(2, -1, m)
    tup = pair_tuples(prefix + "_all", edge_set(m), 2, lambda r: r.randrange(m))
    inp, exp = [], []
    for a, b in tup:
        inp.append(w8(a) + w8(b))
        res = [(a + b) % m, (a - b) % m, a * b * Ri % m, a * a * Ri % m, (-a) % m, 2 * a % m, a * i2 % m, a * Ri % m,
               a * Rm % m, 2 * a % m, 3 * a % m, 4 * a % m, 8 * a % m]
        exp.append(sum((w8(x) for x in res), []))
    names = ["add", "sub", "mul", "sqr", "neg", "dbl", "div2", "from_mont", "to_mont", "mul_small2", "mul_small3",
             "mul_small4", "mul_small8"]
    return Case(prefix + "_all", inp, exp, [(nm, 8 * i, 8) for i, nm in enumerate(names)])


def case_field_dot2(prefix):
    m = _field(prefix)
    Ri = pow(MONT, -1, m)
    edges = edge_set(m) + (m,)      # operands <= m: neg_raw(0) = m is a legal mul2 operand
    tup = pair_tuples(prefix + "_dot2", edges, 4, lambda r: r.randrange(m + 1))
    inp = [sum((w8(x) for x in t), []) for t in tup]
    exp = [w8((a * b + c * d) * Ri % m) + w8((a * b - c * d) * Ri % m) + w8(m - a) for a, b, c, d in tup]
    return Case(prefix + "_dot2", inp, exp, [("mul2", 0, 8), ("mulsub", 8, 8), ("neg_raw", 16, 8)])


def case_field_dot4(prefix):
    m = _field(prefix)
    Ri = pow(MONT, -1, m)
    edges = edge_set(m) + (m,)
    tup = pair_tuples(prefix + "_dot4", edges, 8, lambda r: r.randrange(m + 1), extra=[[m] * 8, [m - 1] * 8])
    inp = [sum((w8(x) for x in t), []) for t in tup]
    exp = [w8((t[0] * t[1] + t[2] * t[3] + t[4] * t[5] + t[6] * t[7]) * Ri % m) for t in tup]
    return Case(prefix + "_dot4", inp, exp, [("mul4", 0, 8)])


def case_field_cmp(prefix):
    m = _field(prefix)
    edges = edge_set(m) + (m, m + 1, (1 << 256) - 1, 1 << 255, m + (1 << 224))
    tup = pair_tuples(prefix + "_cmp", edges, 2, lambda r: r.choice([r.randrange(1 << 256), r.randrange(m)]))
    inp = [w8(a) + w8(b) for a, b in tup]
    exp = [[(1 if a >= b else 0) | (2 if a < m else 0)] for a, b in tup]
    return Case(prefix + "_cmp", inp, exp, [("geq | is_canonical << 1", 0, 1)])


def case_field_inv(prefix, which):
    """canonical operands only (Field::inv loops until g = 0; the CPU run of these very vectors shows each ends)"""
    m = _field(prefix)
    Rm = MONT % m
    tup = pair_tuples(prefix + which, edge_set(m), 1, lambda r: r.randrange(m))
    inp = [w8(a) for (a,) in tup]
    exp = [w8(pow(a, -1, m) * Rm * Rm % m if a else 0) for (a,) in tup]
    return Case(prefix + which, inp, exp, [(which.strip("_"), 0, 8)])


# ---- Fp2 -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def fp2_edges():
    e = edge_set(P)
    n = len(e)
    out = [(e[i], e[(7 * i + 3) % n]) for i in range(n)]
    out += [(x, 0) for x in (0, 1, P - 1)] + [(0, x) for x in (1, P - 1)] + [(P - 1, P - 1), (1, 1)]
    return tuple(dict.fromkeys(out))


def _w16(a):
    return w8(a[0]) + w8(a[1])


def _f2m(a, b, Ri):   # Montgomery-domain Fp2 product of raw residues
    return ((a[0] * b[0] - a[1] * b[1]) * Ri % P, (a[0] * b[1] + a[1] * b[0]) * Ri % P)


def case_fp2_all():
    Ri = pow(MONT, -1, P)
    tup = pair_tuples("fp2_all", fp2_edges(), 2, lambda r: (r.randrange(P), r.randrange(P)))
    inp, exp = [], []
    for a, b in tup:
        inp.append(_w16(a) + _w16(b))
        res = [((a[0] + b[0]) % P, (a[1] + b[1]) % P), ((a[0] - b[0]) % P, (a[1] - b[1]) % P), _f2m(a, b, Ri),
               _f2m(a, a, Ri)] + [(k * a[0] % P, k * a[1] % P) for k in (2, 3, 4, 8)]
        exp.append(sum((_w16(x) for x in res), []))
    names = ["add", "sub", "mul", "sqr", "mul_small2", "mul_small3", "mul_small4", "mul_small8"]
    return Case("fp2_all", inp, exp, [(nm, 16 * i, 16) for i, nm in enumerate(names)])


def case_fp2_mulsub():
    Ri = pow(MONT, -1, P)
    tup = pair_tuples("fp2_mulsub", fp2_edges(), 4, lambda r: (r.randrange(P), r.randrange(P)))
    inp, exp = [], []
    for a, b, c, d in tup:
        inp.append(_w16(a) + _w16(b) + _w16(c) + _w16(d))
        x, y = _f2m(a, b, Ri), _f2m(c, d, Ri)
        exp.append(_w16(((x[0] - y[0]) % P, (x[1] - y[1]) % P)))
    return Case("fp2_mulsub", inp, exp, [("mulsub", 0, 16)])


def case_fp2_inv():
    Rm = MONT % P
    Ri = pow(Rm, -1, P)
    tup = pair_tuples("fp2_inv", fp2_edges(), 1, lambda r: (r.randrange(P), r.randrange(P)))
    inp, exp = [], []
    for (a,) in tup:
        inp.append(_w16(a))
        if a == (0, 0):
            exp.append(_w16(a))
        else:
            i = o.fp2_inv((a[0] * Ri % P, a[1] * Ri % P))
            exp.append(_w16((i[0] * Rm % P, i[1] * Rm % P)))
    return Case("fp2_inv", inp, exp, [("inv", 0, 16)])


# ---- Field29 ---------------------------------------------------------------------------------------------------------
PINV261 = pow(P, -1, R261)
PINV0 = pow(P, -1, 1 << B29)
limbs, val = M.limbs, M.val
# value bounds (multiples of p) of normalized operands: the loop invariants the model proves, and the documented input
# bound of a product (the 13p x 13p that ff29_model.main() checks, and to_std's "any normalized value < 13p")
VALUE_BOUNDS = sorted(set(M.G1_INV.values()) | set(M.G2_INV.values()) | {1, 13})


def mont_exact(pairs):
    """(sum a*b) / 2^261 as the product-scanning reduction computes it: the unique r = (S + m p) / 2^261 with
    m = -S / p mod 2^261.  -> 9 limbs, limbs 0..7 masked, the top limb whatever is left"""
    S = sum(val(a) * val(b) for a, b in pairs)
    r = (S + ((-S * PINV261) % R261) * P) >> (B29 * L29)
    out = limbs(r)
    assert out[-1] < (1 << 32)
    return out


def _E(v):
    return M.E(v, v, val(v))     # an element whose bounds are its own limbs and value


def _checked_dot(pairs, square=False):
    """expected limbs, after the model has checked every column and limb bound on these very operands"""
    got = M.sqr(_E(pairs[0][0])) if square else M.mont(*[(_E(a), _E(b)) for a, b in pairs])
    exp = mont_exact(pairs)
    assert got.v == exp
    return exp


@functools.lru_cache(None)
def lazy_pool():
    """normalized operands at the proven bounds: limbs 0..7 at the limb bound (2^29 - 1), at bound - 1, alternating
    bound / 0 (both phases), zero; the top limb as large as the value bound k*p allows, and one below"""
    pool = []
    for k in VALUE_BOUNDS:
        vb = k * P - (1 if k in (1, 13) else 0)      # canonical values and product inputs are < k p, invariants <= k p
        for low in ([MASK] * 8, [MASK - 1] * 8, [MASK, 0] * 4, [0, MASK] * 4, [0] * 8):
            lowv = val(low + [0])
            top = (vb - lowv) >> M.TOPSH
            for t in (top, top - 1):
                if t >= 0:
                    v = low + [t]
                    assert val(v) <= vb
                    pool.append(tuple(v))
        pool.append(tuple(limbs(vb)))
    return tuple(dict.fromkeys(pool))


def _rand_norm(rng):
    return tuple(limbs(rng.randrange(rng.choice(VALUE_BOUNDS) * P)))


def column_limit_tuples(npairs, square=False):
    """limb patterns that bring a column sum as close to 2^64 as dot<NP>'s stated inequality
    9*(sum la*lb + 2^58) < 2^64 allows: uniform limbs la, lb with NP*la*lb at the largest admissible value"""
    room = ((1 << 64) - 1) // 9 - (1 << 58)          # sum la*lb <= room
    per = room // npairs
    out = []
    las = [math.isqrt(per)] if square else [(1 << 32) - 1, (1 << 31) + 12345, 1 << 30, math.isqrt(per), MASK]
    for la in las:
        lb = la if square else min(per // la, (1 << 32) - 1)
        assert 9 * (npairs * la * lb + (1 << 58)) < (1 << 64)
        a = tuple([la] * 8 + [min(la, MASK)])
        b = tuple([lb] * 8 + [min(lb, MASK)])
        out.append([a, b])
        if not square:
            out.append([b, a])
            out.append([tuple([la, 0] * 4 + [min(la, MASK)]), b])
    return out


def f29_tuples(name, arity, square=False, npairs=None):
    npairs = npairs or max(1, arity // 2)
    canon = tuple(tuple(limbs(x)) for x in edge_set(P))
    pool = lazy_pool()
    rng = _rng(name)
    out = []
    for i, a in enumerate(canon):
        for j, b in enumerate(canon):
            out.append([a, b] + [pool[(i * (3 + 2 * k) + j * (5 + 2 * k) + k) % len(pool)] for k in range(arity - 2)])
    if arity == 1:
        out = [[a] for a in canon]
    for i, a in enumerate(pool):                      # the bound operands against each other
        for s in (0, 1, 7):
            out.append([pool[(i + s * (k + 1)) % len(pool)] if k else a for k in range(arity)])
    out += [t[:1] if arity == 1 else t * (arity // 2) for t in column_limit_tuples(npairs, square)]
    out += [[_rand_norm(rng) for _ in range(arity)] for _ in range(NRANDOM)]
    if len(out) % 64 == 0:
        out.append([_rand_norm(rng) for _ in range(arity)])
    return out


def _post_product(pairs_of):
    """the post-condition dot<NP> states: normalized, the residue, and value < (sum a b) / 2^261 + p"""
    def post(row_in, row_out, nout=1):
        ins = [tuple(int(x) for x in row_in[9 * i:9 * i + 9]) for i in range(len(row_in) // 9)]
        for k, pairs in enumerate(pairs_of(ins)):
            r = [int(x) for x in row_out[9 * k:9 * k + 9]]
            S = sum(val(a) * val(b) for a, b in pairs)
            assert all(x <= MASK for x in r[:8]), "limbs 0..7 not normalized"
            assert val(r) % P == S * M.RINV % P, "wrong residue"
            assert val(r) < S // R261 + P + 1, "value above sum/2^261 + p"
    return post


def case_f29_dot(name, arity, pairs_of, square=False, npairs=None):
    tup = f29_tuples(name, arity, square, npairs)
    inp = [sum((list(x) for x in t), []) for t in tup]
    exp = [sum((_checked_dot(pairs, square) for pairs in pairs_of(t)), []) for t in tup]
    nout = len(exp[0]) // 9
    return Case(name, inp, exp, [("r%d" % i, 9 * i, 9) for i in range(nout)], post=_post_product(pairs_of))


def _pair_split(np_):
    def f(t):
        return [[(t[2 * i], t[2 * i + 1]) for i in range(np_)], [(t[2 * np_ + 2 * i], t[2 * np_ + 2 * i + 1]) for i in range(np_)]]
    return f


LIN_SEL = {0: ("add", None), 1: ("norm", None), 2: ("subk", (16, 1)), 3: ("subk", (4, 1)), 4: ("subk", (32, 1)),
           5: ("subk", (8, 1)), 6: ("subk2", (8, 3)), 7: ("negk", (2, 1)), 8: ("negk", (4, 1)), 9: ("negk", (8, 1)),
           10: ("negk", (16, 1)), 11: ("negk", (32, 1))}
U32 = (1 << 32) - 1


def case_f29_lin():
    rng = _rng("f29_lin")
    tup = []
    zero = [0] * 9
    alt = lambda v: [x if i % 2 == 0 else 0 for i, x in enumerate(v)]      # noqa: E731
    for sel, (kind, K) in LIN_SEL.items():
        nrand = NRANDOM // len(LIN_SEL) + 1
        if kind == "add":
            a = [U32 - 5] * 9
            sets = [(a, [5] * 9, zero), (zero, zero, zero), ([MASK] * 9, [MASK] * 9, zero), (alt(a), alt([5] * 9), zero)]
            for _ in range(nrand):
                x = [rng.randrange(1 << 32) for _ in range(9)]
                sets.append((x, [rng.randrange(U32 - v + 1) for v in x], zero))
        elif kind == "norm":
            # every carry is < 2^3 when the limbs are < 2^32 - 8: no 32-bit overflow
            a = [U32 - 8] * 8 + [U32 - 7]
            sets = [(a, zero, zero), (zero, zero, zero), ([MASK] * 9, zero, zero), ([MASK + 1] * 9, zero, zero),
                    ([MASK] + [MASK - 1] * 8, zero, zero), (alt(a), zero, zero)]
            sets += [([rng.randrange(U32 - 8) for _ in range(9)], zero, zero) for _ in range(nrand)]
        else:
            k = M.kform(*K)       # the limb bounds of the subtrahend, from the model
            room = [U32 - x for x in k]
            sets = []
            subs = [k, [max(x - 1, 0) for x in k], alt(k), zero, [min(x, MASK) for x in k]]
            subs += [[rng.randrange(x + 1) for x in k] for _ in range(nrand // 3 + 1)]
            for b in subs:
                for a in (zero, room, alt(room)):
                    if kind == "subk2":
                        c = [x // 2 for x in b]
                        sets.append((a, [x - 2 * y for x, y in zip(b, c)], c))
                        sets.append((a, b, zero))
                    else:
                        sets.append((a, b, zero))
        for a, b, c in sets:
            tup.append((sel, list(a), list(b), list(c)))
    if len(tup) % 64 == 0:
        tup.append((0, zero, zero, zero))
    inp, exp = [], []
    for sel, a, b, c in tup:
        kind, K = LIN_SEL[sel]
        inp.append([sel] + a + b + c)
        if kind == "add":
            r = [x + y for x, y in zip(a, b)]
        elif kind == "norm":
            r, cy = [], 0
            for i in range(8):
                t = a[i] + cy
                r.append(t & MASK)
                cy = t >> B29
            r.append(a[8] + cy)
            assert val(r) == val(a)
        else:
            k = M.kform(*K)
            r = [kk - y - 2 * z + (x if kind != "negk" else 0) for x, kk, y, z in zip(a, k, b, c)]
            want = (val(a) if kind != "negk" else 0) + K[0] * P - val(b) - 2 * val(c)
            assert val(r) == want
        assert all(0 <= x <= U32 for x in r), (sel, r)
        exp.append(r)
    return Case("f29_lin", inp, exp, [("result (sel: %s)" % ", ".join("%d %s%s" % (s, k, K or "") for s, (k, K) in LIN_SEL.items()), 0, 9)])


def case_f29_canon():
    rng = _rng("f29_canon")
    tup = []
    for mm in (1, 4, 16):
        vals = []
        for j in range(2 * mm):                                   # exact multiples of p and their neighbours
            vals += [j * P, j * P + 1] + ([j * P - 1] if j else [])
        vals.append(2 * mm * P - 1)
        vals += [x for x in edge_set(P)]
        for _ in range(64):                                       # maybe_zero false positives: low limb of j*p, not j*p
            j = rng.randrange(32)
            v = (rng.randrange(2 * mm * P) >> B29 << B29) | ((j * P) & MASK)
            if v < 2 * mm * P:
                vals.append(v)
        vals += [rng.randrange(2 * mm * P) for _ in range(NRANDOM // 3 + 1)]
        tup += [(mm, v) for v in vals]
    if len(tup) % 64 == 0:
        tup.append((1, 5))
    inp = [[mm] + limbs(v) for mm, v in tup]
    exp = [limbs(v % P) + [(1 if ((v & MASK) * PINV0 & MASK) < 32 else 0) | (2 if v % P == 0 else 0)] for mm, v in tup]
    fp = sum(1 for e, (mm, v) in zip(exp, tup) if e[9] == 1)
    assert fp >= 64, "false-positive vectors missing"
    return Case("f29_canon", inp, exp, [("canon", 0, 9), ("maybe_zero | is_zero_exact << 1", 9, 1)])


def case_f29_convert(name):
    rng = _rng(name)
    i32 = pow(32, -1, P)
    if name == "f29_relimb_in":
        xs = list(edge_set(P)) + [(1 << 256) - 1, P, 1 << 255] + [rng.randrange(1 << 256) for _ in range(NRANDOM)]
        return Case(name, [w8(x) for x in xs], [limbs(x) for x in xs], [("relimb", 0, 9)])
    if name == "f29_relimb_out":
        xs = list(edge_set(P)) + [rng.randrange(P) for _ in range(NRANDOM)]
        return Case(name, [limbs(x) for x in xs], [w8(x) for x in xs], [("relimb", 0, 8)])
    if name == "f29_from_std":      # x 2^256 -> x 2^261, canonical
        xs = list(edge_set(P)) + [rng.randrange(P) for _ in range(NRANDOM)]
        return Case(name, [w8(x) for x in xs], [limbs(x * 32 % P) for x in xs], [("from_std", 0, 9)])
    xs = [val(v) for v in lazy_pool() if val(v) < 13 * P] + list(edge_set(P)) + [rng.randrange(13 * P) for _ in range(NRANDOM)]
    return Case(name, [limbs(x) for x in xs], [w8(x * i32 % P) for x in xs], [("to_std", 0, 8)])


# ---- curves ----------------------------------------------------------------------------------------------------------
def _fp2_sqrt(a):
    """square root in Fp2 = Fp[u]/(u^2+1) (p = 3 mod 4), or None"""
    p = P
    if a == (0, 0):
        return (0, 0)
    norm = (a[0] * a[0] + a[1] * a[1]) % p
    s = pow(norm, (p + 1) // 4, p)
    if s * s % p != norm:
        return None
    for sgn in (s, p - s):
        t = (a[0] + sgn) * pow(2, -1, p) % p
        x0 = pow(t, (p + 1) // 4, p)
        if x0 * x0 % p == t and x0:
            x1 = a[1] * pow(2 * x0, -1, p) % p
            if o.fp2_sqr((x0, x1)) == (a[0] % p, a[1] % p):
                return (x0, x1)
    return None


@functools.lru_cache(None)
def edge_points(group):
    """points with a coordinate from the edge set, where the curve has one (G2: on the twist, any subgroup)"""
    pts = []
    if group == 1:
        for x in edge_set(P) + tuple(range(3, 12)):
            rhs = (x * x * x + 3) % P
            y = pow(rhs, (P + 1) // 4, P)
            if y * y % P == rhs and (x, y) != (0, 0):
                pts.append((x, y))
        assert (1, 2) in pts
    else:
        e = edge_set(P)
        for x in [(a, 0) for a in e[:24]] + [(0, a) for a in e[1:12]] + [(a, a) for a in e[1:12]] + [(3 + i, 1) for i in range(6)]:
            y = _fp2_sqrt(o.fp2_add(o.fp2_mul(o.fp2_sqr(x), x), o.TWIST_B))
            if y is not None and (x, y) != o.INF_G2:
                pts.append((x, y))
    assert len(pts) >= 8
    return tuple(pts)


def _curve(group):
    return (o.G1, o.GEN1, o.g1_to_bytes, o.g1_from_bytes, 16) if group == 1 else (o.G2, o.GEN2, o.g2_to_bytes, o.g2_from_bytes, 32)


def _pw(enc, pt):
    return list(np.frombuffer(enc(pt), dtype=np.uint32))


@functools.lru_cache(None)
def point_lists(group, nrand):
    """the curve sequences (<= 8 points each) and their sums"""
    C, gen, enc, dec, pw = _curve(group)
    rng = _rng("points%d" % group)
    P1, P2, P3 = (C.mul(rng.randrange(1, R), gen) for _ in range(3))
    S12 = C.add(P1, P2)
    ep = list(edge_points(group))
    lists = [[P1, P2, P3], [P1, P1], [P1, C.neg(P1)], [C.inf, P1, C.inf, P2], [P1, P1, P1, C.neg(P1), P2], [C.inf], [],
             [P1, P2, C.neg(P2), C.neg(P1)], [P1] * 5, [P1] * 8, [P1, P2, S12], [P1, P2, C.neg(S12)], [P1, P2, C.neg(S12), P3],
             [P1, P2, S12, P3], [P1, C.inf], [C.inf, C.inf, P1], [P1, P2, P3, C.inf], [P1, C.neg(P1), P2, C.neg(P2), P3, P3]]
    for i, e in enumerate(ep):
        lists += [[e], [e, e], [e, C.neg(e)], [P1, e, ep[(i + 1) % len(ep)]], [e, P1, C.neg(e)]]
    pool = [C.mul(rng.randrange(1, R), gen) for _ in range(24)] + ep
    pool += [C.neg(q) for q in pool[:12]] + [C.inf, C.inf]
    for _ in range(nrand):
        lists.append([rng.choice(pool) for _ in range(rng.randrange(1, 9))])
    out = []
    for pts in lists:
        s = C.inf
        for q in pts:
            s = C.add(s, q)
        out.append((tuple(pts), s))
    return tuple(out)


def _seq_case(name, group, modes, cap, lists):
    C, gen, enc, dec, pw = _curve(group)
    inp, exp = [], []
    infw = [0] * pw
    for pts, s in lists:
        body = sum((_pw(enc, q) for q in pts), []) + infw * (cap - len(pts))
        for mode in modes:
            inp.append([len(pts), mode, 0, 0] + body)
            exp.append(_pw(enc, s))
    return inp, exp


def case_ec_seq(group):
    C, gen, enc, dec, pw = _curve(group)
    name = "g%d_seq" % group
    lists = point_lists(group, NRANDOM // 3 + 1)
    inp, exp = _seq_case(name, group, (0, 1, 5), 8, lists)
    rng = _rng(name)
    singles = [l[0][0] for l in lists if len(l[0]) >= 1 and l[0][0] != C.inf][:40] + list(edge_points(group))
    infw = [0] * pw
    for q in singles:
        for k in (0, 1, 2, 3, 12345, rng.randrange(1 << 16)):                      # mul_small
            inp.append([k, 2, 0, 0] + _pw(enc, q) + infw * 7)
            exp.append(_pw(enc, C.mul(k, q)))
        for n in (0, 1, 3, 8):                                                      # n doublings
            inp.append([n, 3, 0, 0] + _pw(enc, q) + infw * 7)
            exp.append(_pw(enc, C.mul(1 << n, q)))
        inp.append([1, 4, 0, 0] + _pw(enc, q) + infw * 7)                           # dbl_affine
        exp.append(_pw(enc, C.add(q, q)))
    for mode, k in ((2, 7), (3, 4)):                                                # infinity in
        inp.append([k, mode, 0, 0] + infw * 8)
        exp.append(infw)
    if len(inp) % 64 == 0:
        inp.append(inp[0]), exp.append(exp[0])
    return Case(name, inp, exp, [("affine sum (mode 0 madd, 1 add, 2 mul_small, 3 dbl, 4 dbl_affine, 5 neg)", 0, pw)])


def case_ec29_seq(group):
    name = "g%d_seq29" % group
    inp, exp = _seq_case(name, group, (0, 1, 2, 3, 4), 8, point_lists(group, NRANDOM // 5 + 1))
    if len(inp) % 64 == 0:
        inp.append(inp[0]), exp.append(exp[0])
    pw = 16 * group
    return Case(name, inp, exp, [("affine sum (mode 0 madd, 1 madd sign flag, 2 add tree, 3 via to_std/acc_from_std, 4 repacked)", 0, pw)])


def case_ec29_chain(group):
    """400-term chains: accumulators that stay lazy for hundreds of additions"""
    C, gen, enc, dec, pw = _curve(group)
    rng = _rng("chain%d" % group)
    pool = [C.mul(rng.randrange(1, R), gen) for _ in range(12)]
    ep = list(edge_points(group))
    lists = [[rng.choice(pool + [C.inf]) if rng.random() < 0.8 else C.neg(rng.choice(pool)) for _ in range(400)],
             [pool[0]] * 400,
             [pool[i % 2] if i % 4 < 2 else C.neg(pool[i % 2]) for i in range(400)],
             [rng.choice(ep + pool) for _ in range(399)]]
    sums = []
    for pts in lists:
        s = C.inf
        for q in pts:
            s = C.add(s, q)
        sums.append((tuple(pts), s))
    inp, exp = _seq_case("chain", group, (0, 1, 2, 3, 4), 400, sums)
    return Case("g%d_chain29" % group, inp, exp, [("affine sum (modes as g%d_seq29)" % group, 0, pw)])


def case_tab29(group):
    C, gen, enc, dec, pw = _curve(group)
    rng = _rng("tab%d" % group)
    pts = [C.inf] + list(edge_points(group)) + [C.mul(rng.randrange(1, R), gen) for _ in range(40)]
    pts += [rng.choice(pts) for _ in range(64 - len(pts) % 64 + 1)] if len(pts) % 64 == 0 else []
    inp, exp = [], []
    for q in pts:
        inp.append(_pw(enc, q))
        cs = [q[0], q[1]] if group == 1 else [q[0][0], q[0][1], q[1][0], q[1][1]]
        # the bytes hold c * 2^256 mod p; the entry holds c * 2^261 mod p as a plain 256-bit word
        t = sum((w8(c * R261 % P) for c in cs), [])
        exp.append(t + t)
    return Case("g%d_tab29" % group, inp, exp, [("tab_from_std", 0, pw), ("pack(unpack)", pw, pw)])


# ---- the Fp12 tower, the Miller loop and the final exponentiation (pairing.cuh) --------------------------------------
# An element is a tuple of six Fp2 values g[k] = (a, b) over w^k, as plain residues (not Montgomery); the references
# work in the oracle's 12-coefficient polynomial basis Fp[w]/(w^12 - 18 w^6 + 82), where u = w^6 - 9.  The oracle's
# _f12_mul costs about 50 us, so a power with a 3000-bit exponent (the inverse, the final exponentiation) costs 0.2 s
# for a dense element and a fraction of that for a sparse one: the operand counts below are sized by that.
RM_P = MONT % P
RI_P = pow(RM_P, -1, P)
F2Z = (0, 0)
F12_ONE = ((1, 0),) + (F2Z,) * 5
BN_X = 4965661367192848881
assert 6 * BN_X * BN_X == o.ATE_LOOP


def f12_to_poly(g):
    """six Fp2 values over w^k -> the oracle's 12 coefficients: (a + b u) w^k = (a - 9 b) w^k + b w^(k+6)"""
    out = [0] * 12
    for k, c in enumerate(g):
        out = [(x + y) % P for x, y in zip(out, o._emb(c, k))]
    return out


def f12_from_poly(c):
    """the inverse of f12_to_poly"""
    return tuple(((c[k] + 9 * c[k + 6]) % P, c[k + 6] % P) for k in range(6))


def f12_from_bytes(raw):
    """384-byte flat Fp12 (6 x Fp2 over w^k, Montgomery), the layout g16_pairing returns -> six Fp2 values"""
    return tuple((o.fp_from_mont_bytes(raw[64 * k:64 * k + 32]), o.fp_from_mont_bytes(raw[64 * k + 32:64 * k + 64]))
                 for k in range(6))


def gt_from_bytes(raw):
    """384-byte flat Fp12 -> the oracle's degree-12 polynomial basis"""
    return f12_to_poly(f12_from_bytes(raw))


def _fpw(x):
    return w8(x * RM_P % P)


def _f12w(g):
    return sum((_fpw(c[0]) + _fpw(c[1]) for c in g), [])


def _polyw(c):
    return _f12w(f12_from_poly(c))


def _stored(x):
    """the residue whose Montgomery word is x: edge patterns of the stored limbs, not of the value"""
    return x * RI_P % P


@functools.lru_cache(None)
def _f12_pool_named():
    rng = _rng("f12_pool")
    r2 = lambda: (rng.randrange(P), rng.randrange(P))      # noqa: E731

    def basis(k, c):
        return tuple(c if i == k else F2Z for i in range(6))
    pool = [(F2Z,) * 6, F12_ONE]
    for k in range(6):                                      # one basis element w^k
        pool += [basis(k, c) for c in ((1, 0), (P - 1, 0), (0, 1), (P - 1, P - 1), (1, P - 1))]
    pool.append(((P - 1, P - 1),) * 6)                      # all twelve coordinates p - 1 ...
    pool.append(((_stored(P - 1),) * 2,) * 6)               # ... and all twelve stored words p - 1, and 1
    pool.append(((_stored(1),) * 2,) * 6)
    named = {"stored1": pool[-1]}
    pool.append(basis(0, (rng.randrange(2, P), 0)))         # in Fp, in Fp2
    named["fp"] = pool[-1]
    pool.append(basis(0, r2()))
    pool.append((r2(), F2Z, r2(), F2Z, r2(), F2Z))          # in Fp6: the B = 0 side of inv
    named["fp6"] = pool[-1]
    pool.append((F2Z, r2(), F2Z, r2(), F2Z, r2()))          # pure w: the A = 0 side of inv
    # g[0..2] = 0: among themselves every product term has i + j >= 6, so mul_xi carries the whole result
    pool.append((F2Z, F2Z, F2Z, r2(), r2(), r2()))
    pool.append((F2Z, F2Z, F2Z) + ((P - 1, P - 1),) * 3)
    for _ in range(2):                                      # the cyclotomic subgroup: outputs of the easy part
        x = [rng.randrange(P) for _ in range(12)]
        pool.append(f12_from_poly(o._f12_pow(x, (P ** 6 - 1) * (P ** 2 + 1))))
    named["cyclotomic"] = pool[-1]
    pool += [tuple(r2() for _ in range(6)) for _ in range(3)]
    return tuple(dict.fromkeys(pool)), named


def f12_pool():
    return _f12_pool_named()[0]


def _f12_rand(rng):
    return tuple((rng.randrange(P), rng.randrange(P)) for _ in range(6))


@functools.lru_cache(None)
def _pow_ref(g, e):
    return tuple(o._f12_pow(f12_to_poly(g), e))


def case_f12_mul():
    tup = pair_tuples("f12_mul", f12_pool(), 2, _f12_rand, nrandom=64)
    inp, exp = [], []
    for a, b in tup:
        r = _polyw(o._f12_mul(f12_to_poly(a), f12_to_poly(b)))
        inp.append(_f12w(a) + _f12w(b))
        exp.append(r + r)
    return Case("f12_mul", inp, exp, [("mul(a,b)", 0, 96), ("mul(b,a)", 96, 96)])


def case_f12_sqr():
    tup = pair_tuples("f12_sqr", f12_pool(), 1, _f12_rand, nrandom=64)
    inp, exp = [], []
    for (a,) in tup:
        pa = f12_to_poly(a)
        r = _polyw(o._f12_mul(pa, pa))
        inp.append(_f12w(a))
        exp.append(r + r)
    return Case("f12_sqr", inp, exp, [("sqr(a)", 0, 96), ("mul(a,a)", 96, 96)])


def case_f12_mul_line():
    rng = _rng("f12_mul_line")
    r2 = lambda: (rng.randrange(P), rng.randrange(P))      # noqa: E731
    base = (rng.randrange(P), r2(), r2())
    lines = [base, (0, F2Z, F2Z), (1, (1, 0), (1, 0)), (P - 1, (P - 1, P - 1), (P - 1, P - 1))]
    for x in (0, 1, P - 1, _stored(1), _stored(P - 1)):     # each coefficient at its edges in turn
        lines.append((x, base[1], base[2]))
    for c in (F2Z, (1, 0), (0, 1), (P - 1, 0), (P - 1, P - 1), (_stored(P - 1), _stored(1))):
        lines += [(base[0], c, base[2]), (base[0], base[1], c), (0, c, F2Z), (0, F2Z, c)]
    tup = [(f, l) for f in f12_pool() for l in lines]
    tup += [(_f12_rand(rng), (rng.randrange(P), r2(), r2())) for _ in range(64)]
    inp, exp = [], []
    for f, (l0, l1, l3) in tup:
        line = [(x + y + z) % P for x, y, z in zip([l0] + [0] * 11, o._emb(l1, 1), o._emb(l3, 3))]
        inp.append(_f12w(f) + _fpw(l0) + _fpw(l1[0]) + _fpw(l1[1]) + _fpw(l3[0]) + _fpw(l3[1]))
        exp.append(_polyw(o._f12_mul(line, f12_to_poly(f))))
    if len(inp) % 64 == 0:
        inp.append(inp[0]), exp.append(exp[0])
    return Case("f12_mul_line", inp, exp, [("mul_line", 0, 96)])


def case_f12_frob():
    tup = pair_tuples("f12_frob", f12_pool(), 1, _f12_rand, nrandom=2)
    inp = [_f12w(a) for (a,) in tup]
    exp = [sum((_polyw(_pow_ref(a, P ** n)) for n in (6, 1, 2, 3)), []) for (a,) in tup]
    return Case("f12_frob", inp, exp, [("conj", 0, 96)] + [("frobenius(a,%d)" % n, 96 * n, 96) for n in (1, 2, 3)])


def _f6_embed(c):
    """Fp6 = Fp2[v]/(v^3 - xi) into Fp12 through v = w^2"""
    return (c[0], F2Z, c[1], F2Z, c[2], F2Z)


def _f6_back(g):
    assert g[1] == g[3] == g[5] == F2Z
    return (g[0], g[2], g[4])


def _f6w(c):
    return sum((_fpw(x[0]) + _fpw(x[1]) for x in c), [])


@functools.lru_cache(None)
def f6_pool():
    rng = _rng("f6_pool")
    r2 = lambda: (rng.randrange(P), rng.randrange(P))      # noqa: E731
    pool = [(F2Z,) * 3, ((1, 0), F2Z, F2Z)]
    for k in range(3):
        pool += [tuple(c if i == k else F2Z for i in range(3)) for c in ((1, 0), (P - 1, 0), (0, 1), (P - 1, P - 1), (1, P - 1))]
    pool += [((P - 1, P - 1),) * 3, ((_stored(P - 1),) * 2,) * 3, ((rng.randrange(1, P), 0), F2Z, F2Z), (r2(), F2Z, F2Z)]
    pool += [(F2Z, r2(), r2()), (r2(), F2Z, r2()), (r2(), r2(), F2Z)]
    pool += [(r2(), r2(), r2()) for _ in range(4)]
    return tuple(dict.fromkeys(pool))


def case_f6_mul():
    tup = pair_tuples("f6_mul", f6_pool(), 2, lambda r: tuple((r.randrange(P), r.randrange(P)) for _ in range(3)), nrandom=64)
    inp, exp = [], []
    for a, b in tup:
        inp.append(_f6w(a) + _f6w(b))
        exp.append(_f6w(_f6_back(f12_from_poly(o._f12_mul(f12_to_poly(_f6_embed(a)), f12_to_poly(_f6_embed(b)))))))
    return Case("f6_mul", inp, exp, [("f6mul", 0, 48)])


def _post_inverse(words, embed):
    """a * inv(a) = 1, on the words the op returned"""
    def post(row_in, row_out):
        def elem(row):
            c = [from_w8(row[8 * i:8 * i + 8]) * RI_P % P for i in range(words // 8)]
            return embed(tuple((c[2 * i], c[2 * i + 1]) for i in range(words // 16)))
        assert o._f12_mul(f12_to_poly(elem(row_in[:words])), f12_to_poly(elem(row_out[:words]))) == o._f12_one(), \
            "a * inv(a) is not 1"
    return post


def case_f6_inv():
    """nonzero operands only: f6inv hands its norm to Fp2::inv"""
    rng = _rng("f6_inv")
    xs = [c for c in f6_pool() if c != (F2Z,) * 3] + [tuple((rng.randrange(P), rng.randrange(P)) for _ in range(3)) for _ in range(4)]
    inp = [_f6w(c) for c in xs]
    exp = [_f6w(_f6_back(f12_from_poly(_pow_ref(_f6_embed(c), P ** 12 - 2)))) for c in xs]
    return Case("f6_inv", inp, exp, [("f6inv", 0, 48)], post=_post_inverse(48, _f6_embed))


def case_f12_inv():
    """nonzero operands only: inv reaches Fp2::inv through f6inv"""
    rng = _rng("f12_inv")
    xs = [g for g in f12_pool() if g != (F2Z,) * 6] + [_f12_rand(rng) for _ in range(2)]
    inp = [_f12w(g) for g in xs]
    exp = [_polyw(_pow_ref(g, P ** 12 - 2)) for g in xs]
    return Case("f12_inv", inp, exp, [("inv", 0, 96)], post=_post_inverse(96, lambda g: g))


POW_EXPONENTS = (0, 1, 2, 1 << 63, (1 << 64) - 1, BN_X)


def case_f12_pow_u64():
    rng = _rng("f12_pow_u64")
    tup = [(g, e) for g in f12_pool() for e in POW_EXPONENTS]
    tup += [(_f12_rand(rng), rng.randrange(1 << 64)) for _ in range(9)]
    inp = [_f12w(g) + [e & 0xffffffff, e >> 32] for g, e in tup]
    exp = [_polyw(_pow_ref(g, e)) for g, e in tup]
    return Case("f12_pow_u64", inp, exp, [("pow_u64", 0, 96)])


def case_f12_small_pows():
    tup = pair_tuples("f12_small_pows", f12_pool(), 1, _f12_rand, nrandom=32)
    inp = [_f12w(a) for (a,) in tup]
    exp = [sum((_polyw(_pow_ref(a, e)) for e in (6, 12, 18, 30, 36)), []) for (a,) in tup]
    return Case("f12_small_pows", inp, exp, [("p%d" % e, 96 * i, 96) for i, e in enumerate((6, 12, 18, 30, 36))])


def case_f12_is_one():
    """the pool, and one with a single bit of a single stored word flipped, in each of the twelve coordinates"""
    rng = _rng("f12_is_one")
    one_w = _f12w(F12_ONE)
    inp = [_f12w(g) for g in f12_pool()]
    for coord in range(12):
        for bit in (0, 31, 32 * rng.randrange(1, 7) + rng.randrange(32), 224, 252):
            row = list(one_w)
            row[8 * coord + bit // 32] ^= 1 << (bit % 32)
            if from_w8(row[8 * coord:8 * coord + 8]) < P:      # canonical operands only
                inp.append(row)
    inp += [one_w, _f12w(((P - 1, 0),) + (F2Z,) * 5), _f12w(((_stored(1), 0),) + (F2Z,) * 5)]
    exp = [[1 if row == one_w else 0] for row in inp]
    assert sum(e[0] for e in exp) == 2 and len(inp) % 64 != 0
    return Case("f12_is_one", inp, exp, [("is_one", 0, 1)])


def twist_walk(x=(3, 1)):
    """points of the twist outside the order-r subgroup, walking x upwards (as the verifier's subgroup test does)"""
    while True:
        y = _fp2_sqrt(o.fp2_add(o.fp2_mul(o.fp2_sqr(x), x), o.TWIST_B))
        if y is not None and not o.G2.is_inf(o.G2.mul(R, (x, y))):
            yield (x, y)
        x = (x[0] + 1, x[1])


G2_COFACTOR = 2 * P - R           # #E'(Fp2) = r (2p - r)
SMALL_ORDER = 10069               # 2p - r = 10069 * (a 241-bit number)
assert G2_COFACTOR % SMALL_ORDER == 0


@functools.lru_cache(None)
def twist_points():
    """(a twist point of order 10069, the first twist point outside the order-r subgroup)"""
    full = None
    for T in twist_walk():
        full = full or T
        Q = o.G2.mul(R * (G2_COFACTOR // SMALL_ORDER), T)
        if not o.G2.is_inf(Q):
            assert o.G2.is_on_curve(Q) and o.G2.is_inf(o.G2.mul(SMALL_ORDER, Q))
            return Q, full


@functools.lru_cache(None)
def miller_ref(Pt, Q):
    return tuple(o.miller_loop(Pt, Q))


@functools.lru_cache(None)
def miller_pairs():
    """(P, Q) operands of the Miller loop.  The oracle's loop is the reference for every one of them: it asserts
    T = -Q wherever it meets T.x = Q.x, and that assertion holds on all of these (no case had to be left out; the
    multiples 6x^2 visits of the order-10069 point never meet +-Q or infinity modulo 10069)."""
    rng = _rng("pair_miller")
    P1, P2, P3 = (o.G1.mul(rng.randrange(1, R), o.GEN1) for _ in range(3))
    Q1, Q2, Q3 = (o.G2.mul(rng.randrange(1, R), o.GEN2) for _ in range(3))
    small, full = twist_points()
    pairs = [(o.INF_G1, Q1), (P1, o.INF_G2), (o.INF_G1, o.INF_G2), (o.GEN1, o.GEN2), (P1, Q1), (o.G1.neg(P1), Q1),
             (P1, o.G2.neg(Q1)), (P2, Q2), (P3, Q3), (o.GEN1, Q2), (P2, o.GEN2),
             (P1, small), (o.GEN1, small), (P2, o.G2.neg(small)), (P1, full), (o.GEN1, full), (o.INF_G1, small)]
    e1, e2 = edge_points(1), edge_points(2)
    pairs += [(e, (Q1, o.GEN2)[i % 2]) for i, e in enumerate(e1[::max(1, len(e1) // 10)][:10])]
    pairs += [((P1, o.GEN1)[i % 2], e) for i, e in enumerate(e2[::max(1, len(e2) // 10)][:10])]
    pairs += [(e1[-1], e2[-1]), (e1[0], e2[0])]
    pairs = list(dict.fromkeys(pairs))
    assert len(pairs) <= 40 and len(pairs) % 64 != 0
    return tuple(pairs)


def case_pair_miller():
    inp = [_pw(o.g1_to_bytes, Pt) + _pw(o.g2_to_bytes, Q) for Pt, Q in miller_pairs()]
    exp = [_polyw(miller_ref(Pt, Q)) for Pt, Q in miller_pairs()]
    return Case("pair_miller", inp, exp, [("miller", 0, 96)])


def case_pair_final_exp():
    """nonzero operands only (final_exp inverts its operand)"""
    rng = _rng("pair_final_exp")
    named = _f12_pool_named()[1]
    mp = miller_pairs()
    # the generators, random pairs, -P and -Q, the order-10069 and the cofactor point, three edge points
    fs = [f12_from_poly(miller_ref(*mp[i])) for i in (3, 4, 5, 6, 7, 9, 11, 12, 14, -1, -2, -3)]
    subfield = [F12_ONE, named["fp"], named["fp6"]]         # 1, an element of Fp*, one of Fp6*: all give 1
    fs += subfield + [named["cyclotomic"], named["stored1"]] + [_f12_rand(rng) for _ in range(3)]
    assert len(fs) <= 24 and (F2Z,) * 6 not in fs
    exp = [tuple(o.final_exp(f12_to_poly(f))) for f in fs]
    for f, e in zip(fs, exp):
        assert (e == tuple(o._f12_one())) == (f in subfield)
    return Case("pair_final_exp", [_f12w(f) for f in fs], [_polyw(e) for e in exp], [("final_exp", 0, 96)])



# ---- msm_digits (device only) ------------------------------------------------------------------------------------------
def class_weight(c, bucket):
    """weight of a bucket of the class set (msm.cuh), as restated in shim_class_buckets_check"""
    h = 1 << (c - 1)
    if bucket < h // 2:
        return 2 * bucket + 1
    if bucket < h // 2 + h // 8:
        return 4 * (2 * (bucket - h // 2) + 1)
    if bucket < h // 2 + h // 8 + h // 32:
        return 16 * (2 * (bucket - h // 2 - h // 8) + 1)
    return 64 * (bucket - h // 2 - h // 8 - h // 32 + 1)


def digit_configs():
    """(c, mtab): every window width 5..22 with one table; with two tables every width whose class set exists --
    at c = 5 magnitude 16 would need class 2, which has 2^(c-1)/32 = 0 buckets there (registered sets use c >= 15)"""
    return [(c, 1) for c in range(5, 23)] + [(c, 2) for c in range(6, 23)]


def digit_scalars(c, rng):
    nwin = 254 // c + 1
    h = 1 << (c - 1)
    allw = lambda d: sum(d << (c * w) for w in range(nwin))     # noqa: E731
    s = [0, 1, R - 1, h, h + 1, (1 << c) - 1, allw(h) % R, allw(h + 1) % R, allw((1 << c) - 1) % R, allw(h + 1) % (1 << 253),
         allw(h) % (1 << 253), (1 << 253), R - 2, (R - 1) // 2, 64, 1 << 6, (1 << c) - 64 if c > 6 else 3]
    return s + [rng.randrange(R) for _ in range(48)] + [rng.randrange(1 << rng.randrange(1, 254)) for _ in range(16)]


def case_msm_digits():
    rng = _rng("msm_digits")
    Rm = MONT % R
    inp, meta = [], []
    for c, mtab in digit_configs():
        for mont in (0, 1):
            for s in digit_scalars(c, rng):
                inp.append([c, mtab, mont, 0] + w8(s * Rm % R if mont else s))
                meta.append((c, mtab, mont, s))
    if len(inp) % 64 == 0:
        inp.append(inp[0]), meta.append(meta[0])
    return inp, meta


def check_msm_digits(label, inp, meta, got):
    """the emitted (window, bucket, sign) triples must reconstruct the scalar: sum +- weight * 2^(c w [+ sel])"""
    for i, (c, mtab, mont, s) in enumerate(meta):
        nwin = 254 // c + 1
        row = got[i]
        cnt = int(row[0])
        where = "%s msm_digits: tuple %d (c=%d mtab=%d mont=%d scalar=%#x) -> %s" % (
            label, i, c, mtab, mont, s, " ".join("%08x" % int(x) for x in row[:min(cnt, 63) + 1]))
        assert cnt <= nwin, where
        total, seen = 0, set()
        for e in row[1:1 + cnt]:
            e = int(e)
            neg, wv, bucket = e >> 31, (e >> 24) & 0x7f, e & 0xffffff
            sel, w = divmod(wv, nwin)
            assert sel < mtab and w not in seen, where
            seen.add(w)
            if mtab == 2:
                assert bucket < (1 << (c - 1)) // 2 + (1 << (c - 1)) // 8 + (1 << (c - 1)) // 32 + (1 << (c - 1)) // 64, where
                mag = class_weight(c, bucket) << sel
            else:
                assert bucket < (1 << (c - 1)), where
                mag = bucket + 1
            assert 1 <= mag <= (1 << (c - 1)), where
            total += (-mag if neg else mag) << (c * w)
        assert total == s, where + " reconstructs %#x" % total


# ---- the table ---------------------------------------------------------------------------------------------------------
BUILDERS = {
    "fp_all": lambda: case_field_all("fp"), "fr_all": lambda: case_field_all("fr"),
    "fp_dot2": lambda: case_field_dot2("fp"), "fr_dot2": lambda: case_field_dot2("fr"),
    "fp_dot4": lambda: case_field_dot4("fp"), "fr_dot4": lambda: case_field_dot4("fr"),
    "fp_cmp": lambda: case_field_cmp("fp"), "fr_cmp": lambda: case_field_cmp("fr"),
    "fp_inv": lambda: case_field_inv("fp", "_inv"), "fr_inv": lambda: case_field_inv("fr", "_inv"),
    "fp_inv_fermat": lambda: case_field_inv("fp", "_inv_fermat"), "fr_inv_fermat": lambda: case_field_inv("fr", "_inv_fermat"),
    "fp2_all": case_fp2_all, "fp2_mulsub": case_fp2_mulsub, "fp2_inv": case_fp2_inv,
    "f29_relimb_in": lambda: case_f29_convert("f29_relimb_in"), "f29_relimb_out": lambda: case_f29_convert("f29_relimb_out"),
    "f29_from_std": lambda: case_f29_convert("f29_from_std"), "f29_to_std": lambda: case_f29_convert("f29_to_std"),
    "f29_mul": lambda: case_f29_dot("f29_mul", 2, lambda t: [[(t[0], t[1])]]),
    "f29_sqr": lambda: case_f29_dot("f29_sqr", 1, lambda t: [[(t[0], t[0])]], square=True),
    "f29_dot2": lambda: case_f29_dot("f29_dot2", 4, lambda t: [[(t[0], t[1]), (t[2], t[3])]]),
    "f29_dot4": lambda: case_f29_dot("f29_dot4", 8, lambda t: [[(t[2 * i], t[2 * i + 1]) for i in range(4)]]),
    "f29_pair1": lambda: case_f29_dot("f29_pair1", 4, _pair_split(1), npairs=1),
    "f29_pair2": lambda: case_f29_dot("f29_pair2", 8, _pair_split(2), npairs=2),
    "f29_pair4": lambda: case_f29_dot("f29_pair4", 16, _pair_split(4), npairs=4),
    "f29_lin": case_f29_lin, "f29_canon": case_f29_canon,
    "g1_seq": lambda: case_ec_seq(1), "g2_seq": lambda: case_ec_seq(2),
    "g1_seq29": lambda: case_ec29_seq(1), "g2_seq29": lambda: case_ec29_seq(2),
    "g1_chain29": lambda: case_ec29_chain(1), "g2_chain29": lambda: case_ec29_chain(2),
    "g1_tab29": lambda: case_tab29(1), "g2_tab29": lambda: case_tab29(2),
    "f12_mul": case_f12_mul, "f12_sqr": case_f12_sqr, "f12_mul_line": case_f12_mul_line, "f12_frob": case_f12_frob,
    "f6_mul": case_f6_mul, "f6_inv": case_f6_inv, "f12_inv": case_f12_inv, "f12_pow_u64": case_f12_pow_u64,
    "f12_small_pows": case_f12_small_pows, "f12_is_one": case_f12_is_one, "pair_miller": case_pair_miller,
    "pair_final_exp": case_pair_final_exp,
}
HOST_OPS = tuple(BUILDERS)                    # every op of devops.inc that also compiles with g++
DEVICE_OPS = HOST_OPS + ("msm_digits",)       # the op groups of the GPU test
# the ops of pairing.cuh run in the builds whose configuration ships pairing.o: plain, and calls (make DEV=1); the
# reduced-radix macros of the other three do not reach pairing.cuh, and their builds leave these ops out
PAIRING_OPS = ("f12_mul", "f12_sqr", "f12_mul_line", "f12_frob", "f6_mul", "f6_inv", "f12_inv", "f12_pow_u64",
               "f12_small_pows", "f12_is_one", "pair_miller", "pair_final_exp")
PAIRING_VARIANTS = ("plain", "calls")


def variant_ops(variant):
    """the ops the build `variant` (a name of VARIANTS) carries"""
    return tuple(op for op in DEVICE_OPS if op not in PAIRING_OPS or variant in PAIRING_VARIANTS)


@functools.lru_cache(None)
def build_case(op):
    return BUILDERS[op]()


class OpLibrary:
    """a loaded build of the op table: run(op name, uint32 [n, in_words]) -> uint32 [n, out_words]"""

    def __init__(self, lib, runner):
        self.lib, self.runner, self.ops = lib, runner, {}
        nm, a, b = ctypes.c_char_p(), ctypes.c_uint32(), ctypes.c_uint32()
        for op in range(lib.devops_nops()):
            assert lib.devops_info(op, ctypes.byref(nm), ctypes.byref(a), ctypes.byref(b)) == 0
            self.ops[nm.value.decode()] = (op, a.value, b.value)

    def run(self, name, inp, variant=0):
        op, inw, outw = self.ops[name]
        inp = np.ascontiguousarray(inp, dtype=np.uint32)
        assert inp.ndim == 2 and inp.shape[1] == inw, (name, inp.shape, inw)
        out = np.zeros((inp.shape[0], outw), dtype=np.uint32)
        rc = self.runner(variant, op, inp.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(inp.shape[0]),
                         out.ctypes.data_as(ctypes.c_void_p))
        assert rc == 0, "%s: the library returned error %d" % (name, rc)
        return out


def _hex(row):
    return " ".join("%08x" % int(x) for x in row)


def check_op(oplib, op, label, variant=0):
    """runs one op over its full operand set; on a mismatch names the build, the op, the output slot, the first failing
    tuple and its operands in hex"""
    if op == "msm_digits":
        inp, meta = case_msm_digits()
        got = oplib.run(op, np.array(inp, dtype=np.uint64).astype(np.uint32), variant)
        check_msm_digits(label, inp, meta, got)
        return len(inp)
    case = build_case(op)
    got = oplib.run(op, case.inp, variant)
    bad = np.nonzero((got != case.exp).any(axis=1))[0]
    if len(bad):
        i = int(bad[0])
        slot = next((nm for nm, s, n in case.slots if (got[i, s:s + n] != case.exp[i, s:s + n]).any()), "?")
        s, n = next((s, n) for nm, s, n in case.slots if nm == slot)
        raise AssertionError("%s op %s, output %s: %d of %d tuples differ, first at index %d\n  operands: %s\n  got:      %s\n  expected: %s"
                             % (label, op, slot, len(bad), len(case.inp), i, _hex(case.inp[i]), _hex(got[i, s:s + n]),
                                _hex(case.exp[i, s:s + n])))
    if case.post is not None:
        for i in range(len(case.inp)):
            try:
                case.post(case.inp[i], got[i])
            except AssertionError as e:
                raise AssertionError("%s op %s: post-condition at index %d: %s\n  operands: %s\n  got: %s"
                                     % (label, op, i, e, _hex(case.inp[i]), _hex(got[i])))
    return len(case.inp)
