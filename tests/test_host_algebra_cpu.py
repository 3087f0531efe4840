"""The host side of a proof's last step on the CPU: the 4 x u64 host field (csrc/host_ff64.hpp: HFp, HFp2), the curve
templates of ec.cuh instantiated over it, host_add / host_mul / host_mul2 and the two combine halves
(csrc/host_curve.hpp), compiled with g++ (tests/cpu_kernels/hostalg_shim.cpp) and held to Python integers.  Points are
k * G with known logs (the C oracle's fixed-base multiplier), so every expected value is a closed form mod r
(tests/combine_pictures.py); nothing expected comes from the code under test."""
import ctypes
import glob
import os
import subprocess

import pytest

from oracle import bn254_ref as o
from tests import combine_pictures as cp

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpu_kernels")
P, R = o.P, o.R
RM = o.FP_MONT_R                 # R mod p: the Montgomery one
RI = o.FP_INV_MONT_R
MASK64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def alg():
    so = os.path.join(HERE, "libhostalg_shim.so")
    src = os.path.join(HERE, "hostalg_shim.cpp")
    csrc = os.path.join(HERE, "..", "..", "nim_groth16_amd", "csrc")
    deps = [src] + glob.glob(os.path.join(csrc, "*.cuh")) + glob.glob(os.path.join(csrc, "*.hpp")) + \
        glob.glob(os.path.join(csrc, "*.inc"))
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", src, "-o", so])
    lib = ctypes.CDLL(so)
    vp, i32, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    lib.shim_hfp_batch.argtypes = lib.shim_hfp2_batch.argtypes = [i32, sz, vp, vp, vp, vp, vp]
    lib.shim_host_add.argtypes = [i32, vp, vp, vp]
    lib.shim_host_mul.argtypes = [i32, vp, vp, vp]
    lib.shim_host_mul2.argtypes = [i32, vp, vp, vp, vp, vp]
    lib.shim_host_sum.argtypes = [i32, i32, vp, sz, sz, vp]
    lib.shim_combine_pre.argtypes = [vp] * 8
    lib.shim_combine_finish.argtypes = [vp] * 3
    lib.shim_sizes.restype = ctypes.c_uint32
    assert (lib.shim_sizes(0), lib.shim_sizes(1)) == (320, 384)
    return lib


class Points:
    """k -> k * G as bytes and as integers, from the C oracle's fixed-base multiplier, computed in batches and kept"""

    def __init__(self, orc):
        self.orc, self.raw = orc, ({0: bytes(64)}, {0: bytes(128)})

    def need(self, group, logs):
        t, psz = self.raw[group - 1], 64 * group
        new = sorted({k % R for k in logs} - t.keys())
        if new:
            buf = self.orc.fixed_base(group, b"".join(o.fr_to_mont_bytes(k) for k in new))
            t.update((k, buf[psz * i: psz * (i + 1)]) for i, k in enumerate(new))

    def b(self, group, k):
        k %= R
        if k not in self.raw[group - 1]:
            self.need(group, [k])
        return self.raw[group - 1][k]

    def aff(self, group, k):
        return (o.g1_from_bytes if group == 1 else o.g2_from_bytes)(self.b(group, k))


@pytest.fixture(scope="module")
def pts(orc):
    p = Points(orc)
    # the fixed-base multiplier itself, once, against the Python oracle's double-and-add: 0 -> (0,0)
    for g, C, gen, enc in ((1, o.G1, o.GEN1, o.g1_to_bytes), (2, o.G2, o.GEN2, o.g2_to_bytes)):
        for k in (0, 1, 2, R - 1, cp.ALPHA):
            assert p.b(g, k) == enc(C.mul(k, gen)), (g, k)
    return p


# ---- a. the field ---------------------------------------------------------------------------------------------------
def fp_pool(nrandom):
    """limb patterns below p.  Each special value twice: as the pattern itself, and as the standard value it is the
    Montgomery form of (x -> x R mod p)"""
    top = P >> 192
    low = (1 << 192) - 1
    g = o.SplitMix64(0xF1E1D)
    x = P // 2 + 1 + g.fr() % (P // 2 - 1)                        # above p / 2: 2 x - p is a value of its own
    y = 1 + g.fr() % (P // 2 - 1)
    special = [0, 1, 2, P - 1, P - 2, (P + 1) // 2, (P - 1) // 2, RM, RM * RM % P, P - RM,
               MASK64, MASK64 << 64, MASK64 << 128,               # 2^64 - 1 in one limb (in the top limb it exceeds p)
               ((top - 1) << 192) | low,                          # the largest pattern with all lower limbs full; with
               top << 192, (top << 192) | (P & low) - 1,          # p's own top limb such a pattern is not below p
               (top << 192) | (P & MASK64 << 128 & low),
               1 << 192, 1 << 253, (1 << 64), (1 << 128) - 1,
               x, P - x, 2 * x - P, y, P - y, 2 * y]
    assert all(0 <= v < P for v in special)
    pool = special + [v * RM % P for v in special] + [v * RI % P for v in (1, 2, P - 1)]
    pool += [g.fr() * g.fr() % P for _ in range(nrandom)]
    return list(dict.fromkeys(pool))


def _b32(v):
    return v.to_bytes(32, "little")


def _batch(fn, op, size, *ops):
    n = len(ops[0]) // size
    ops = list(ops) + [ops[0]] * (4 - len(ops))
    out = ctypes.create_string_buffer(size * n)
    fn(op, n, *ops, out)
    return out.raw


def test_hfp_every_function_on_the_limb_edges(alg):
    pool = fp_pool(40)
    n = len(pool)
    assert n >= 90

    def run(op, *cols):
        raw = _batch(alg.shim_hfp_batch, op, 32, *(b"".join(_b32(v) for v in col) for col in cols))
        return [int.from_bytes(raw[32 * i: 32 * i + 32], "little") for i in range(len(cols[0]))]
    # unary, on every element
    for op, fn in ((2, lambda a: -a % P), (3, lambda a: 2 * a % P), (5, lambda a: a * a * RI % P),
                   (8, lambda a: 2 * a % P), (9, lambda a: 3 * a % P), (10, lambda a: 4 * a % P),
                   (11, lambda a: 8 * a % P), (12, lambda a: RM if a == 0 else 0)):
        assert run(op, pool) == [fn(a) for a in pool], op
    # inv: a inv(a) = 1 and inv(a) = a^(p-2), both in the Montgomery domain (a = x R: inv = x^-1 R = a^-1 R^2)
    nz = [a for a in pool if a]
    inv = run(7, nz)
    assert inv == [pow(a * RI % P, P - 2, P) * RM % P for a in nz]
    assert run(4, nz, inv) == [RM] * len(nz)
    assert run(7, [0]) == [0]
    # binary: the pool crossed with itself
    A = [a for a in pool for _ in pool]
    B = pool * n
    assert run(0, A, B) == [(a + b) % P for a, b in zip(A, B)]
    assert run(1, A, B) == [(a - b) % P for a, b in zip(A, B)]
    assert run(4, A, B) == [a * b * RI % P for a, b in zip(A, B)]
    assert run(13, A, B) == [RM if a == b else 0 for a, b in zip(A, B)]
    # mulsub(a, b, c, d) = a b - c d: the cross again, against the same pairs shifted and transposed
    C = B[7:] + B[:7]
    D = A[n + 3:] + A[:n + 3]
    assert run(6, A, B, C, D) == [(a * b - c * d) * RI % P for a, b, c, d in zip(A, B, C, D)]
    assert run(6, A, B, A, B) == [0] * len(A) and run(6, A, B, B, A) == [0] * len(A)
    # the pairs the pool is built around are really in the cross: x + (p - x) = 0 exactly at the comparison with p
    assert sum(1 for a, b in zip(A, B) if a + b == P) >= 10 and sum(1 for a, b in zip(A, B) if a + b == P - 1) >= 2
    assert sum(1 for a, b in zip(A, B) if a + b >= 1 << 256) == 0          # (two reduced values never reach 2^256)
    assert any(a + b > P and (a + b) >> 192 == P >> 192 for a, b in zip(A, B))


def fp2_pool():
    g = o.SplitMix64(0xF2F2)
    top = P >> 192
    x = P // 2 + 1 + g.fr() % (P // 2 - 1)
    coord = [0, 1, P - 1, (P + 1) // 2, RM, P - RM, MASK64, ((top - 1) << 192) | ((1 << 192) - 1), x, P - x,
             g.fr() * g.fr() % P, g.fr() * g.fr() % P]
    return [(a, b) for a in coord for b in coord]


def test_hfp2_every_function_incl_the_zero_factors_of_sqr(alg):
    pool = fp2_pool()
    n = len(pool)
    assert n == 144
    assert sum(1 for a, b in pool if a == b) >= 12 and sum(1 for a, b in pool if a and (a + b) % P == 0) >= 6
    assert sum(1 for a, b in pool if a == 0) == 12 == sum(1 for a, b in pool if b == 0)
    enc = lambda col: b"".join(_b32(a) + _b32(b) for a, b in col)                    # noqa: E731
    mred = lambda z: (z[0] * RI % P, z[1] * RI % P)                                  # noqa: E731
    one, zero = (RM, 0), (0, 0)

    def run(op, *cols):
        raw = _batch(alg.shim_hfp2_batch, op, 64, *(enc(col) for col in cols))
        return [(int.from_bytes(raw[64 * i: 64 * i + 32], "little"), int.from_bytes(raw[64 * i + 32: 64 * i + 64], "little"))
                for i in range(len(cols[0]))]
    for op, fn in ((2, o.fp2_neg), (3, lambda a: o.fp2_add(a, a)), (5, lambda a: mred(o.fp2_sqr(a))),
                   (8, lambda a: o.fp2_scal(a, 2)), (9, lambda a: o.fp2_scal(a, 3)), (10, lambda a: o.fp2_scal(a, 4)),
                   (11, lambda a: o.fp2_scal(a, 8)), (12, lambda a: one if a == zero else zero)):
        assert run(op, pool) == [tuple(v % P for v in fn(a)) for a in pool], op
    nz = [a for a in pool if a != zero]
    inv = run(7, nz)
    std = lambda a: (a[0] * RI % P, a[1] * RI % P)                                   # noqa: E731
    assert inv == [tuple(v * RM % P for v in o.fp2_inv(std(a))) for a in nz]
    assert run(4, nz, inv) == [one] * len(nz)
    A = [a for a in pool for _ in pool]
    B = pool * n
    assert run(0, A, B) == [o.fp2_add(a, b) for a, b in zip(A, B)]
    assert run(1, A, B) == [o.fp2_sub(a, b) for a, b in zip(A, B)]
    prod = [mred(o.fp2_mul(a, b)) for a, b in zip(A, B)]
    assert run(4, A, B) == prod
    assert run(13, A, B) == [one if a == b else zero for a, b in zip(A, B)]
    C = B[5:] + B[:5]
    D = A[n + 1:] + A[:n + 1]
    prod2 = [mred(o.fp2_mul(c, d)) for c, d in zip(C, D)]
    assert run(6, A, B, C, D) == [o.fp2_sub(x, y) for x, y in zip(prod, prod2)]


# ---- b. the curve helpers -------------------------------------------------------------------------------------------
def mul_scalars():
    s = [0, 1, 2, 15, 16, 17, R - 1, R - 2, (R - 1) // 2, 1 << 253, cp.TOP_F, cp.ALL3]
    for j in range(1, 64):
        s += [1 << (4 * j - 1), 1 << (4 * j), 1 << (4 * j + 1)]
    s += [1 | 1 << 252, 0xF | 0xF << 248, 1 | 1 << 128 | 1 << 252, 0x9 << 200 | 0x7, 0xF << 124, 0x10001 << 60,
          int("1" * 63, 16), int("10" * 31, 16), int("01" * 32, 16)]                 # long zero runs, sparse nibbles
    g = o.SplitMix64(0xABCD)
    s += [g.fr() for _ in range(4)]
    assert all(0 <= k < R for k in s)
    return list(dict.fromkeys(s))


MUL2_SCALARS = [0, 1, 2, 3, R - 1, R - 2, cp.ALL3, 1 << 253, int("5" * 63, 16), cp.R0]   # thinned; ALL3: all windows 3
X1, X2 = cp.slot_seeds("a")                                                               # logs of two unrelated points


@pytest.mark.parametrize("group", [1, 2])
def test_host_add_exceptional_operands(alg, pts, group):
    psz = 64 * group
    out = ctypes.create_string_buffer(psz)
    pairs = [(X1, X2), (X1, X1), (X1, -X1), (0, X1), (X1, 0), (0, 0), (X2, 2 * X2), (-X1, X1), (1, 1), (1, R - 1)]
    pts.need(group, [x for a, b in pairs for x in (a, b, a + b)])
    for a, b in pairs:
        alg.shim_host_add(group, pts.b(group, a), pts.b(group, b), out)
        assert out.raw == pts.b(group, a + b), (group, cp.kind(a, b), a, b)
    # the same through the two running sums the kernels use: [k, k] with ZZ = 1 (mixed and general addition), the list
    # pictures with every scaling of the records
    for mode in (0, 1):
        rec = b"".join(pts.b(group, X1) if mode == 0 else cp.xyzz_bytes(group, pts.aff(group, X1), cp.lam_of("unit", group, 0))
                       for _ in range(2))
        alg.shim_host_sum(group, mode, rec, 2, len(rec) // 2, out)
        assert out.raw == pts.b(group, 2 * X1), (group, mode)


@pytest.mark.parametrize("group", [1, 2])
def test_list_pictures_through_the_host_instantiation_of_the_kernel_sums(alg, pts, group):
    """Curve<HFp> / Curve<HFp2>::add over XYZZ records, as prove_combine_kernel and sum_partials_kernel run Curve<Fp> /
    Curve<Fp2>::add on the GPU: every list picture at 1, 2, 3, 8 and 64 records, every scaling"""
    out = ctypes.create_string_buffer(64 * group)
    k, m = cp.slot_seeds("b2" if group == 2 else "h")
    ran = 0
    sizes = (1, 2, 3, 8, 64)
    pts.need(group, [x for n in sizes for _, build in cp.list_pictures(n) for x in build(n, k, m) + [sum(build(n, k, m))]])
    for n in sizes:
        for name, build in cp.list_pictures(n):
            logs = build(n, k, m)
            for mode in cp.LAMBDA_MODES:
                rec = b"".join(cp.xyzz_bytes(group, pts.aff(group, x), cp.lam_of(mode, group, i)) for i, x in enumerate(logs))
                alg.shim_host_sum(group, 1, rec, n, 128 * group, out)
                assert out.raw == pts.b(group, sum(logs)), (group, n, name, mode)
                ran += 1
    assert ran >= 120


@pytest.mark.parametrize("group", [1, 2])
def test_host_mul_window_edges(alg, pts, group):
    out = ctypes.create_string_buffer(64 * group)
    ks = mul_scalars()
    assert len(ks) >= 200
    pts.need(group, [k * x for k in ks for x in (X1, 1, R - 1)])
    for x in (X1, 1, 0, R - 1):                            # a random point, the generator, infinity, -G
        for k in ks:
            alg.shim_host_mul(group, o.fr_to_std_bytes(k), pts.b(group, x), out)
            assert out.raw == pts.b(group, k * x), (group, hex(k), x)


@pytest.mark.parametrize("group", [1, 2])
def test_host_mul2_tables_through_infinity_and_doublings(alg, pts, group):
    out = ctypes.create_string_buffer(64 * group)
    ks = MUL2_SCALARS
    # p2 = p1, -p1, 2 p1, 3 p1, -2 p1, an unrelated point, infinity; and p1 = infinity
    bases = [(X1, X1), (X1, -X1), (X1, 2 * X1), (X1, 3 * X1), (X1, -2 * X1), (X1, X2), (X1, 0), (0, X2), (0, 0)]
    pts.need(group, [k1 * x1 + k2 * x2 for x1, x2 in bases for k1 in ks for k2 in ks])
    for x1, x2 in bases:
        for k1 in ks:
            for k2 in ks:
                alg.shim_host_mul2(group, o.fr_to_std_bytes(k1), pts.b(group, x1), o.fr_to_std_bytes(k2), pts.b(group, x2), out)
                assert out.raw == pts.b(group, k1 * x1 + k2 * x2), (group, hex(k1), hex(k2), x1 == X1, x2 % R)
    # what those bases do to the table i p1 + j p2 (log space), beyond its two own doublings 2 p1 and 2 p2: the mixed
    # addition that forms an entry meets p1 again, or -p1 and leaves an entry at infinity
    for (x1, x2), want in ((bases[0], "equal"), (bases[1], "opposite"), (bases[4], "opposite")):
        kinds = [cp.kind((i - 1) * x1 + j * x2, x1) for i in range(1, 4) for j in range(1, 4)]
        assert want in kinds, (x2 % R, kinds)


# ---- c. the combine algebra as a whole ------------------------------------------------------------------------------
def run_combine(alg, pts, r, s, sums):
    key = [pts.b(1, cp.ALPHA), pts.b(1, cp.BETA), pts.b(1, cp.DELTA), pts.b(2, cp.BETA), pts.b(2, cp.DELTA)]
    pre = ctypes.create_string_buffer(320)
    alg.shim_combine_pre(*key, o.fr_to_mont_bytes(r), o.fr_to_mont_bytes(s), pre)
    a, b1, b2, h, c = sums
    res = pts.b(1, a) + pts.b(1, b1) + pts.b(2, b2) + pts.b(1, h) + pts.b(1, c)
    out = ctypes.create_string_buffer(256)
    alg.shim_combine_finish(pre, res, out)
    return pre.raw, out.raw


def proof_bytes(pts, logs):
    return pts.b(1, logs[0]) + pts.b(2, logs[1]) + pts.b(1, logs[2])


def test_combine_algebra_against_the_closed_form(alg, pts):
    pics = cp.mask_pictures()
    assert len(pics) >= 50 and len({p.name for p in pics}) == len(pics)
    jobs = [(p.name, p.r, p.s, p.sums) for p in pics]
    # the sums of the list pictures, given directly ("count = 1"): every slot its own picture
    for n in cp.COMBINE_COUNTS:
        for shift in range(len(cp.list_pictures(n))):
            logs = cp.record_logs(n, cp.mixed_names(n, shift))
            jobs.append(((n, shift), cp.R0, cp.S0, tuple(sum(logs[slot]) % R for slot in cp.SLOTS)))
    g1, g2 = [], []
    for _, r, s, sums in jobs:                              # every point of every job in two calls of the multiplier
        pre, exp = cp.pre_logs(r, s), cp.expected_logs(r, s, *sums)
        g1 += [sums[0], sums[1], sums[3], sums[4], pre[0], pre[2], exp[0], exp[2]]
        g2 += [sums[2], pre[1], exp[1]]
    pts.need(1, g1)
    pts.need(2, g2)
    for name, r, s, sums in jobs:
        pre, proof = run_combine(alg, pts, r, s, sums)
        ap, bp, cpre = cp.pre_logs(r, s)
        assert pre[:64] == o.fr_to_std_bytes(r) + o.fr_to_std_bytes(s), name
        assert pre[64:] == pts.b(1, ap) + pts.b(2, bp) + pts.b(1, cpre), name
        assert proof == proof_bytes(pts, cp.expected_logs(r, s, *sums)), name


def test_every_picture_reaches_the_branch_it_is_named_for():
    """in log space (nothing is instrumented): the operand logs of each addition of the walk"""
    seen = {}
    for p in cp.mask_pictures():
        t, got = cp.walk_combine(p.r, p.s, p.sums)
        assert got == p.expected(), p.name                 # a check OF the walk: it regroups the closed form faithfully
        for cell, kind in p.reach:
            assert t[cell][kind] >= 1, (p.name, cell, kind, {c: dict(v) for c, v in t.items()})
        for cell, kinds in t.items():
            seen.setdefault(cell, set()).update(kinds)
    # every addition of the two halves meets an equal, an opposite and an infinite operand somewhere in the list
    for cell in ("pi_a", "pi_b", "pi_c.t", "pi_c.h", "pi_c.c"):
        assert {"inf", "equal", "opposite", "generic"} <= seen[cell], (cell, seen[cell])
    for cell in ("a_pre", "b_pre", "c_pre"):
        assert {"inf", "opposite", "generic"} <= seen[cell], (cell, seen[cell])
    assert {"inf", "equal", "opposite", "empty", "generic"} <= seen["fin.mul2.tab"]
    # pi_a = alpha1, pi_b = beta2, pi_c = infinity when everything is zero
    zero = [p for p in cp.mask_pictures() if p.name == "all_zero,r=s=0"][0]
    assert zero.expected() == (cp.ALPHA, cp.BETA, 0)
    # the list pictures: what the running sum of a slot meets
    k, m = cp.slot_seeds("a")
    for name, (build, kinds) in cp.LIST_PICTURES.items():
        for n in cp.COMBINE_COUNTS + cp.SUM_COUNTS:
            logs = build(n, k, m)
            if logs is None:
                assert n < 3, (name, n)
                continue
            t, total = cp.walk_list(logs)
            assert total == sum(logs) % R and len(logs) == n
            if n >= 3:
                for kd in kinds:
                    assert t[kd] >= 1, (name, n, kd, dict(t))
    big = {name: cp.walk_list(build(1024, k, m))[0] for name, (build, _) in cp.LIST_PICTURES.items()}
    assert big["all_infinity"] == {"empty": 1024} and big["same_record"]["equal"] == 1 == big["k_2k_3k"]["equal"]
    assert big["alternating"] == {"inf": 512, "opposite": 512}
    assert big["k_-k_m"]["opposite"] == 1 and big["k_-k_m"]["inf"] == 2 and big["k_-k_m"]["generic"] == 1021
    # the slots' seeds are independent: no two slots of a picture share a sum (b1 and b2 differ) unless the picture's
    # sum is infinity by construction
    for n in (1, 2, 3, 8, 1024):
        for name, _ in cp.list_pictures(n):
            sums = [sum(v) % R for v in cp.record_logs(n, name).values()]
            assert len(set(sums)) == 5 or set(sums) == {0}, (n, name)


def test_closed_form_equals_the_oracle_prover_on_the_toy_circuit():
    """the logs of the toy witness' five sums (combine_pictures.toy_sum_logs) and the closed form, against the oracle's
    own generateProofWithMask on points"""
    sums = cp.toy_sum_logs()
    zk = o.fake_circuit_setup(o.toy_r1cs(), o.ToxicWaste(*cp.TOXIC), o.SNARKJS)
    for r, s in ((cp.R0, cp.S0), (0, 0)):
        pr = o.generate_proof_with_mask(zk, o.TOY_WITNESS, r, s)
        la, lb, lc = cp.expected_logs(r, s, *sums)
        assert (pr.pi_a, pr.pi_b, pr.pi_c) == (o.G1.mul(la, o.GEN1), o.G2.mul(lb, o.GEN2), o.G1.mul(lc, o.GEN1))
    # the pictures that solve for the mask land where they are meant to
    for p in cp.mask_pictures(sums):
        t, got = cp.walk_combine(p.r, p.s, p.sums)
        assert got == p.expected() and p.sums == sums, p.name
        for cell, kind in p.reach:
            assert t[cell][kind] >= 1, (p.name, cell, kind)
        if p.name.startswith("pi_c=inf"):
            assert got[2] == 0, p.name
