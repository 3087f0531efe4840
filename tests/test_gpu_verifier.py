"""GPU parity for the verifier row through the C ABI: the raw ate pairing bit-exact against the
oracle, and verifyProof on the reference's toy circuit (tests/groth16/testProver.nim:59-73: prove -> verify),
incl. the negative cases (tampered proof / public input, malformed points, subgroup check); instances built in log
space (points at infinity on every side, vk_x at infinity, edge public inputs, no public input, a B of small order)
with the verdict of the oracle's Miller loop and final exponentiation on the same points."""
import pytest

from oracle import bn254_ref as o
from tests import device_ops as D
from tests import inputs as I

pytestmark = pytest.mark.gpu

_gt = D.gt_from_bytes       # 384-byte flat Fp12 (6 x Fp2 over w^k, Montgomery) -> the oracle's degree-12 polynomial basis


def test_pairing_vs_oracle_and_bilinear(ctx):
    rng = o.SplitMix64(31)
    ks = [(rng.fr(), rng.fr()) for _ in range(3)]
    Ps = [o.G1.mul(a, o.GEN1) for a, _ in ks] + [o.INF_G1, o.GEN1, o.G1.mul(ks[0][0] * ks[0][1] % o.R, o.GEN1)]
    Qs = [o.G2.mul(b, o.GEN2) for _, b in ks] + [o.GEN2, o.INF_G2, o.GEN2]
    raw = ctx.pairing(b"".join(o.g1_to_bytes(p) for p in Ps), b"".join(o.g2_to_bytes(q) for q in Qs))
    gts = [_gt(raw[384 * i:384 * i + 384]) for i in range(len(Ps))]
    assert gts[0] == o.pairing(Ps[0], Qs[0])                 # bit-exact incl. the final exponentiation
    for i, (p, q) in enumerate(zip(Ps, Qs)):                  # ... and every other finite pairing of the batch
        if p != o.INF_G1 and q != o.INF_G2:
            assert gts[i] == o.pairing(p, q), i
    assert gts[3] == o._f12_one() and gts[4] == o._f12_one()  # infinity on either side
    assert gts[5] == gts[0]                                   # e(aP, bQ) == e(abP, Q)
    assert gts[1] != gts[2] and gts[1] != o._f12_one()
    assert ctx.pairing(b"", b"") == b""


def _toy(ctx, flavour=1):
    from nim_groth16_amd import Mask, Witness, generateProofWithMask
    from nim_groth16_amd.fake_setup import R1CS, ToxicWaste, fakeCircuitSetup
    rng = o.SplitMix64(5)
    a, b, g, d, t = (rng.fr() for _ in range(5))
    zk = fakeCircuitSetup(R1CS(8, 1, 1, 3, o.toy_r1cs().constraints), ToxicWaste(a, b, g, d, t), flavour, ctx)
    wt = Witness("bn128", 8, I.fr_mont_bytes(o.TOY_WITNESS))
    m = o.SplitMix64(6)
    return zk, [generateProofWithMask(0, False, zk, wt, Mask(m.fr(), m.fr()), ctx) for _ in range(2)]


@pytest.mark.parametrize("flavour", [0, 1])
def test_verify_toy_proofs(ctx, flavour):
    import dataclasses
    from nim_groth16_amd import extractVKey, loadVerifyingKey, verifyProof, verifyProofs
    zk, proofs = _toy(ctx, flavour)
    vkey = extractVKey(zk)
    assert vkey.npubs == 2
    assert verifyProof(vkey, proofs[0], ctx)                  # testProver.nim:65-73
    dev = loadVerifyingKey(vkey, ctx)
    good, other = proofs
    bad_c = dataclasses.replace(good, pi_c=other.pi_c)
    bad_a = dataclasses.replace(good, pi_a=o.g1_to_bytes(o.G1.mul(7, o.GEN1)))
    bad_pub = dataclasses.replace(good, publicIO=I.fr_mont_bytes([1, 2024, 1022]))
    zero_pub = dataclasses.replace(good, publicIO=I.fr_mont_bytes([1, 0, 0]))
    res = verifyProofs(dev, [good, bad_c, other, bad_a, bad_pub, zero_pub], ctx, subgroup=True)
    assert res == [True, False, True, False, False, False]
    # agreement with the oracle's verifier on the same objects
    from tests.test_gpu_prover import _zkey_to_oracle
    oz = _zkey_to_oracle(zk)
    for prf, exp in zip([good, bad_c, bad_pub], [True, False, False]):
        ref = o.Proof(I.fr_from_mont(prf.publicIO), o.g1_from_bytes(prf.pi_a), o.g2_from_bytes(prf.pi_b),
                      o.g1_from_bytes(prf.pi_c))
        assert o.verify_proof(oz, ref) == exp


def test_verify_rejects_malformed_points(ctx):
    import dataclasses
    from nim_groth16_amd import extractVKey, loadVerifyingKey, verifyProof
    zk, (good, _) = _toy(ctx)
    dev = loadVerifyingKey(extractVKey(zk), ctx)
    off_g1 = o.fp_to_mont_bytes(5) + o.fp_to_mont_bytes(7)             # not on y^2 = x^3 + 3
    with pytest.raises(AssertionError, match="pi_a is not in G1"):
        verifyProof(dev, dataclasses.replace(good, pi_a=off_g1), ctx)
    with pytest.raises(AssertionError, match="pi_c is not in G1"):
        verifyProof(dev, dataclasses.replace(good, pi_c=off_g1), ctx)
    with pytest.raises(AssertionError, match="pi_b is not in G2"):
        verifyProof(dev, dataclasses.replace(good, pi_b=bytes(good.pi_b[:64]) + bytes(64)), ctx)
    # a point of the twist outside the order-r subgroup: on the curve (the reference would accept it as input
    # and fail the pairing equation); with subgroup=True it is refused up front
    x = (3, 1)
    while True:
        rhs = o.fp2_add(o.fp2_mul(o.fp2_sqr(x), x), o.TWIST_B)
        y = _fp2_sqrt(rhs)
        if y is not None and not o.G2.is_inf(o.G2.mul(o.R, (x, y))):
            break
        x = (x[0] + 1, x[1])
    rogue = dataclasses.replace(good, pi_b=o.g2_to_bytes((x, y)))
    assert dev.verify([(rogue.pi_a, rogue.pi_b, rogue.pi_c)], rogue.publicIO) == [0]
    assert dev.verify([(rogue.pi_a, rogue.pi_b, rogue.pi_c)], rogue.publicIO, subgroup=True) == [-4]
    assert dev.verify([], b"") == []


def test_verify_batch_of_mixed_outcomes_across_block_boundaries(ctx):
    """131 proofs in one g16_verify call: three Miller values per proof, so the kernels' t / 3 indexing crosses two
    64-lane block boundaries; every status code in one batch, each at its own index; of two defects the smallest
    code wins"""
    import dataclasses
    from nim_groth16_amd import extractVKey, loadVerifyingKey
    zk, (good, other) = _toy(ctx)
    dev = loadVerifyingKey(extractVKey(zk), ctx)
    off_g1 = o.fp_to_mont_bytes(5) + o.fp_to_mont_bytes(7)             # not on y^2 = x^3 + 3
    off_g2 = bytes(good.pi_b[:64]) + bytes(64)
    x = (3, 1)
    while True:                                                        # on the twist, outside the order-r subgroup
        y = _fp2_sqrt(o.fp2_add(o.fp2_mul(o.fp2_sqr(x), x), o.TWIST_B))
        if y is not None and not o.G2.is_inf(o.G2.mul(o.R, (x, y))):
            break
        x = (x[0] + 1, x[1])
    ax = int.from_bytes(good.pi_a[:32], "little")
    noncanon_a = (ax + o.P).to_bytes(32, "little") + bytes(good.pi_a[32:])      # the same residue, limbs >= p
    pub = bytes(good.publicIO)
    noncanon_pub = pub[:32] + (int.from_bytes(pub[32:64], "little") + o.R).to_bytes(32, "little") + pub[64:]
    rep = dataclasses.replace
    kinds = [(good, 1), (other, 1), (rep(good, pi_c=other.pi_c), 0), (rep(good, pi_a=off_g1), -1),
             (rep(good, pi_b=off_g2), -2), (rep(good, pi_c=off_g1), -3), (rep(good, pi_b=o.g2_to_bytes((x, y))), -4),
             (rep(good, pi_a=noncanon_a), -5), (rep(good, publicIO=noncanon_pub), -6),
             (rep(good, pi_a=off_g1, pi_c=off_g1), -3),                                  # two defects: -1 and -3
             (rep(good, pi_a=off_g1, publicIO=noncanon_pub), -6),                        # -1 and -6
             (rep(good, pi_b=off_g2, pi_a=noncanon_a), -5)]                              # -2 and -5
    n = 131
    batch = [kinds[(5 * i + i // len(kinds)) % len(kinds)] for i in range(n)]
    assert {e for _, e in batch} == {1, 0, -1, -2, -3, -4, -5, -6}
    st = dev.verify([(p.pi_a, p.pi_b, p.pi_c) for p, _ in batch], b"".join(bytes(p.publicIO) for p, _ in batch),
                    mont=True, subgroup=True)
    assert st == [e for _, e in batch], [(i, s, e) for i, (s, (_, e)) in enumerate(zip(st, batch)) if s != e]
    # alone, each kind gives the same answer as in the batch
    for p, e in kinds:
        assert dev.verify([(p.pi_a, p.pi_b, p.pi_c)], bytes(p.publicIO), mont=True, subgroup=True) == [e]


def _fp2_sqrt(a):
    """square root in Fp2 = Fp[u]/(u^2+1) (p = 3 mod 4), or None"""
    p = o.P
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


# ---- instances built in log space: the verdict is known without a prover ----------------------------------------------
# A = a G1, B = b G2, C = c G1, alpha1 = alpha G1, beta2 = beta G2, gamma2 = gamma G2, delta2 = delta G2, IC_i = ic_i G1:
#   e(-A, B) e(alpha1, beta2) e(C, delta2) e(sum pub_i IC_i, gamma2) = 1   <=>   -ab + alpha beta + c delta + x gamma = 0
# (mod r), x = sum pub_i ic_i with pub_0 = 1.
class _LogKey:
    def __init__(self, ctx, seed, npubs):
        from nim_groth16_amd.verifier import VKey, loadVerifyingKey
        from nim_groth16_amd.zkey_types import SpecPoints
        rng = o.SplitMix64(seed)
        self.alpha, self.beta, self.gamma, self.delta = (rng.fr() or 1 for _ in range(4))
        self.ics = [rng.fr() or 1 for _ in range(npubs + 1)]
        self.rng = rng
        self.alpha1, self.beta2 = o.G1.mul(self.alpha, o.GEN1), o.G2.mul(self.beta, o.GEN2)
        self.gamma2, self.delta2 = o.G2.mul(self.gamma, o.GEN2), o.G2.mul(self.delta, o.GEN2)
        self.ic = [o.G1.mul(k, o.GEN1) for k in self.ics]
        spec = SpecPoints(alpha1=o.g1_to_bytes(self.alpha1), beta2=o.g2_to_bytes(self.beta2),
                          gamma2=o.g2_to_bytes(self.gamma2), delta2=o.g2_to_bytes(self.delta2))
        self.dev = loadVerifyingKey(VKey("bn128", spec, b"".join(o.g1_to_bytes(q) for q in self.ic)), ctx)
        self.ab = D.miller_ref(self.alpha1, self.beta2)

    def x(self, pubs):
        return sum(p * k for p, k in zip(pubs, self.ics)) % o.R

    def solve_c(self, a, b, pubs):
        return (a * b - self.alpha * self.beta - self.x(pubs) * self.gamma) * pow(self.delta, -1, o.R) % o.R

    def solve_a(self, b, c, pubs):
        return (self.alpha * self.beta + c * self.delta + self.x(pubs) * self.gamma) * pow(b, -1, o.R) % o.R

    def holds(self, a, b, c, pubs):
        return (-a * b + self.alpha * self.beta + c * self.delta + self.x(pubs) * self.gamma) % o.R == 0

    def oracle_status(self, A, B, C, pubs):
        """the pairing product of verifier.nim:31-52 with the oracle's Miller loop and final exponentiation"""
        vk_x = o.G1.msm_naive(pubs, self.ic)
        f = list(self.ab)
        for Pt, Q in ((o.G1.neg(A), B), (C, self.delta2), (vk_x, self.gamma2)):
            f = o._f12_mul(f, o.miller_loop(Pt, Q))
        return 1 if o.final_exp(f) == o._f12_one() else 0


def _run_instances(key, insts, subgroup=False):
    """insts: (A, B, C, pubs, expected status).  Each alone and all in one batch (twice over, so that lanes differ),
    with the public inputs in Montgomery and in standard form: the same statuses"""
    proofs = [(o.g1_to_bytes(A), o.g2_to_bytes(B), o.g1_to_bytes(C)) for A, B, C, _, _ in insts]
    want = [e for *_, e in insts]
    for mont in (True, False):
        enc = I.fr_mont_bytes if mont else (lambda xs: b"".join(o.fr_to_std_bytes(x) for x in xs))
        pub = [enc(pubs) for _, _, _, pubs, _ in insts]
        for i in range(len(insts)):
            assert key.dev.verify([proofs[i]], pub[i], mont=mont, subgroup=subgroup) == [want[i]], (i, mont)
        order = list(range(len(insts))) + list(reversed(range(len(insts))))
        st = key.dev.verify([proofs[i] for i in order], b"".join(pub[i] for i in order), mont=mont, subgroup=subgroup)
        assert st == [want[i] for i in order], (mont, st)


LOG_CASES = ("A_inf", "C_inf", "B_inf", "vk_x_inf", "pub_0_and_r_minus_1", "npubs_0")


@pytest.mark.parametrize("case", LOG_CASES)
def test_verify_log_space_instances(ctx, case):
    """an accepting instance and a neighbour that is off by one in a single scalar; the expected status is the
    oracle's verdict on the same points, and it is 1 and 0 as the scalars say"""
    key = _LogKey(ctx, 40 + LOG_CASES.index(case), 0 if case == "npubs_0" else 2)
    rng = key.rng
    a, b, c = rng.fr() or 1, rng.fr() or 1, rng.fr() or 1
    pubs = [1] + [rng.fr() for _ in range(len(key.ics) - 1)]
    if case == "A_inf":
        a = 0
    elif case == "B_inf":
        b = 0
    elif case == "vk_x_inf":      # the public inputs cancel IC_0
        pubs[1] = -(key.ics[0] + pubs[2] * key.ics[2]) * pow(key.ics[1], -1, o.R) % o.R
        assert key.x(pubs) == 0
    elif case == "pub_0_and_r_minus_1":
        pubs = [1, 0, o.R - 1]
    if case == "C_inf":
        c = 0
        a = key.solve_a(b, c, pubs)
        scalars = [(a, b, c, pubs), ((a + 1) % o.R, b, c, pubs)]
    else:
        c = key.solve_c(a, b, pubs)
        scalars = [(a, b, c, pubs), (a, b, (c + 1) % o.R, pubs)]
    if case == "vk_x_inf":
        scalars.append((a, b, c, [1, (pubs[1] + 1) % o.R, pubs[2]]))
    elif case == "pub_0_and_r_minus_1":
        scalars += [(a, b, c, [1, 1, o.R - 1]), (a, b, c, [1, 0, o.R - 2])]
    insts = []
    for k, (a_, b_, c_, pubs_) in enumerate(scalars):
        A, B, C = o.G1.mul(a_, o.GEN1), o.G2.mul(b_, o.GEN2), o.G1.mul(c_, o.GEN1)
        status = key.oracle_status(A, B, C, pubs_)
        assert status == (1 if k == 0 else 0) and key.holds(a_, b_, c_, pubs_) == (k == 0)
        insts.append((A, B, C, pubs_, status))
    A, B, C, pubs0, _ = insts[0]
    assert {"A_inf": A == o.INF_G1, "B_inf": B == o.INF_G2, "C_inf": C == o.INF_G1,
            "vk_x_inf": o.G1.msm_naive(pubs0, key.ic) == o.INF_G1}.get(case, True)
    _run_instances(key, insts)
    _run_instances(key, insts, subgroup=True)       # every B here is in the subgroup (or at infinity)
    key.dev.destroy()


def test_verify_b_of_small_order(ctx):
    """B of order 10069 on the twist (the G2 cofactor 2p - r is 10069 x a 241-bit number): without the subgroup flag
    the status is the oracle's verdict on that pairing product, with it -4; next to an accepting instance"""
    key = _LogKey(ctx, 50, 2)
    rng = key.rng
    small, _ = D.twist_points()
    a, b = rng.fr() or 1, rng.fr() or 1
    pubs = [1, rng.fr(), rng.fr()]
    c = key.solve_c(a, b, pubs)
    A, C = o.G1.mul(a, o.GEN1), o.G1.mul(c, o.GEN1)
    good = (A, o.G2.mul(b, o.GEN2), C, pubs)
    rogue = (A, small, C, pubs)
    st_good, st_rogue = key.oracle_status(*good), key.oracle_status(*rogue)
    assert st_good == 1 and st_rogue == 0     # a product with a factor outside GT's order-r structure is not 1
    _run_instances(key, [good + (st_good,), rogue + (st_rogue,)])
    _run_instances(key, [good + (1,), rogue + (-4,)], subgroup=True)
    key.dev.destroy()


def test_pairing_batch_with_infinities_across_block_boundaries(ctx):
    """131 pairs in one g16_pairing call (three 64-lane blocks, the last one partial), infinity on either side or both at
    lanes 0, 63, 64, 127 and the last; every finite lane is one of three pairs whose oracle value is computed once"""
    rng = o.SplitMix64(61)
    distinct = [(o.GEN1, o.GEN2), (o.G1.mul(rng.fr(), o.GEN1), o.G2.mul(rng.fr(), o.GEN2)),
                (o.G1.neg(o.G1.mul(rng.fr(), o.GEN1)), o.G2.mul(rng.fr(), o.GEN2))]
    want = [o.final_exp(list(D.miller_ref(p, q))) for p, q in distinct]
    n = 131
    infs = {0: (o.INF_G1, distinct[0][1]), 63: (distinct[1][0], o.INF_G2), 64: (o.INF_G1, o.INF_G2),
            127: (o.INF_G1, distinct[2][1]), n - 1: (distinct[2][0], o.INF_G2)}
    lanes = [infs.get(i, distinct[(i + i // 64) % 3]) for i in range(n)]
    raw = ctx.pairing(b"".join(o.g1_to_bytes(p) for p, _ in lanes), b"".join(o.g2_to_bytes(q) for _, q in lanes))
    assert len(raw) == 384 * n
    for i in range(n):
        exp = o._f12_one() if i in infs else want[(i + i // 64) % 3]
        assert _gt(raw[384 * i:384 * i + 384]) == exp, i
