"""Batches for the random-linear-combination verifier (g16_verify_batch), built in log space: every point is a known
multiple of a generator, so each expected verdict is integer arithmetic mod r and owes nothing to the code under test.

    A_j = a_j G1, B_j = b_j G2, C_j = c_j G1, alpha1 = alpha G1, beta2 = beta G2, gamma2 = gamma G2, delta2 = delta G2,
    IC_i = ic_i G1, x_j = sum_i pub_{j,i} ic_i:

    defect_j = -a_j b_j + alpha beta + c_j delta + x_j gamma          (proof j verifies alone  <=>  defect_j = 0)
    batch accepts  <=>  sum_j z_j defect_j = 0  (mod r)               (and no proof is malformed)

picture(kind, count, at) -> Picture(proofs, pubs, multipliers, expected result, expected statuses); the statuses are
all 1 for an accepted batch and the per-proof verdicts (with the order-r check) for a rejected one."""
import functools
from dataclasses import dataclass, field
from typing import List

from oracle import bn254_ref as o

R = o.R
Z_MAX = (1 << 128) - 1
Z_EDGE = (1, Z_MAX, 1 << 127, 3, (1 << 64) + 1, (1 << 127) + 1, 2, 1 << 64)      # cycled over a batch


@functools.lru_cache(None)
def g1(k):
    return o.G1.mul(k % R, o.GEN1)


@functools.lru_cache(None)
def g2(k):
    return o.G2.mul(k % R, o.GEN2)


class Model:
    """a verification key in log space; needs no GPU"""

    def __init__(self, seed, npubs):
        self.rng = rng = o.SplitMix64(seed)
        self.alpha, self.beta, self.gamma, self.delta = (rng.fr() or 1 for _ in range(4))
        self.ics = [rng.fr() or 1 for _ in range(npubs + 1)]
        self.npubs = npubs

    alpha1 = property(lambda self: g1(self.alpha))
    beta2 = property(lambda self: g2(self.beta))
    gamma2 = property(lambda self: g2(self.gamma))
    delta2 = property(lambda self: g2(self.delta))
    ic = property(lambda self: [g1(k) for k in self.ics])

    def x(self, pubs):
        return sum(p * k for p, k in zip(pubs, self.ics)) % R

    def solve_c(self, a, b, pubs):
        return (a * b - self.alpha * self.beta - self.x(pubs) * self.gamma) * pow(self.delta, -1, R) % R

    def solve_a(self, b, c, pubs):
        return (self.alpha * self.beta + c * self.delta + self.x(pubs) * self.gamma) * pow(b, -1, R) % R

    def defect(self, a, b, c, pubs):
        return (-a * b + self.alpha * self.beta + c * self.delta + self.x(pubs) * self.gamma) % R

    def accepts(self, scalars, zs):
        return sum(z * self.defect(*s) for s, z in zip(scalars, zs)) % R == 0

    def load(self, ctx):
        from nim_groth16_amd.verifier import VKey, loadVerifyingKey
        from nim_groth16_amd.zkey_types import SpecPoints
        spec = SpecPoints(alpha1=o.g1_to_bytes(self.alpha1), beta2=o.g2_to_bytes(self.beta2),
                          gamma2=o.g2_to_bytes(self.gamma2), delta2=o.g2_to_bytes(self.delta2))
        return loadVerifyingKey(VKey("bn128", spec, b"".join(o.g1_to_bytes(q) for q in self.ic)), ctx)


@dataclass
class Picture:
    model: Model
    scalars: list                    # (a, b, c, pubs) per proof
    multipliers: List[int]
    result: int
    statuses: List[int]
    proofs: list = field(default=None)          # (pi_a, pi_b, pi_c) byte triples
    pub_bytes: dict = field(default_factory=dict)   # proof index -> raw bytes of its public inputs, if not from `scalars`

    def __post_init__(self):
        if self.proofs is None:
            self.proofs = [(o.g1_to_bytes(g1(a)), o.g2_to_bytes(g2(b)), o.g1_to_bytes(g1(c)))
                           for a, b, c, _ in self.scalars]

    @property
    def pubs(self):
        return [p for _, _, _, p in self.scalars]

    def public_io(self, mont):
        from tests import inputs as I
        enc = I.fr_mont_bytes if mont else (lambda xs: b"".join(o.fr_to_std_bytes(x) for x in xs))
        rows = [self.pub_bytes[j] if j in self.pub_bytes else enc(p) for j, p in enumerate(self.pubs)]
        return b"".join(rows)

    def points(self):
        return [(g1(a), g2(b), g1(c)) for a, b, c, _ in self.scalars]


SCALAR_KINDS = ("valid", "one_bad", "cancel_equal", "cancel_unequal", "cancel_wide", "cancel_wide_broken",
                "cancel_pub", "cancel_a_c", "A_inf", "B_inf", "C_inf", "vk_x_inf", "sum_zC_inf", "sum_sIC_inf",
                "same_twice", "opposite_C", "npubs_0")
EXPECTED = {"one_bad": 0, "cancel_unequal": 0, "cancel_wide_broken": 0}          # every other kind: 1
PAIR_KINDS = ("cancel_equal", "cancel_unequal", "cancel_wide", "cancel_wide_broken", "cancel_pub", "cancel_a_c",
              "same_twice", "opposite_C")
STRUCTURAL = {"off_curve_a": -1, "off_curve_b": -2, "off_curve_c": -3, "small_order_b": -4, "noncanonical_coord": -5,
              "noncanonical_pub": -6}


def picture(kind, count=3, at=None, seed=None):
    """`at`: the index of the special proof (or the pair of indices, for PAIR_KINDS); default: the first (two)"""
    npubs = 0 if kind == "npubs_0" else 2
    m = Model(900 + (SCALAR_KINDS.index(kind) if seed is None else seed), npubs)
    rng = m.rng
    pair = kind in PAIR_KINDS
    at = at if at is not None else ((0, 1) if pair else 0)
    i0, i1 = at if pair else (at, None)
    assert count > (i1 if pair else i0)
    # three distinct accepting proofs, cycled; the kinds that make a tree add two chosen points keep every other C at
    # infinity, so that the two meet unchanged wherever the tree joins their lanes
    c_inf_base = kind in ("same_twice", "opposite_C")
    pool = []
    for _ in range(min(count, 3)):
        b = rng.fr() or 1
        pubs = [1] + [rng.fr() for _ in range(npubs)]
        if c_inf_base:
            c = 0
            a = m.solve_a(b, c, pubs)
        else:
            a = rng.fr() or 1
            c = m.solve_c(a, b, pubs)
        pool.append((a, b, c, pubs))
    sc = [pool[j % len(pool)] for j in range(count)]
    zs = [Z_EDGE[j % len(Z_EDGE)] if j % 16 < 8 else (rng.fr() & Z_MAX) or 1 for j in range(count)]
    inv = lambda v: pow(v, -1, R)   # noqa: E731

    def fresh(c=None, b=None, pubs=None, a=None):
        """an accepting proof of its own"""
        b = (rng.fr() or 1) if b is None else b
        pubs = ([1] + [rng.fr() for _ in range(npubs)]) if pubs is None else pubs
        if c is not None:
            return (m.solve_a(b, c, pubs), b, c, pubs)
        a = (rng.fr() or 1) if a is None else a
        return (a, b, m.solve_c(a, b, pubs), pubs)

    def shift(s, da=0, dc=0, dpub=0):
        a, b, c, pubs = s
        pubs = list(pubs)
        if dpub:
            pubs[1] = (pubs[1] + dpub) % R
        return ((a + da) % R, b, (c + dc) % R, pubs)

    if kind == "one_bad":
        sc[i0] = shift(sc[i0], dc=1)
    elif kind in ("cancel_equal", "cancel_unequal"):
        d = rng.fr() or 1
        sc[i0], sc[i1] = shift(sc[i0], dc=d), shift(sc[i1], dc=-d)
        zs[i0] = zs[i1] = (rng.fr() & Z_MAX) | (1 << 127)
        if kind == "cancel_unequal":
            zs[i1] ^= 1 << 100
    elif kind in ("cancel_wide", "cancel_wide_broken"):
        z1, z2, k = Z_MAX, (1 << 127) + 1, rng.fr() or 1
        sc[i0], sc[i1] = shift(sc[i0], dc=z2 * k), shift(sc[i1], dc=-z1 * k)
        zs[i0], zs[i1] = (z1 if kind == "cancel_wide" else z1 - (1 << 64)), z2
    elif kind == "cancel_pub":
        e = rng.fr() or 1
        zs[i0], zs[i1] = (rng.fr() & Z_MAX) | (1 << 127), (rng.fr() & Z_MAX) | 1
        sc[i0], sc[i1] = shift(sc[i0], dpub=e), shift(sc[i1], dpub=-e * zs[i0] * inv(zs[i1]))
    elif kind == "cancel_a_c":
        e = rng.fr() or 1
        zs[i0], zs[i1] = (rng.fr() & Z_MAX) | (1 << 127), (rng.fr() & Z_MAX) | 1
        b1 = sc[i0][1]
        sc[i0], sc[i1] = shift(sc[i0], da=e), shift(sc[i1], dc=zs[i0] * e * b1 * inv(zs[i1] * m.delta))
    elif kind == "A_inf":
        sc[i0] = fresh(a=0)
    elif kind == "B_inf":
        sc[i0] = fresh(b=0, a=rng.fr() or 1)
    elif kind == "C_inf":
        sc[i0] = fresh(c=0)
    elif kind == "vk_x_inf":
        p2 = rng.fr()
        p1 = -(m.ics[0] + p2 * m.ics[2]) * inv(m.ics[1]) % R
        sc[i0] = fresh(pubs=[1, p1, p2])
        assert m.x(sc[i0][3]) == 0
    elif kind == "sum_zC_inf":      # the last proof's C cancels the weighted sum of all others
        rest = sum(z * s[2] for s, z in zip(sc[:-1], zs[:-1]))
        sc[-1] = fresh(c=-rest * inv(zs[-1]) % R)
        assert sum(z * s[2] for s, z in zip(sc, zs)) % R == 0
    elif kind == "sum_sIC_inf":     # the last proof's public inputs cancel the weighted sum of all x_j
        rest = sum(z * m.x(s[3]) for s, z in zip(sc[:-1], zs[:-1]))
        p2 = rng.fr()
        want = -rest * inv(zs[-1]) % R
        sc[-1] = fresh(pubs=[1, (want - m.ics[0] - p2 * m.ics[2]) * inv(m.ics[1]) % R, p2])
        assert sum(z * m.x(s[3]) for s, z in zip(sc, zs)) % R == 0
    elif kind == "same_twice":
        sc[i0] = sc[i1] = fresh(c=rng.fr() or 1)
        zs[i0] = zs[i1] = (rng.fr() & Z_MAX) | (1 << 127)
    elif kind == "opposite_C":
        c = rng.fr() or 1
        sc[i0], sc[i1] = fresh(c=c), fresh(c=R - c)
        zs[i0] = zs[i1] = (rng.fr() & Z_MAX) | (1 << 127)
    assert all(0 < z <= Z_MAX for z in zs)
    result = 1 if m.accepts(sc, zs) else 0
    assert result == EXPECTED.get(kind, 1), kind
    statuses = [1] * count if result else [1 if m.defect(*s) == 0 else 0 for s in sc]
    return Picture(m, sc, zs, result, statuses)


def structural(kind, count=5, at=2):
    """an accepted batch with one malformed proof put in: result 0, the proof's code among statuses of 1"""
    from tests import device_ops as D
    pic = picture("valid", count, seed=100 + list(STRUCTURAL).index(kind))
    pa, pb, pc = pic.proofs[at]
    off_g1 = o.fp_to_mont_bytes(5) + o.fp_to_mont_bytes(7)             # not on y^2 = x^3 + 3
    if kind == "off_curve_a":
        pa = off_g1
    elif kind == "off_curve_b":
        pb = bytes(pb[:64]) + bytes(64)
    elif kind == "off_curve_c":
        pc = off_g1
    elif kind == "small_order_b":
        pb = o.g2_to_bytes(D.twist_points()[0])
    elif kind == "noncanonical_coord":
        pa = (int.from_bytes(pa[:32], "little") + o.P).to_bytes(32, "little") + bytes(pa[32:])
    pic.proofs[at] = (pa, pb, pc)
    if kind == "noncanonical_pub":
        row = pic.public_io(True)[at * 96:(at + 1) * 96]
        bad = row[:32] + (int.from_bytes(row[32:64], "little") + R).to_bytes(32, "little") + row[64:]
        pic.pub_bytes[at] = bad                                            # Montgomery rows only
    pic.result = 0
    pic.statuses = [STRUCTURAL[kind] if j == at else 1 for j in range(count)]
    return pic


def oracle_result(pic):
    """the equation of g16_verify_batch with the oracle's Miller loop and final exponentiation on the points"""
    from tests import device_ops as D
    m, zs = pic.model, pic.multipliers
    f = o._f12_one()
    csum = o.INF_G1
    for (A, B, C), z in zip(pic.points(), zs):
        f = o._f12_mul(f, D.miller_ref(o.G1.neg(o.G1.mul(z, A)), B))
        csum = o.G1.add(csum, o.G1.mul(z, C))
    s = [sum(z * p[i] for z, p in zip(zs, pic.pubs)) % R for i in range(m.npubs + 1)]
    fixed = ((csum, m.delta2), (o.G1.msm_naive(s, m.ic), m.gamma2), (o.G1.mul(sum(zs) % R, m.alpha1), m.beta2))
    for Pt, Q in fixed:
        f = o._f12_mul(f, D.miller_ref(Pt, Q))
    return 1 if o.final_exp(list(f)) == o._f12_one() else 0
