"""Exceptional pictures for a proof's last step: the sums of the ranks' XYZZ partial records (prove_combine_kernel,
sum_partials_kernel) and the host mask algebra behind them (csrc/host_curve.hpp over csrc/host_ff64.hpp).

Pure Python: no GPU, no ctypes.  Everything lives in log space: a point is k * G with a chosen k, a record slot is a list
of such logs (one per rank), and the proof of a picture is

    pi_a = (alpha + r delta + sum a) G1
    pi_b = (beta + s delta + sum b2) G2
    pi_c = (s alpha + r beta + r s delta + s sum a + r sum b1 + sum h + sum c) G1       (mod r; 0 -> all-zero bytes)

computed on integers (`expected_logs`) -- never anything the code under test produced.  `walk_list` and `walk_combine`
replay the additions of the kernels and of the host algebra on the logs only to show that a picture reaches the branch it
is named for (tests/test_host_algebra_cpu.py asserts that); tests/test_gpu_combine_edges.py runs the pictures on the
GPU.  H and C enter pi_c symmetrically: an exchange of those two slots cannot show and is not claimed.
"""
from collections import Counter, defaultdict

from oracle import bn254_ref as o

R, P = o.R, o.P

# the toxic waste of the toy key (alpha, beta, gamma, delta, tau)
_g = o.SplitMix64(5)
TOXIC = tuple(_g.fr() for _ in range(5))
ALPHA, BETA, GAMMA, DELTA, TAU = TOXIC

# the 768-byte record: XYZZ accumulators (Montgomery), fixed order
SLOTS = ("a", "b1", "b2", "h", "c")
SLOT_GROUP = {"a": 1, "b1": 1, "b2": 2, "h": 1, "c": 1}
SLOT_OFF = {"a": 0, "b1": 128, "b2": 256, "h": 512, "c": 640}
RECORD_BYTES = 768
COMBINE_COUNTS = (1, 2, 3, 8, 64, 1024)          # 1024: the ABI's maximum
SUM_COUNTS = (0, 1, 2, 3, 4096)                  # 4096: the ABI's maximum

ALL3 = (1 << 252) - 1                            # every 2-bit window below bit 252 is 3: the largest such value below r
TOP_F = (2 << 252) | ALL3                        # 0x2FF..F: the largest value below r whose lower 63 nibbles are all 0xF
EDGE_MASKS = (1, 2, 3, R - 1, R - 2, 1 << 253, ALL3)
assert TOP_F < R < TOP_F + (1 << 252) and (1 << 253) < R


def _inv(x):
    return pow(x % R, -1, R)


def kind(a, b):
    """what an addition of the points a G and b G meets"""
    a, b = a % R, b % R
    return ("empty" if a == 0 and b == 0 else "inf" if a == 0 or b == 0 else "equal" if a == b
            else "opposite" if (a + b) % R == 0 else "generic")


# ---- list pictures --------------------------------------------------------------------------------------------------
def _tail(k, m, lo, n):
    """unrelated entries for the positions lo .. n-1 (the same value at the same position in every picture)"""
    return [(k + (i + 1) * m) % R for i in range(lo, n)]


def _head(head):
    def build(n, k, m):
        h = head(k, m)
        return None if n < len(h) else [x % R for x in h] + _tail(k, m, len(h), n)
    return build


def _inf_at(where):
    def build(n, k, m):
        if n < (3 if where == "middle" else 2):
            return None
        out = _tail(k, m, 0, n)
        out[{"first": 0, "middle": n // 2, "last": n - 1}[where]] = 0
        return out
    return build


def _alternating(n, k, m):
    return None if n < 2 else [k if i % 2 == 0 else R - k for i in range(n)]


# name -> (build(count, k, m) -> the logs of one slot's records in rank order, or None where the count is too small,
#          the kinds the running sum must meet)
LIST_PICTURES = {
    "all_infinity": (lambda n, k, m: [0] * n, ()),
    "infinity_first": (_inf_at("first"), ("empty", "inf")),
    "infinity_middle": (_inf_at("middle"), ("inf", "generic")),
    "infinity_last": (_inf_at("last"), ("inf",)),
    "k_k": (_head(lambda k, m: [k, k]), ("equal",)),                               # the doubling branch of the XYZZ add
    "k_-k_m": (_head(lambda k, m: [k, -k]), ("opposite",)),                        # back to infinity, and on from there
    "k_k_-2k": (_head(lambda k, m: [k, k, -2 * k]), ("equal", "opposite")),
    "k_m_-(k+m)": (_head(lambda k, m: [k, m, -(k + m)]), ("generic", "opposite")),
    "same_record": (lambda n, k, m: [k] * n, ()),
    "alternating": (_alternating, ("opposite",)),
    "k_2k_3k": (lambda n, k, m: [(i + 1) * k % R for i in range(n)], ()),          # 3k + 3k: a doubling at the third
}


def list_pictures(n):
    """[(name, build)] of the pictures that exist at `n` records"""
    return [(name, b) for name, (b, _) in LIST_PICTURES.items() if b(n, 1, 2) is not None]


def slot_seeds(slot):
    """(k, m) of a slot: independent of the other slots', so that a slot or offset mix-up shows (b1 and b2 differ)"""
    g = o.SplitMix64(0x5107 + SLOTS.index(slot))
    return g.fr(), g.fr()


def walk_list(logs):
    """the running sum of a kernel over one slot: (Counter of the kinds its additions meet, the sum)"""
    seen, acc = Counter(), 0
    for x in logs:
        seen[kind(acc, x)] += 1
        acc = (acc + x) % R
    return seen, acc


def record_logs(n, names):
    """{slot: logs} of `n` records whose slots follow the list pictures `names` (one name, or one per slot)"""
    if isinstance(names, str):
        names = (names,) * 5
    return {slot: LIST_PICTURES[name][0](n, *slot_seeds(slot)) for slot, name in zip(SLOTS, names)}


def mixed_names(n, shift):
    """one list picture per slot, rotated through the ones that exist at n records"""
    have = [name for name, _ in list_pictures(n)]
    return tuple(have[(shift + 2 * i) % len(have)] for i in range(5))


# ---- XYZZ records ---------------------------------------------------------------------------------------------------
LAMBDA_MODES = ("unit", "random", "edge")
_EDGE_L1 = (1, P - 1, 2)
_EDGE_L2 = ((1, 0), (P - 1, 0), (2, 0), (0, 1))


def lam_of(mode, group, index):
    """the scaling of record `index`: lambda in Fp (G1) or Fp2 (G2), never zero"""
    if mode == "unit":
        return 1 if group == 1 else (1, 0)
    if mode == "edge":
        return _EDGE_L1[index % 3] if group == 1 else _EDGE_L2[index % 4]
    g = o.SplitMix64(0x1a3b + 977 * index + group)
    return 1 + g.fr() % (P - 1) if group == 1 else (1 + g.fr() % (P - 1), g.fr() % P)


def xyzz_bytes(group, aff, lam):
    """the XYZZ form (x l^2, y l^3, l^2, l^3) of an affine point (integers; (0,0) = infinity -> all zero), Montgomery"""
    f = o.fp_to_mont_bytes
    if group == 1:
        if aff == o.INF_G1:
            return bytes(128)
        zz = lam * lam % P
        zzz = zz * lam % P
        return f(aff[0] * zz) + f(aff[1] * zzz) + f(zz) + f(zzz)
    if aff == o.INF_G2:
        return bytes(256)
    zz = o.fp2_sqr(lam)
    zzz = o.fp2_mul(zz, lam)
    return b"".join(f(c) for e in (o.fp2_mul(aff[0], zz), o.fp2_mul(aff[1], zzz), zz, zzz) for c in e)


def build_records(slot_logs, mode, point):
    """{slot: logs} -> the records' bytes; point(group, log) -> affine integers; every slot of every record its own
    scaling"""
    n = len(slot_logs["a"])
    out = bytearray(RECORD_BYTES * n)
    for j, slot in enumerate(SLOTS):
        g, off, size = SLOT_GROUP[slot], SLOT_OFF[slot], 128 * SLOT_GROUP[slot]
        for i, k in enumerate(slot_logs[slot]):
            if k:
                out[RECORD_BYTES * i + off: RECORD_BYTES * i + off + size] = xyzz_bytes(g, point(g, k), lam_of(mode, g, 5 * i + j))
    return bytes(out)


# ---- the closed form ------------------------------------------------------------------------------------------------
def pre_logs(r, s):
    return (ALPHA + r * DELTA) % R, (BETA + s * DELTA) % R, (s * ALPHA + r * BETA + r * s % R * DELTA) % R


def expected_logs(r, s, a, b1, b2, h, c):
    """(log pi_a, log pi_b, log pi_c) for the mask (r, s) and the five sums"""
    return ((ALPHA + r * DELTA + a) % R, (BETA + s * DELTA + b2) % R,
            (s * ALPHA + r * BETA + r * s % R * DELTA + s * a + r * b1 + h + c) % R)


# ---- mask and point pictures ----------------------------------------------------------------------------------------
class MaskPicture:
    """name; mask r, s; the five sums; reach: the (cell, kind) pairs `walk_combine` must report"""

    def __init__(self, name, r, s, sums, reach=()):
        self.name, self.r, self.s = name, r % R, s % R
        self.sums = tuple(x % R for x in sums)
        self.reach = tuple(reach)

    def expected(self):
        return expected_logs(self.r, self.s, *self.sums)


_g = o.SplitMix64(0xC0DE)
R0, S0, A0, B10, B20, H0, C0 = (_g.fr() for _ in range(7))
GENERIC_SUMS = (A0, B10, B20, H0, C0)


def _edge_name(v):
    return {R - 1: "r-1", R - 2: "r-2", 1 << 253: "2^253", ALL3: "all3"}.get(v, str(v))


def mask_pictures(sums=None):
    """Every mask and point picture.  With `sums` given (the MSM sums of a real witness, which a test cannot choose)
    only the pictures that leave the sums alone, and those that can be reached by solving for the mask instead."""
    fixed = sums is not None
    a, b1, b2, h, c = sums = tuple(x % R for x in (sums if fixed else GENERIC_SUMS))
    M = MaskPicture
    out = [
        M("r=s=0", 0, 0, sums, [("r_delta.loop", "none"), ("a_pre", "inf"), ("b_pre", "inf"), ("c_pre", "empty")]),
        M("r=0", 0, S0, sums, [("a_pre", "inf"), ("rs_delta.loop", "none")]),
        M("s=0", R0, 0, sums, [("b_pre", "inf"), ("rs_delta.loop", "none")]),
        M("r=s", R0, R0, sums, [("fin.mul2.loop", "generic")]),
        M("s=1/r", R0, _inv(R0), sums, [("c_pre", "generic")]),
        M("a_pre=inf", -ALPHA * _inv(DELTA), S0, sums, [("a_pre", "opposite"), ("pi_a", "inf")]),
        M("b_pre=inf", R0, -BETA * _inv(DELTA), sums, [("b_pre", "opposite"), ("pi_b", "inf")]),
        M("c_pre=inf", R0, -R0 * BETA * _inv(ALPHA + R0 * DELTA), sums, [("c_pre", "opposite"), ("pi_c.t", "inf")]),
    ]
    for i, v in enumerate(EDGE_MASKS):
        w = EDGE_MASKS[(i + 3) % len(EDGE_MASKS)]
        out += [M(f"r={_edge_name(v)}", v, S0, sums), M(f"s={_edge_name(v)}", R0, v, sums),
                M(f"r={_edge_name(v)},s={_edge_name(w)}", v, w, sums)]
    r, s = R0, S0
    ap, bp, cp = pre_logs(r, s)
    if fixed:      # the sums are what they are: solve for the mask
        t = _inv(ALPHA + a)                                            # pi_c = s (alpha + r delta + a) + r (beta + b1) + h + c
        r_inf, r_dbl = -(ALPHA + a) * _inv(DELTA), (a - ALPHA) * _inv(DELTA)
        s_inf, s_dbl = -(BETA + b2) * _inv(DELTA), (b2 - BETA) * _inv(DELTA)
        out += [
            M("pi_a=inf", r_inf, S0, sums, [("pi_a", "opposite")]),
            M("pi_a.doubling", r_dbl, S0, sums, [("pi_a", "equal")]),
            M("pi_b=inf", R0, s_inf, sums, [("pi_b", "opposite")]),
            M("pi_b.doubling", R0, s_dbl, sums, [("pi_b", "equal")]),
            M("pi_c=inf", R0, -(R0 * (BETA + b1) + h + c) * _inv(ALPHA + R0 * DELTA + a), sums),
            M("pi_c=inf,r=0", 0, -(h + c) * t, sums),
        ]
        return out
    t0 = (s * a + r * b1) % R                                          # the joint multiplication of the finish half
    out += [
        M("pi_a=inf", r, s, (-ap, b1, b2, h, c), [("pi_a", "opposite")]),
        M("pi_a.doubling", r, s, (ap, b1, b2, h, c), [("pi_a", "equal")]),
        M("a=0", r, s, (0, b1, b2, h, c), [("pi_a", "inf"), ("fin.mul2.tab", "inf")]),
        M("pi_b=inf", r, s, (a, b1, -bp, h, c), [("pi_b", "opposite")]),
        M("pi_b.doubling", r, s, (a, b1, bp, h, c), [("pi_b", "equal")]),
        M("b2=0", r, s, (a, b1, 0, h, c), [("pi_b", "inf")]),
        # the table i a + j b1 of the joint multiplication through infinity and through a doubling
        M("b1=a", r, s, (a, a, b2, h, c), [("fin.mul2.tab", "equal")]),
        M("b1=-a", r, s, (a, -a, b2, h, c), [("fin.mul2.tab", "opposite"), ("fin.mul2.tab", "inf")]),
        M("b1=2a", r, s, (a, 2 * a, b2, h, c), [("fin.mul2.tab", "equal")]),
        M("b1=0", r, s, (a, 0, b2, h, c), [("fin.mul2.tab", "empty"), ("fin.mul2.tab", "inf")]),
        M("a=0,b1!=0", r, s, (0, b1, b2, h, c), [("fin.mul2.tab", "inf")]),
        M("b1=-a,r=s", r, r, (a, -a, b2, h, c), [("fin.mul2.loop", "empty"), ("pi_c.t", "inf")]),
        M("b1=a,r=-s", r, -r, (a, a, b2, h, c), [("pi_c.t", "inf")]),
        # c_pre + (s A + r B1)
        M("t=-c_pre", r, s, ((-cp - r * b1) * _inv(s), b1, b2, h, c), [("pi_c.t", "opposite"), ("pi_c.h", "inf")]),
        M("t=c_pre", r, s, ((cp - r * b1) * _inv(s), b1, b2, h, c), [("pi_c.t", "equal")]),
        # the last two additions of pi_c
        M("h=-before", r, s, (a, b1, b2, -(cp + t0), c), [("pi_c.h", "opposite"), ("pi_c.c", "inf")]),
        M("h=before", r, s, (a, b1, b2, cp + t0, c), [("pi_c.h", "equal")]),
        M("c=running", r, s, (a, b1, b2, h, cp + t0 + h), [("pi_c.c", "equal")]),
        M("c=-running", r, s, (a, b1, b2, h, -(cp + t0 + h)), [("pi_c.c", "opposite")]),
        M("h=c=0", r, s, (a, b1, b2, 0, 0), [("pi_c.h", "inf"), ("pi_c.c", "inf")]),
        M("h=-c", r, s, (a, b1, b2, h, -h), []),
        M("all_zero,r=s=0", 0, 0, (0, 0, 0, 0, 0), [("pi_a", "inf"), ("pi_b", "inf"), ("pi_c.t", "empty"),
                                                     ("pi_c.h", "empty"), ("pi_c.c", "empty")]),
        M("all_zero", r, s, (0, 0, 0, 0, 0), [("fin.mul2.loop", "empty")]),
    ]
    return out


# ---- the log-space walk of the host algebra -------------------------------------------------------------------------
def walk_combine(r, s, sums):
    """The additions of host_combine_pre and host_combine_finish (csrc/host_curve.hpp) on logs, in the order and
    grouping of the code: host_mul (table of 16 by mixed additions, 4-bit windows from the top), host_mul2 (table
    i p1 + j p2 by mixed additions, 2-bit joint windows), host_add.  -> ({cell: Counter(kind)}, (pi_a, pi_b, pi_c)).
    Cells: <name>.tab / <name>.loop for the multiplications r_delta, s_delta2, rs_delta, pre.mul2, fin.mul2 (a loop
    that adds nothing reports "none"), and a_pre b_pre c_pre pi_a pi_b pi_c.t pi_c.h pi_c.c for the additions.  It
    exists only to show what a picture reaches; no expected value comes from it."""
    t = defaultdict(Counter)

    def add(cell, x, y):
        t[cell][kind(x, y)] += 1
        return (x + y) % R

    def mul(cell, k, x):
        tab = [0, x % R]
        for _ in range(2, 16):
            tab.append(add(cell + ".tab", tab[-1], x))
        acc, used = 0, False
        for nib in range(63, -1, -1):
            acc = 16 * acc % R
            w = (k >> (4 * nib)) & 15
            if w:
                acc, used = add(cell + ".loop", acc, tab[w]), True
        if not used:
            t[cell + ".loop"]["none"] += 1
        return acc

    def mul2(cell, k1, x1, k2, x2):
        tab = [0] * 16
        for j in range(1, 4):
            tab[j] = add(cell + ".tab", tab[j - 1], x2)
        for i in range(1, 4):
            for j in range(4):
                tab[4 * i + j] = add(cell + ".tab", tab[4 * (i - 1) + j], x1)
        acc, used = 0, False
        for pos in range(127, -1, -1):
            acc = 4 * acc % R
            w = 4 * ((k1 >> (2 * pos)) & 3) + ((k2 >> (2 * pos)) & 3)
            if w:
                acc, used = add(cell + ".loop", acc, tab[w]), True
        if not used:
            t[cell + ".loop"]["none"] += 1
        return acc

    a, b1, b2, h, c = sums
    a_pre = add("a_pre", ALPHA, mul("r_delta", r, DELTA))
    b_pre = add("b_pre", BETA, mul("s_delta2", s, DELTA))
    c_pre = add("c_pre", mul2("pre.mul2", s, ALPHA, r, BETA), mul("rs_delta", r * s % R, DELTA))
    pi_a = add("pi_a", a_pre, a)
    pi_b = add("pi_b", b_pre, b2)
    pi_c = add("pi_c.t", c_pre, mul2("fin.mul2", s, a, r, b1))
    pi_c = add("pi_c.h", pi_c, h)
    pi_c = add("pi_c.c", pi_c, c)
    return t, (pi_a, pi_b, pi_c)


# ---- the toy circuit ------------------------------------------------------------------------------------------------
def toy_sum_logs(flavour=o.SNARKJS):
    """The logs of the five MSM sums A, B1, B2, H, C of the reference's toy witness under TOXIC, from the oracle's setup
    and prover run on integers: fake_circuit_setup with `k -> k` in place of `k -> k G` leaves the logs of every key
    point, and the sums are the prover's five MSMs (oracle/bn254_ref.py: generate_proof_with_mask) over them."""
    ident = lambda ks: [k % R for k in ks]                                          # noqa: E731
    zk = o.fake_circuit_setup(o.toy_r1cs(), o.ToxicWaste(*TOXIC), flavour, ident, ident)
    assert (zk.alpha1, zk.beta1, zk.delta1, zk.beta2, zk.delta2) == (ALPHA, BETA, DELTA, BETA, DELTA)
    wit = o.TOY_WITNESS
    Az, Bz, Cz = o.build_abc(zk.coeffs, zk.domainSize, wit)
    qs = o.compute_snarkjs_scalar_coeffs(Az, Bz, Cz) if flavour == o.SNARKJS else o.compute_quotient_pointwise(Az, Bz, Cz)
    dot = lambda cs, ks: sum(x * k for x, k in zip(cs, ks)) % R                     # noqa: E731
    return (dot(wit, zk.pointsA1), dot(wit, zk.pointsB1), dot(wit, zk.pointsB2), dot(qs, zk.pointsH1),
            dot(wit[zk.npubs + 1:], zk.pointsC1))
