"""Keys and point arrays with planted defects for the key audit (g16_points_audit_g1/g2, g16_points_pairs_check,
g16_key_audit), and the integer model of what the audit must report.  The model reads the same BYTES the library gets
and owes nothing to the code under test: a limb pattern is canonical iff its integer is < p; a point is on its curve by
the oracle's equation; a twist point is in the subgroup iff o.G2.mul(R, Q) is infinity; a relation holds iff the
oracle's pairing of the two sums says so.

An element counts under the FIRST check it fails (canonical, curve, subgroup) and only there.

    array_pictures()     -> [ArrayPicture]: a group, the bytes of an array, expected (first_bad, bad_count)
    relation_pictures()  -> [RelationPicture]: a G1 array, a G2 array, multipliers, the expected verdict
    key_pictures()       -> {name: KeyPicture}: a toy key with one planted defect each, the expected report"""
import copy
import functools
from dataclasses import dataclass, field
from typing import List, Optional

from oracle import bn254_ref as o

R, P = o.R, o.P
SECTIONS = ("alpha1", "beta1", "delta1", "beta2", "gamma2", "delta2", "pointsIC", "pointsA1", "pointsB1", "pointsB2",
            "pointsC1", "pointsH1", "coeffs")
GROUP = {"alpha1": 1, "beta1": 1, "delta1": 1, "beta2": 2, "gamma2": 2, "delta2": 2, "pointsIC": 1, "pointsA1": 1,
         "pointsB1": 1, "pointsB2": 2, "pointsC1": 1, "pointsH1": 1}
CANONICAL, CURVE, SUBGROUP, RELATION, SPEC_INFINITY = 1, 2, 4, 8, 16
SIZES = (1, 63, 64, 65, 255, 256, 257, 301)
Z_MAX = (1 << 128) - 1


# ---- honest points: multiples of the generators by repeated addition ---------------------------------------------
@functools.lru_cache(None)
def honest(group, n):
    """[1 G, 2 G, ..., n G]"""
    C, G = (o.G1, o.GEN1) if group == 1 else (o.G2, o.GEN2)
    out, acc = [], (o.INF_G1 if group == 1 else o.INF_G2)
    for _ in range(n):
        acc = C.add(acc, G)
        out.append(acc)
    return tuple(out)


def enc(group, pt) -> bytes:
    return o.g1_to_bytes(pt) if group == 1 else o.g2_to_bytes(pt)


def coords(group, b: bytes) -> List[int]:
    """the stored limb patterns as integers: 2 (G1) or 4 (G2: x.c0, x.c1, y.c0, y.c1)"""
    return [int.from_bytes(b[k:k + 32], "little") for k in range(0, 64 * group, 32)]


def raise_by_p(group, b: bytes, which: int) -> bytes:
    """a non-canonical alias: coordinate `which` stored as its residue + p (fits: 2p < 2^256)"""
    c = coords(group, b)
    c[which] += P
    assert c[which] < 1 << 256
    return b"".join(x.to_bytes(32, "little") for x in c)


def off_curve(group) -> bytes:
    pt = (5, 7) if group == 1 else ((5, 1), (7, 2))
    assert not (o.G1 if group == 1 else o.G2).is_on_curve(pt)
    return enc(group, pt)


@functools.lru_cache(None)
def twist_outsiders():
    """twist points outside the order-r subgroup: order 10069, the first full twist point, small + G, [r] full"""
    from tests import device_ops as D
    small, full = D.twist_points()
    mixed = o.G2.add(small, o.G2.mul(77, o.GEN2))
    rfull = o.G2.mul(R, full)
    assert not o.G2.is_inf(rfull)
    return {"small": small, "full": full, "small_plus_g": mixed, "r_full": rfull}


# ---- the model of one element -------------------------------------------------------------------------------------
@functools.lru_cache(None)
def element_verdict(group, b: bytes) -> Optional[int]:
    """None = passes, else the index of the one check the element is counted under"""
    if any(c >= P for c in coords(group, b)):
        return 0
    pt = o.g1_from_bytes(b) if group == 1 else o.g2_from_bytes(b)
    C = o.G1 if group == 1 else o.G2
    if C.is_inf(pt):
        return None
    if not C.is_on_curve(pt):
        return 1
    if group == 2 and not o.G2.is_inf(o.G2.mul(R, pt)):
        return 2
    return None


def array_model(group, raw: bytes):
    psz = 64 * group
    first, count = [None] * 3, [0] * 3
    for i in range(len(raw) // psz):
        v = element_verdict(group, raw[i * psz:(i + 1) * psz])
        if v is not None:
            count[v] += 1
            first[v] = i if first[v] is None else first[v]
    return first, count


def coeff_model(values: List[bytes]):
    """only the canonical check: the 32-byte integer is < r"""
    bad = [i for i, v in enumerate(values) if int.from_bytes(v, "little") >= R]
    return [bad[0] if bad else None, None, None], [len(bad), 0, 0]


@functools.lru_cache(None)
def relation_model(S1, S2) -> int:
    """e(S1, gen2) * e(-gen1, S2) == 1 by the oracle's pairing"""
    f = o._f12_mul(o.miller_loop(S1, o.GEN2), o.miller_loop(o.G1.neg(o.GEN1), S2))
    return 1 if o.final_exp(f) == o._f12_one() else 0


# ---- arrays ---------------------------------------------------------------------------------------------------------
@dataclass
class ArrayPicture:
    name: str
    group: int
    raw: bytes
    first_bad: list
    bad_count: list


def defects(group):
    """name -> (bytes of the planted element, the check it must be counted under or None)"""
    hon = honest(group, 9)
    good = enc(group, hon[4])
    d = {"inf": (bytes(64 * group), None), "off_curve": (off_curve(group), 1)}
    for k in range(2 * group):                       # each coordinate; each half of an Fp2
        d[f"alias_{k}"] = (raise_by_p(group, good, k), 0)
    # a coordinate equal to exactly p: the alias of zero.  x = 0 has no point on either curve, so put it into a point
    # that is off the curve as well: counted once, as not canonical
    zero_x = b"".join(x.to_bytes(32, "little") for x in [P] + coords(group, good)[1:])
    d["coord_is_p"] = (zero_x, 0)
    d["alias_of_off_curve"] = (raise_by_p(group, off_curve(group), 2 * group - 1), 0)       # precedence: two defects
    if group == 2:
        for name, pt in twist_outsiders().items():
            d[name] = (o.g2_to_bytes(pt), 2)
        d["alias_of_small"] = (raise_by_p(2, o.g2_to_bytes(twist_outsiders()["small"]), 1), 0)   # precedence again
        d["neg_honest"] = (enc(2, o.G2.neg(hon[2])), None)
    for name, (b, want) in d.items():
        assert element_verdict(group, b) == want, (group, name)
    return d


def positions(n):
    """0, n - 1, both sides of every workgroup / wave boundary inside the array, and two in one wave"""
    pos = {0, n - 1}
    for edge in (64, 128, 256):
        pos |= {p for p in (edge - 1, edge, edge + 1) if 0 <= p < n}
    if n > 12:
        pos |= {7, 9}                               # one wave: a good lane between two bad ones
    return sorted(pos)


@functools.lru_cache(None)
def array_pictures():
    pics = []
    for group in (1, 2):
        d = defects(group)
        names = sorted(d)
        for n in SIZES:
            hon = [enc(group, pt) for pt in honest(group, n)]
            pics.append(ArrayPicture(f"g{group}_clean_{n}", group, b"".join(hon), [None] * 3, [0] * 3))
            arr = list(hon)
            for j, p_ in enumerate(positions(n)):   # every defect kind in turn, cycled over the positions
                arr[p_] = d[names[(j + n) % len(names)]][0]
            raw = b"".join(arr)
            pics.append(ArrayPicture(f"g{group}_mixed_{n}", group, raw, *array_model(group, raw)))
        # each kind alone, at a wave-interior lane of a two-workgroup array
        hon = [enc(group, pt) for pt in honest(group, 257)]
        for name in names:
            for at in ((3,), (255, 256)):
                arr = list(hon)
                for p_ in at:
                    arr[p_] = d[name][0]
                raw = b"".join(arr)
                want = d[name][1]
                first, count = array_model(group, raw)
                assert count == [len(at) if k == want else 0 for k in range(3)], name
                pics.append(ArrayPicture(f"g{group}_{name}_at_{'_'.join(map(str, at))}", group, raw, first, count))
    pics.append(ArrayPicture("g1_empty", 1, b"", [None] * 3, [0] * 3))
    pics.append(ArrayPicture("g2_empty", 2, b"", [None] * 3, [0] * 3))
    return tuple(pics)


# ---- relations between a G1 and a G2 array --------------------------------------------------------------------------
@dataclass
class RelationPicture:
    name: str
    a: List[int]                      # P_i = a_i gen1
    b: List[int]                      # Q_i = b_i gen2
    multipliers: List[int]
    result: int = field(default=None)

    def __post_init__(self):
        assert all(0 < z <= Z_MAX for z in self.multipliers)
        s1 = sum(z * k for z, k in zip(self.multipliers, self.a)) % R
        s2 = sum(z * k for z, k in zip(self.multipliers, self.b)) % R
        self.result = relation_model(o.G1.mul(s1, o.GEN1), o.G2.mul(s2, o.GEN2))

    @property
    def g1(self) -> bytes:
        return b"".join(o.g1_to_bytes(_g1(k)) for k in self.a)

    @property
    def g2(self) -> bytes:
        return b"".join(o.g2_to_bytes(_g2(k)) for k in self.b)


@functools.lru_cache(None)
def _g1(k):
    return o.G1.mul(k % R, o.GEN1)


@functools.lru_cache(None)
def _g2(k):
    return o.G2.mul(k % R, o.GEN2)


RELATION_KINDS = {"clean": 1, "swapped": 0, "cancel_bit127": 0, "cancel_equal_z": 1, "cancel_weighted": 1, "b1_inf": 0,
                  "both_inf": 1, "one_off": 0}


def relation_logs(kind, n, i, j, seed=0):
    """(a, b, multipliers) of one relation picture over n pairs; i, j: where the defect sits"""
    rng = o.SplitMix64(4000 + seed)
    ks = [rng.fr() or 1 for _ in range(n)]
    a, b = list(ks), list(ks)
    zs = [(rng.fr() & Z_MAX) or 1 for _ in range(n)]
    e = rng.fr() or 1
    if kind == "swapped":
        a[i], a[j] = a[j], a[i]
    elif kind in ("cancel_bit127", "cancel_equal_z"):            # +E at i, -E at j
        a[i], a[j] = (a[i] + e) % R, (a[j] - e) % R
        zs[i] = zs[j] = (rng.fr() & Z_MAX) | 1
        if kind == "cancel_bit127":
            zs[j] ^= 1 << 127                                    # the two differ only in the top bit
    elif kind == "cancel_weighted":                              # a E at i, -b E at j with z_i a = z_j b (mod r)
        wa = rng.fr() or 1
        wb = zs[i] * wa * pow(zs[j], -1, R) % R
        a[i], a[j] = (a[i] + wa * e) % R, (a[j] - wb * e) % R
    elif kind == "b1_inf":
        a[i] = 0
    elif kind == "both_inf":
        a[i] = b[i] = 0
    elif kind == "one_off":
        a[i] = (a[i] + 1) % R
    return a, b, zs


@functools.lru_cache(None)
def relation_pictures():
    pics = []
    for n, i, j in ((2, 0, 1), (65, 63, 64), (301, 255, 256)):
        for kind, want in RELATION_KINDS.items():
            a, b, zs = relation_logs(kind, n, i, j, seed=n)
            pic = RelationPicture(f"{kind}_{n}", a, b, zs)
            assert pic.result == want, (kind, n)
            pics.append(pic)
    pics.append(RelationPicture("single", [5], [5], [Z_MAX]))
    pics.append(RelationPicture("single_wrong", [5], [6], [1 << 127]))
    assert [p.result for p in pics[-2:]] == [1, 0]
    return tuple(pics)


# ---- whole keys -------------------------------------------------------------------------------------------------------
@dataclass
class Key:
    """a proving key as bytes per section; coefficient values in the form the library is handed (Montgomery limbs of a
    g16_coeff, or the doubly-Montgomery integer of a .zkey's section 4)"""
    nvars: int
    npubs: int
    log2_domain: int
    sections: dict                    # name -> bytes (all but "coeffs")
    coeffs: list                      # (matrix, row, col, 32 value bytes)
    logs_b: list = None               # pointsB1[i] = pointsB2[i] = logs_b[i] times the generators, where known

    def section4(self) -> bytes:
        out = len(self.coeffs).to_bytes(4, "little")
        for m, r_, c, v in self.coeffs:
            out += m.to_bytes(4, "little") + r_.to_bytes(4, "little") + c.to_bytes(4, "little") + v
        return out


@dataclass
class KeyPicture:
    name: str
    key: Key
    multipliers: Optional[List[int]]
    raw_coeffs: bool = False          # hand the coefficients over as section 4
    with_vk: bool = True
    report: dict = None


@functools.lru_cache(None)
def _toy_key():
    rng = o.SplitMix64(77)
    tw = o.ToxicWaste(*[rng.fr() or 1 for _ in range(5)])
    zk = o.fake_circuit_setup(o.toy_r1cs(), tw, o.SNARKJS)
    sec = {"alpha1": o.g1_to_bytes(zk.alpha1), "beta1": o.g1_to_bytes(zk.beta1), "delta1": o.g1_to_bytes(zk.delta1),
           "beta2": o.g2_to_bytes(zk.beta2), "gamma2": o.g2_to_bytes(zk.gamma2), "delta2": o.g2_to_bytes(zk.delta2)}
    for name in ("pointsIC", "pointsA1", "pointsB1", "pointsC1", "pointsH1"):
        sec[name] = b"".join(o.g1_to_bytes(q) for q in getattr(zk, name))
    sec["pointsB2"] = b"".join(o.g2_to_bytes(q) for q in zk.pointsB2)
    coeffs = [(m, r_, c, o.fr_to_mont_bytes(v)) for m, r_, c, v in zk.coeffs]
    return Key(zk.nvars, zk.npubs, zk.logDomainSize, sec, coeffs), zk


def toy_key() -> Key:
    return copy.deepcopy(_toy_key()[0])


def toy_zkey():
    """the oracle's ZKey the toy key was taken from"""
    return _toy_key()[1]


def key_model(pic: KeyPicture) -> dict:
    key = pic.key
    first, count = [], []
    for name in SECTIONS[:-1]:
        raw = key.sections[name]
        if not pic.with_vk and name in ("gamma2", "pointsIC"):
            raw = b""
        f, c = array_model(GROUP[name], raw)
        first.append(f)
        count.append(c)
    f, c = coeff_model([v for _, _, _, v in key.coeffs])
    first.append(f)
    count.append(c)
    failed = 0
    for c in count:
        for k in range(3):
            if c[k]:
                failed |= (CANONICAL, CURVE, SUBGROUP)[k]
    spec_inf = 0
    for s, name in enumerate(SECTIONS[:6]):
        if (pic.with_vk or name != "gamma2") and key.sections[name] == bytes(64 * GROUP[name]):
            spec_inf |= 1 << s
    if spec_inf:
        failed |= SPEC_INFINITY
    clean = lambda name: count[SECTIONS.index(name)] == [0, 0, 0]       # noqa: E731
    rel = [-1, -1, -1]
    if pic.multipliers is not None and clean("pointsB1") and clean("pointsB2"):
        b1 = [o.g1_from_bytes(key.sections["pointsB1"][k:k + 64]) for k in range(0, 64 * key.nvars, 64)]
        b2 = [o.g2_from_bytes(key.sections["pointsB2"][k:k + 128]) for k in range(0, 128 * key.nvars, 128)]
        rel[0] = relation_model(o.G1.msm_naive(pic.multipliers, b1), o.G2.msm_naive(pic.multipliers, b2))
    for k, (n1, n2) in ((1, ("beta1", "beta2")), (2, ("delta1", "delta2"))):
        if clean(n1) and clean(n2):
            rel[k] = relation_model(o.g1_from_bytes(key.sections[n1]), o.g2_from_bytes(key.sections[n2]))
    if 0 in rel:
        failed |= RELATION
    return {"failed": failed, "spec_infinity": spec_inf, "relation": rel, "first_bad": first, "bad_count": count}


def _set(raw: bytes, psz: int, i: int, elem: bytes) -> bytes:
    return raw[:i * psz] + elem + raw[(i + 1) * psz:]


def _get(raw: bytes, psz: int, i: int) -> bytes:
    return raw[i * psz:(i + 1) * psz]


@functools.lru_cache(None)
def key_pictures():
    pics = {}
    d1, d2 = defects(1), defects(2)
    zs = [Z_MAX, 1 << 127, 3, (1 << 64) + 1, 0x1234567890abcdef1234567890abcdef, 1, (1 << 127) + 1, 7]

    def add(name, edit=None, multipliers=zs, **kw):
        key = toy_key()
        assert len(multipliers or zs) == key.nvars
        if edit:
            edit(key)
        pic = KeyPicture(name, key, multipliers, **kw)
        pic.report = key_model(pic)
        pics[name] = pic
        return pic

    def plant(section, i, elem):
        def edit(key):
            key.sections[section] = _set(key.sections[section], 64 * GROUP[section], i, elem)
        return edit

    assert add("clean").report["failed"] == 0
    add("clean_no_multipliers", multipliers=None)
    add("clean_no_vk", with_vk=False)
    add("clean_section4", raw_coeffs=True)
    # element defects, one per section kind and check
    add("a1_alias", plant("pointsA1", 7, d1["alias_1"][0]))
    add("h1_off_curve", plant("pointsH1", 0, d1["off_curve"][0]))
    add("c1_coord_is_p", plant("pointsC1", 2, d1["coord_is_p"][0]))
    add("ic_off_curve", plant("pointsIC", 1, d1["off_curve"][0]))
    add("ic_off_curve_no_vk", plant("pointsIC", 1, d1["off_curve"][0]), with_vk=False)
    add("b2_small_order", plant("pointsB2", 3, d2["small"][0]))
    add("b2_full_twist", plant("pointsB2", 7, d2["full"][0]))
    add("b2_small_plus_g", plant("pointsB2", 0, d2["small_plus_g"][0]))
    add("b2_alias_c1", plant("pointsB2", 4, d2["alias_1"][0]))
    add("b2_alias_of_small", plant("pointsB2", 4, d2["alias_of_small"][0]))
    add("b1_alias_of_off_curve", plant("pointsB1", 5, d1["alias_of_off_curve"][0]))
    add("gamma2_small_order", plant("gamma2", 0, d2["small"][0]))
    add("beta2_off_curve", plant("beta2", 0, d2["off_curve"][0]))
    add("alpha1_alias", plant("alpha1", 0, d1["alias_0"][0]))

    def two(key):                                    # two sections at once, two elements in one of them
        plant("pointsA1", 0, d1["off_curve"][0])(key)
        plant("pointsA1", 6, d1["off_curve"][0])(key)
        plant("pointsB2", 2, d2["r_full"][0])(key)
    add("two_sections", two)

    # coefficients, both forms
    def coeff(i, value):
        def edit(key):
            m, r_, c, _ = key.coeffs[i]
            key.coeffs[i] = (m, r_, c, value.to_bytes(32, "little"))
        return edit
    for raw in (False, True):
        sfx = "_section4" if raw else ""
        add("coeff_is_r" + sfx, coeff(1, R), raw_coeffs=raw)
        add("coeff_all_ones" + sfx, coeff(len(toy_key().coeffs) - 1, (1 << 256) - 1), raw_coeffs=raw)
        add("coeff_r_minus_1" + sfx, coeff(0, R - 1), raw_coeffs=raw)          # canonical: passes

        def both(key):
            coeff(0, R)(key)
            coeff(3, R + 5)(key)
        add("coeff_two" + sfx, both, raw_coeffs=raw)

    # relations.  The toy key's pointsB1 / pointsB2 hold infinity where a wire is absent from B: pick wires that are not
    def live(key):
        return [i for i in range(key.nvars) if _get(key.sections["pointsB1"], 64, i) != bytes(64)]
    li = live(toy_key())
    assert len(li) >= 2, "the toy circuit has two wires in B"
    i, j = li[0], li[1]
    E = o.G1.mul(424242, o.GEN1)

    def b1_points(key):
        return [o.g1_from_bytes(_get(key.sections["pointsB1"], 64, k)) for k in range(key.nvars)]

    def swap(key):
        s = key.sections["pointsB1"]
        pi, pj = _get(s, 64, i), _get(s, 64, j)
        assert pi != pj
        key.sections["pointsB1"] = _set(_set(s, 64, i, pj), 64, j, pi)
    assert add("rel_b1_swapped", swap).report["relation"] == [0, 1, 1]

    def shift(key, wi, wj):
        """B1_i += wi E, B1_j -= wj E"""
        pts = b1_points(key)
        pts[i] = o.G1.add(pts[i], o.G1.mul(wi % R, E))
        pts[j] = o.G1.add(pts[j], o.G1.neg(o.G1.mul(wj % R, E)))
        key.sections["pointsB1"] = b"".join(o.g1_to_bytes(q) for q in pts)

    def zs_with(zi, zj):
        out = list(zs)
        out[i], out[j] = zi, zj
        return out
    z0 = 0x0123456789abcdef0fedcba987654321
    assert add("rel_cancel_bit127", lambda k: shift(k, 1, 1), zs_with(z0, z0 ^ (1 << 127))).report["relation"][0] == 0
    assert add("rel_cancel_equal_z", lambda k: shift(k, 1, 1), zs_with(z0, z0)).report["relation"][0] == 1
    za, zb, wa = Z_MAX, (1 << 127) + 1, 31337
    assert add("rel_cancel_weighted", lambda k: shift(k, wa, za * wa * pow(zb, -1, R)),
               zs_with(za, zb)).report["relation"][0] == 1
    assert add("rel_b1_inf", plant("pointsB1", i, bytes(64))).report["relation"] == [0, 1, 1]
    two_beta = o.g1_to_bytes(o.G1.add(o.g1_from_bytes(toy_key().sections["beta1"]),
                                      o.g1_from_bytes(toy_key().sections["beta1"])))
    assert add("rel_beta1_doubled", plant("beta1", 0, two_beta)).report["relation"] == [1, 0, 1]
    p = add("rel_delta2_inf", plant("delta2", 0, bytes(128)))
    assert p.report["relation"] == [1, 1, 0] and p.report["spec_infinity"] == 1 << 5
    assert p.report["failed"] == RELATION | SPEC_INFINITY
    # a relation is not run on a section that failed an element check
    assert pics["b2_small_order"].report["relation"] == [-1, 1, 1]
    assert pics["beta2_off_curve"].report["relation"] == [1, -1, 1]
    assert pics["clean_no_multipliers"].report["relation"] == [-1, 1, 1]
    return pics
