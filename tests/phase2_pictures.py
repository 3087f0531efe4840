"""Scalars, chains of contributions with planted defects, and the integer model of what g16_key_contribute and
g16_contributions_verify must give (tests/test_phase2_cpu.py, tests/test_gpu_phase2.py).  As in
tests/circuit_audit_pictures.py everything lives in LOG SPACE: every point is a known multiple of its generator, a pairing
equation e(a gen1, b gen2) == e(c gen1, d gen2) is a b == c d (mod r), and the model needs no curve arithmetic.  It owes
nothing to the code under test.

    edge_scalars()            the scalars every scaling test runs
    split(k)                  k = k1 + k2 lambda with exact rounding, in Python integers
    contribute(key, d, s, c)  the model of g16_key_contribute on logarithms
    pictures()                name -> ChainPicture, `report` filled in
    encode(pic, fixed)        the bytes the library is handed; fixed(group, [logs]) -> point bytes (the C oracle)"""
import copy
import functools
from dataclasses import dataclass, field

from oracle import bn254_ref as o
from tests import circuit_audit_pictures as CA
from tests import key_audit_pictures as KA

R, P = o.R, o.P
Z_MAX = (1 << 128) - 1
LAMBDA = 0xb3c4d79d41a917585bfc41088d8daaa78b17ea66b99c90dd
BETA = 2203960485148121921418603742825762020974279258880205651966
ARRAYS = ("delta_after", "g1_s", "g1_sx", "g2_spx", "challenges", "final delta1", "final delta2", "final pointsC1",
          "final pointsH1")
ARRAY_GROUP = (1, 1, 1, 2, 2, 1, 2, 1, 1)
RELATIONS = ("ELEMENTS", "POK", "STEP", "LAST", "DELTA", "C1", "H1")
# the arrays a relation reads (indices into ARRAYS)
READS = {"POK": (1, 2, 3, 4), "STEP": (0, 3, 4), "LAST": (0, 5), "DELTA": (5, 6), "C1": (6, 7), "H1": (6, 8)}


# ---- scalars -----------------------------------------------------------------------------------------------------------
def lattice_basis():
    """the two short vectors (a, b), a + b lambda = 0 (mod r), from the extended Euclid on (r, lambda)"""
    import math
    rows = [(R, 0), (LAMBDA, 1)]
    while rows[-1][0]:
        (r0, t0), (r1, t1) = rows[-2], rows[-1]
        q = r0 // r1
        rows.append((r0 - q * r1, t0 - q * t1))
    root = math.isqrt(R)
    at = next(i for i in range(len(rows) - 1) if rows[i][0] >= root > rows[i + 1][0])
    v1 = (rows[at + 1][0], -rows[at + 1][1])
    cands = [(rows[at][0], -rows[at][1]), (rows[at + 2][0], -rows[at + 2][1])]
    v2 = min(cands, key=lambda v: v[0] ** 2 + v[1] ** 2)
    return v1, v2


def split(k):
    """k = k1 + k2 lambda (mod r) by Babai rounding with exact quotients"""
    (a1, b1), (a2, b2) = _basis()
    det = a1 * b2 - a2 * b1
    c1 = (2 * b2 * k + det) // (2 * det)
    c2 = (-2 * b1 * k + det) // (2 * det)
    k1, k2 = k - c1 * a1 - c2 * a2, -c1 * b1 - c2 * b2
    assert (k1 + k2 * LAMBDA - k) % R == 0
    return k1, k2


@functools.lru_cache(None)
def _basis():
    return lattice_basis()


@functools.lru_cache(None)
def long_half_scalars(draws=4096):
    """of `draws` seeded scalars the two whose first half is longest and the two whose second half is longest"""
    rng = o.SplitMix64(2718)
    ks = [rng.fr() for _ in range(draws)]
    halves = {k: split(k) for k in ks}
    by1 = sorted(ks, key=lambda k: abs(halves[k][0]))[-2:]
    by2 = sorted(ks, key=lambda k: abs(halves[k][1]))[-2:]
    return by1 + by2


@functools.lru_cache(None)
def corner_scalars():
    """Constructed scalars at the edge of the fundamental parallelepiped of the library's decomposition.  It rounds DOWN
    with quotients that may fall short by up to ~0.25 (scale_plan.hpp), so its halves are (k1, k2) = x v1 + y v2 with
    x, y in [0, 1.25): k = k1 + k2 lambda for (x, y) a hair inside each corner of the unit square, and at y = 0.12, where a
    scan of the square found the quotient falling short and the halves longest (0.487 * 2^128: y ~ 1.12 in effect)."""
    (a1, b1), (a2, b2) = _basis()
    out = []
    for x in (1, 999):
        for y in (1, 120, 999):
            k1, k2 = (x * a1 + y * a2) // 1000, (x * b1 + y * b2) // 1000
            out.append((k1 + k2 * LAMBDA) % R)
    return out


def edge_scalars():
    return [0, 1, 2, R - 1, R - 2, LAMBDA, R - LAMBDA, (R - 1) // 2, 1 << 253, (1 << 253) - 1] + long_half_scalars() + \
        corner_scalars()


# ---- the model of a contribution -----------------------------------------------------------------------------------------
def key_part(circuit, flavour=CA.SNARKJS):
    """the logarithms of the part of a key a contribution touches, from the circuit audit's base key with delta = 1 as
    `snarkjs zkey new` leaves it"""
    k = CA.base(circuit, flavour).key
    d = k["delta1"][0]                                  # the base key has a delta of its own: take it out again
    return {"delta1": 1, "delta2": 1, "pointsC1": [x * d % R for x in k["pointsC1"]],
            "pointsH1": [x * d % R for x in k["pointsH1"]]}


def contribute(key, d, s, c):
    """g16_key_contribute on logarithms -> (the new key part, the record)"""
    di = pow(d, -1, R)
    new = {"delta1": key["delta1"] * d % R, "delta2": key["delta2"] * d % R,
           "pointsC1": [x * di % R for x in key["pointsC1"]], "pointsH1": [x * di % R for x in key["pointsH1"]]}
    return new, {"delta_after": new["delta1"], "g1_s": s % R, "g1_sx": d * s % R, "g2_spx": d * c % R}


@dataclass
class ChainPicture:
    name: str
    initial: dict
    final: dict
    records: list                                       # dicts of logarithms: delta_after, g1_s, g1_sx, g2_spx
    challenges: list                                    # logarithms
    zc: list
    zh: list
    overrides: dict = field(default_factory=dict)       # (array index into ARRAYS, element index) -> planted bytes
    report: dict = None
    expect: list = None                                 # the relation vector a picture completed by encode() must get


def _array_logs(pic, a):
    if a < 4:
        return [r[ARRAYS[a]] for r in pic.records]
    if a == 4:
        return list(pic.challenges)
    return {5: [pic.final["delta1"]], 6: [pic.final["delta2"]], 7: pic.final["pointsC1"], 8: pic.final["pointsH1"]}[a]


def model(pic) -> dict:
    first_bad, bad_count, first_inf, clean = [], [], [], []
    for a in range(len(ARRAYS)):
        planted = {i: b for (arr, i), b in pic.overrides.items() if arr == a}
        first, count = [None] * 3, [0] * 3
        for i in sorted(planted):
            v = KA.element_verdict(ARRAY_GROUP[a], planted[i])
            if v is not None:
                count[v] += 1
                first[v] = i if first[v] is None else first[v]
        inf = None
        if a <= 6:
            for i, x in enumerate(_array_logs(pic, a)):
                if (not any(planted[i]) if i in planted else x == 0):
                    inf = i
                    break
        first_bad.append(first)
        bad_count.append(count)
        first_inf.append(inf)
        clean.append(count == [0, 0, 0] and inf is None)
    dot = lambda z, xs: sum(a * b for a, b in zip(z, xs)) % R      # noqa: E731
    rel = {"ELEMENTS": 1 if all(clean) else 0}
    first_record = [None, None]
    runs = {name: all(clean[a] for a in reads) for name, reads in READS.items()}
    n = len(pic.records)
    if runs["POK"]:
        bad = [j for j in range(n) if (pic.records[j]["g1_s"] * pic.records[j]["g2_spx"] -
                                       pic.records[j]["g1_sx"] * pic.challenges[j]) % R]
        rel["POK"], first_record[0] = (0, bad[0]) if bad else (1, None)
    if runs["STEP"]:
        before = [pic.initial["delta1"]] + [r["delta_after"] for r in pic.records]
        bad = [j for j in range(n) if (before[j] * pic.records[j]["g2_spx"] -
                                       pic.records[j]["delta_after"] * pic.challenges[j]) % R]
        rel["STEP"], first_record[1] = (0, bad[0]) if bad else (1, None)
    if runs["LAST"]:
        rel["LAST"] = 1 if pic.final["delta1"] == (pic.records[-1]["delta_after"] if n else pic.initial["delta1"]) else 0
    if runs["DELTA"]:
        rel["DELTA"] = 1 if pic.final["delta1"] == pic.final["delta2"] else 0
    for name, sec, z in (("C1", "pointsC1", pic.zc), ("H1", "pointsH1", pic.zh)):
        if runs[name]:
            form = dot(z, pic.initial[sec]) * pic.initial["delta2"] - dot(z, pic.final[sec]) * pic.final["delta2"]
            rel[name] = 1 if form % R == 0 else 0
    relation = [rel.get(name, -1) for name in RELATIONS]
    failed = sum(1 << k for k, v in enumerate(relation) if v == 0)
    return {"failed": failed, "relation": relation, "first_record": first_record, "first_bad": first_bad,
            "bad_count": bad_count, "first_infinity": first_inf}


def honest(circuit, nrec, seed=0, flavour=CA.SNARKJS) -> ChainPicture:
    rng = o.SplitMix64(500 + seed + nrec + len(circuit))
    ini = key_part(circuit, flavour)
    key, recs, chs = ini, [], []
    for _ in range(nrec):
        d, s, c = (rng.fr() or 1 for _ in range(3))
        key, rec = contribute(key, d, s, c)
        recs.append(rec)
        chs.append(c)
    zc = [(rng.fr() & Z_MAX) or 1 for _ in ini["pointsC1"]]
    zh = [(rng.fr() & Z_MAX) or 1 for _ in ini["pointsH1"]]
    if zc:
        zc[0] = Z_MAX
    zh[0] = 1 << 127
    return ChainPicture("", copy.deepcopy(ini), copy.deepcopy(key), recs, chs, zc, zh)


@functools.lru_cache(None)
def pictures():
    pics = {}

    def add(name, circuit, nrec, edit=None, expect=None, **kw):
        pic = honest(circuit, nrec, **kw)
        pic.name = name
        if edit:
            edit(pic)
        pic.report = model(pic)
        if expect is not None:
            assert pic.report["relation"] == expect, (name, pic.report)
        pics[name] = pic
        return pic

    ok = [1] * 7
    for cname in ("toy", "chain"):
        for nrec in (0, 1, 3):
            assert add(f"honest_{cname}_{nrec}", cname, nrec, expect=ok).report["failed"] == 0
    add("honest_toy_jensgroth", "toy", 2, expect=ok, flavour=CA.JENSGROTH)
    for cname in ("toy", "chain"):
        def other_d(pic):
            pic.records[1]["g2_spx"] = pic.records[1]["g2_spx"] * 7 % R
        p = add(f"spx_other_d_{cname}", cname, 3, other_d, [1, 0, 0, 1, 1, 1, 1])
        assert p.report["first_record"] == [1, 1]

        def sx_wrong(pic):
            pic.records[2]["g1_sx"] = (pic.records[2]["g1_sx"] + 1) % R
        p = add(f"sx_wrong_{cname}", cname, 3, sx_wrong, [1, 0, 1, 1, 1, 1, 1])
        assert p.report["first_record"] == [2, None]

        def swapped(pic):
            pic.records[0], pic.records[1] = pic.records[1], pic.records[0]
            pic.challenges[0], pic.challenges[1] = pic.challenges[1], pic.challenges[0]
        p = add(f"records_swapped_{cname}", cname, 3, swapped, [1, 1, 0, 1, 1, 1, 1])
        assert p.report["first_record"] == [None, 0]

        def wrong_challenge(pic):
            pic.challenges[1] = (pic.challenges[1] + 5) % R
        p = add(f"wrong_challenge_{cname}", cname, 3, wrong_challenge, [1, 0, 0, 1, 1, 1, 1])
        assert p.report["first_record"] == [1, 1]

        def not_last(pic):                                   # a consistent key of another delta than the chain's
            d = 99
            di = pow(d, -1, R)
            pic.final = {"delta1": pic.final["delta1"] * d % R, "delta2": pic.final["delta2"] * d % R,
                         "pointsC1": [x * di % R for x in pic.final["pointsC1"]],
                         "pointsH1": [x * di % R for x in pic.final["pointsH1"]]}
        add(f"final_not_last_{cname}", cname, 2, not_last, [1, 1, 1, 0, 1, 1, 1])
        add(f"final_not_initial_{cname}", cname, 0, not_last, [1, 1, 1, 0, 1, 1, 1])

        def delta2_other(pic):
            pic.final["delta2"] = pic.final["delta2"] * 3 % R
        add(f"delta2_other_factor_{cname}", cname, 2, delta2_other, [1, 1, 1, 1, 0, 0, 0])
        nc1 = len(key_part(cname)["pointsC1"])
        for i in (0, nc1 - 1):
            def c1_moved(pic, i=i):
                pic.final["pointsC1"][i] = (pic.final["pointsC1"][i] + 424242) % R
            add(f"c1_moved_{cname}_{i}", cname, 1, c1_moved, [1, 1, 1, 1, 1, 0, 1])

        def h1_moved(pic):
            pic.final["pointsH1"][-1] = (pic.final["pointsH1"][-1] + 424242) % R
        add(f"h1_moved_{cname}", cname, 1, h1_moved, [1, 1, 1, 1, 1, 1, 0])
    # element defects, one array at a time: a non-canonical or off-curve element, and g2_spx / a challenge / delta2 outside
    # the subgroup; the relations that read the array are not run
    small = o.g2_to_bytes(KA.twist_outsiders()["small"])
    expect = {0: [0, 1, -1, -1, 1, 1, 1], 1: [0, -1, 1, 1, 1, 1, 1], 2: [0, -1, 1, 1, 1, 1, 1], 3: [0, -1, -1, 1, 1, 1, 1],
              4: [0, -1, -1, 1, 1, 1, 1], 5: [0, 1, 1, -1, -1, 1, 1], 6: [0, 1, 1, 1, -1, -1, -1],
              7: [0, 1, 1, 1, 1, -1, 1], 8: [0, 1, 1, 1, 1, 1, -1]}
    for a, name in enumerate(ARRAYS):
        g = ARRAY_GROUP[a]
        at = 1 if a < 5 else 0 if a < 7 else 2
        tag = name.replace(" ", "_")
        p = add(f"off_curve_{tag}", "toy", 2, lambda pic, a=a, at=at, g=g: pic.overrides.update({(a, at): KA.off_curve(g)}),
                expect[a])
        assert p.report["first_bad"][a] == [None, at, None]
        # the non-canonical alias of the honest element (its x raised by p) needs the element's bytes: encode() plants
        # it where the override is None and fills in the report
        pic = honest("toy", 2)
        pic.name = f"not_canonical_{tag}"
        pic.overrides[a, at] = None
        pic.expect = expect[a]
        pics[pic.name] = pic
        if g == 2:
            p = add(f"outside_subgroup_{tag}", "toy", 2, lambda pic, a=a, at=at: pic.overrides.update({(a, at): small}),
                    expect[a])
            assert p.report["first_bad"][a] == [None, None, at]
    p = add("infinity_g1_s", "toy", 2, lambda pic: pic.records[0].update({"g1_s": 0}), [0, -1, 1, 1, 1, 1, 1])
    assert p.report["first_infinity"][1] == 0
    return pics


def encode(pic, fixed):
    """-> (initial, final: {delta1, delta2, pointsC1, pointsH1: bytes}, [record bytes], [challenge bytes]); fixed(group,
    tuple of logs) -> bytes.  A picture whose override is None gets the non-canonical alias of the honest element planted
    there (its x coordinate raised by p), and its report is filled in."""
    arrays = []
    for a in range(len(ARRAYS)):
        logs = _array_logs(pic, a)
        arrays.append(bytearray(fixed(ARRAY_GROUP[a], tuple(logs)) if logs else b""))
    for (a, i), b in list(pic.overrides.items()):
        psz = 64 * ARRAY_GROUP[a]
        if b is None:
            b = KA.raise_by_p(ARRAY_GROUP[a], bytes(arrays[a][psz * i:psz * (i + 1)]), 0)
            pic.overrides[a, i] = b
        arrays[a][psz * i:psz * (i + 1)] = b
    if pic.report is None:
        pic.report = model(pic)
        assert pic.expect is None or pic.report["relation"] == pic.expect, (pic.name, pic.report)
    part = lambda k: {"delta1": fixed(1, (k["delta1"],)), "delta2": fixed(2, (k["delta2"],)),          # noqa: E731
                      "pointsC1": fixed(1, tuple(k["pointsC1"])) if k["pointsC1"] else b"",
                      "pointsH1": fixed(1, tuple(k["pointsH1"]))}
    ini = part(pic.initial)
    fin = {"delta1": bytes(arrays[5]), "delta2": bytes(arrays[6]), "pointsC1": bytes(arrays[7]), "pointsH1": bytes(arrays[8])}
    recs = [bytes(arrays[0][64 * j:64 * j + 64] + arrays[1][64 * j:64 * j + 64] + arrays[2][64 * j:64 * j + 64] +
                  arrays[3][128 * j:128 * j + 128]) for j in range(len(pic.records))]
    chs = [bytes(arrays[4][128 * j:128 * j + 128]) for j in range(len(pic.records))]
    return ini, fin, recs, chs
