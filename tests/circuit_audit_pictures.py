"""Keys, circuits and powers of tau with planted defects for the circuit audit (g16_circuit_audit), and the integer model
of what it must report.  Everything lives in LOG SPACE: every point of a test key and of a test ptau is a known multiple
of its generator (the oracle's fake_circuit_setup with the identity in place of `k * gen`), so each relation of the audit
is a linear form mod r in the caller's multipliers and the model needs no curve arithmetic at all:

    relation holds  <=>  its form is 0 (mod r)

The model owes nothing to the code under test: sparse products, the inverse NTT (oracle.inverse_ntt) and the sums are
Python integers.  Element checks are only ever needed for the few planted BYTES (`overrides`), by the model of
tests/key_audit_pictures.py; every other point is valid by construction.

    circuits()            name -> Circuit
    pictures()            name -> Picture, `report` filled in
    encode(pic, fixed)    the bytes the library is handed; fixed(group, [logs]) -> point bytes (the C oracle)"""
import copy
import functools
from dataclasses import dataclass, field

from oracle import bn254_ref as o
from tests import key_audit_pictures as KA

R = o.R
Z_MAX = (1 << 128) - 1
SNARKJS, JENSGROTH = 1, 0
FLAVOUR = {SNARKJS: o.SNARKJS, JENSGROTH: o.JENS_GROTH}
KEY_SECTIONS = KA.SECTIONS
PTAU_SECTIONS = ("tauG1", "tauG2", "alphaTauG1", "betaTauG1", "betaG2")
PTAU_GROUP = {"tauG1": 1, "tauG2": 2, "alphaTauG1": 1, "betaTauG1": 1, "betaG2": 2}
RELATIONS = ("COEFFS_A", "COEFFS_B", "SPEC", "A1", "B1", "B2", "C1", "IC", "H1")
F_KEY, F_PTAU, F_COEFFS, F_SPEC, F_POINTS = 1, 2, 4, 8, 16
# the sections a relation reads: (key sections, ptau sections)
READS = {"COEFFS_A": (("coeffs",), ()), "COEFFS_B": (("coeffs",), ()),
         "SPEC": (("alpha1", "beta1", "beta2"), PTAU_SECTIONS),
         "A1": (("pointsA1",), ("tauG1",)), "B1": (("pointsB1",), ("tauG1",)), "B2": (("pointsB2",), ("tauG2",)),
         "C1": (("pointsC1", "delta2"), ("tauG1", "alphaTauG1", "betaTauG1")),
         "IC": (("pointsIC", "gamma2"), ("tauG1", "alphaTauG1", "betaTauG1")),
         "H1": (("pointsH1", "delta2"), ("tauG1",))}


@dataclass
class Circuit:
    nvars: int
    npubs: int
    constraints: list                 # [(A, B, C)], each [(wire, value)]: the list form of an R1CS

    @property
    def ncons(self):
        return len(self.constraints)

    @property
    def log2_domain(self):
        return o.ceiling_log2(self.ncons + self.npubs + 1)

    def triplets(self):
        """per matrix [(constraint, wire, value)], in file order: duplicates and zeros stay"""
        out = ([], [], [])
        for i, con in enumerate(self.constraints):
            for k in range(3):
                out[k].extend((i, w, v % R) for w, v in con[k])
        return [list(m) for m in out]


@functools.lru_cache(None)
def circuits():
    from nim_groth16_amd.synthetic import squaringChain
    toy = o.toy_r1cs()
    chain, _ = squaringChain((1 << 9) - 2, seed=4)
    # the toy circuit with a (constraint, wire) pair given twice (values add up) and a pair of entries that cancel
    m1 = R - 1
    dup = [([], [], [(1, m1), (2, 1), (7, 1)]),
           ([(3, 1), (3, 2)], [(4, 1), (1, 3)], [(6, 1)]),                     # ... and a public wire in B
           ([(5, 1)], [(6, 1), (4, 5), (4, R - 5)], [(7, 1)])]
    # no private wire: nvars - npubs - 1 == 0
    nopriv = [([(1, 1)], [(2, 1)], [(0, 6)])]
    return {"toy": Circuit(8, 2, toy.constraints), "chain": Circuit(chain.nWires, 1, chain.constraints),
            "dup": Circuit(8, 2, dup), "nopriv": Circuit(3, 2, nopriv)}


def toxic(seed):
    rng = o.SplitMix64(seed)
    return o.ToxicWaste(*[rng.fr() or 1 for _ in range(5)])


@dataclass
class Picture:
    name: str
    circuit: str
    flavour: int
    nvars: int
    npubs: int
    ncons: int
    log2_domain: int
    r1cs: list                        # three lists of (constraint, wire, value)
    coeffs: list                      # the key's: (matrix, row, wire, value)
    key: dict                         # section -> [logarithms]
    power: int
    ptau: dict                        # section -> [logarithms]
    zw: list
    zh: list
    with_vk: bool = True
    raw_coeffs: bool = False
    overrides: dict = field(default_factory=dict)    # ("key" | "ptau", section, index) -> planted bytes
    report: dict = None

    @property
    def n(self):
        return 1 << self.log2_domain


def ptau_logs(tau, alpha, beta, power):
    n1, n = (2 << power) - 1, 1 << power
    t = [pow(tau, k, R) for k in range(n1)]
    return {"tauG1": t, "tauG2": t[:n], "alphaTauG1": [alpha * x % R for x in t[:n]],
            "betaTauG1": [beta * x % R for x in t[:n]], "betaG2": [beta % R]}


@functools.lru_cache(None)
def _base(circuit, flavour):
    c = circuits()[circuit]
    tw = toxic(1000 + len(circuit))
    ident = lambda ks: [k % R for k in ks]                                   # noqa: E731  the key in log space
    zk = o.fake_circuit_setup(o.R1CS(c.nvars, c.npubs, 0, c.nvars - c.npubs - 1, c.constraints), tw, FLAVOUR[flavour],
                              ident, ident)
    key = {"alpha1": [zk.alpha1], "beta1": [zk.beta1], "delta1": [zk.delta1], "beta2": [zk.beta2], "gamma2": [zk.gamma2],
           "delta2": [zk.delta2]}
    for name in KEY_SECTIONS[6:12]:
        key[name] = list(getattr(zk, name))
    L = c.log2_domain
    rng = o.SplitMix64(31 + len(circuit) + flavour)
    zw = [(rng.fr() & Z_MAX) or 1 for _ in range(c.nvars)]
    zh = [(rng.fr() & Z_MAX) or 1 for _ in range(1 << L)]
    zw[0], zh[0] = Z_MAX, 1 << 127                                           # every one of the 128 bits is in play
    return Picture("", circuit, flavour, c.nvars, c.npubs, c.ncons, L, c.triplets(), list(zk.coeffs), key, L + 1,
                   ptau_logs(tw.tau, tw.alpha, tw.beta, L + 1), zw, zh), tw


def base(circuit, flavour=SNARKJS) -> Picture:
    return copy.deepcopy(_base(circuit, flavour)[0])


# ---- the model ---------------------------------------------------------------------------------------------------------
def with_dummies(pic, k):
    ent = list(pic.r1cs[k])
    if k == 0:
        ent += [(pic.ncons + i, i, 1) for i in range(pic.npubs + 1)]
    return ent


def matvec(entries, z, n):
    out = [0] * n
    for row, col, v in entries:
        out[row] = (out[row] + v * z[col]) % R
    return out


def coef(values):
    """coef_m: the coefficients of the polynomial with these values on the m-point domain"""
    return o.inverse_ntt(values, o.Domain(len(values)))


def h_coefficients(flavour, zh):
    """the vector c of the H relation: MSM(c, tauG1[0 .. 2n)) must be delta * MSM(y, pointsH1)"""
    n = len(zh)
    if flavour == SNARKJS:
        v = [0] * (2 * n)
        v[1::2] = zh
        return coef(v)
    return [(-y) % R for y in zh] + [y % R for y in zh]


def dot(a, b):
    return sum(x * y for x, y in zip(a, b)) % R


def forms(pic):
    """relation -> its linear form in the multipliers (0 = holds); COEFFS_*: (form, first row); SPEC: 0 / 1"""
    n, nv, p = pic.n, pic.nvars, pic.npubs
    zpub = [z if i <= p else 0 for i, z in enumerate(pic.zw)]
    zpriv = [0 if i <= p else z for i, z in enumerate(pic.zw)]
    K, t = pic.key, pic.ptau
    out = {}
    prod = {}
    for k in range(3):
        ent = with_dummies(pic, k)
        prod[k] = (matvec(ent, zpub, n), matvec(ent, zpriv, n))
    for k in range(2):
        kent = [(row, col, v) for m, row, col, v in pic.coeffs if m == k]
        bad = [i for h, z in enumerate((zpub, zpriv)) for i, (a, b) in enumerate(zip(matvec(kent, z, n), prod[k][h]))
               if a != b]
        out[RELATIONS[k]] = (1 if bad else 0, min(bad) if bad else None)
    out["SPEC"] = 0 if (K["alpha1"][0] == t["alphaTauG1"][0] and K["beta1"][0] == t["betaTauG1"][0] and
                        K["beta2"][0] == t["betaG2"][0] and t["tauG1"][0] == 1 and t["tauG2"][0] == 1) else 1
    cf = {(k, h): coef(prod[k][h]) for k in range(3) for h in range(2)}
    cA = [(a + b) % R for a, b in zip(cf[0, 0], cf[0, 1])]
    cB = [(a + b) % R for a, b in zip(cf[1, 0], cf[1, 1])]
    out["A1"] = (dot(pic.zw, K["pointsA1"]) - dot(cA, t["tauG1"])) % R
    out["B1"] = (dot(pic.zw, K["pointsB1"]) - dot(cB, t["tauG1"])) % R
    out["B2"] = (dot(pic.zw, K["pointsB2"]) - dot(cB, t["tauG2"])) % R

    def rhs(h):
        return (dot(cf[0, h], t["betaTauG1"]) + dot(cf[1, h], t["alphaTauG1"]) + dot(cf[2, h], t["tauG1"])) % R
    out["C1"] = (K["delta2"][0] * dot(pic.zw[p + 1:], K["pointsC1"]) - rhs(1)) % R
    out["IC"] = (K["gamma2"][0] * dot(pic.zw[:p + 1], K["pointsIC"]) - rhs(0)) % R
    out["H1"] = (K["delta2"][0] * dot(pic.zh, K["pointsH1"]) - dot(h_coefficients(pic.flavour, pic.zh), t["tauG1"])) % R
    return out


def _counts(group, planted):
    first, count = [None] * 3, [0] * 3
    for idx in sorted(planted):
        v = KA.element_verdict(group, planted[idx]) if group else (0 if int.from_bytes(planted[idx], "little") >= R else None)
        if v is not None:
            count[v] += 1
            first[v] = idx if first[v] is None else first[v]
    return first, count


def model(pic) -> dict:
    planted = lambda space, name: {i: b for (s, nm, i), b in pic.overrides.items() if s == space and nm == name}   # noqa: E731
    # the key on its own: g16_key_audit's report
    kfirst, kcount = [], []
    for name in KEY_SECTIONS:
        skip = not pic.with_vk and name in ("gamma2", "pointsIC")
        f, c = _counts(KA.GROUP.get(name, 0), {} if skip else planted("key", name))
        kfirst.append(f)
        kcount.append(c)
    kclean = lambda name: kcount[KEY_SECTIONS.index(name)] == [0, 0, 0]      # noqa: E731
    kfailed = 0
    for c in kcount:
        for k in range(3):
            if c[k]:
                kfailed |= (KA.CANONICAL, KA.CURVE, KA.SUBGROUP)[k]
    spec_inf = 0
    for s, name in enumerate(KEY_SECTIONS[:6]):
        if (pic.with_vk or name != "gamma2") and pic.key[name][0] == 0 and ("key", name, 0) not in pic.overrides:
            spec_inf |= 1 << s
    if spec_inf:
        kfailed |= KA.SPEC_INFINITY
    krel = [-1, -1, -1]
    if kclean("pointsB1") and kclean("pointsB2"):
        krel[0] = 1 if dot(pic.zw, [(a - b) % R for a, b in zip(pic.key["pointsB1"], pic.key["pointsB2"])]) == 0 else 0
    if kclean("beta1") and kclean("beta2"):
        krel[1] = 1 if pic.key["beta1"] == pic.key["beta2"] else 0
    if kclean("delta1") and kclean("delta2"):
        krel[2] = 1 if pic.key["delta1"] == pic.key["delta2"] else 0
    if 0 in krel:
        kfailed |= KA.RELATION
    key = {"failed": kfailed, "spec_infinity": spec_inf, "relation": krel, "first_bad": kfirst, "bad_count": kcount}
    # the ptau arrays: what the call reads of them
    pfirst, pcount = [], []
    for name in PTAU_SECTIONS:
        f, c = _counts(PTAU_GROUP[name], planted("ptau", name))
        pfirst.append(f)
        pcount.append(c)
    pclean = lambda name: pcount[PTAU_SECTIONS.index(name)] == [0, 0, 0]     # noqa: E731
    failed = (F_KEY if kfailed else 0) | (F_PTAU if any(c != [0, 0, 0] for c in pcount) else 0)
    fm = forms(pic)
    rel, first_row = [], [None, None]
    for k, name in enumerate(RELATIONS):
        ks, ps = READS[name]
        if not (all(kclean(s) for s in ks) and all(pclean(s) for s in ps)) or (name == "IC" and not pic.with_vk):
            rel.append(-1)
            continue
        if k < 2:
            rel.append(1 if fm[name][0] == 0 else 0)
            first_row[k] = fm[name][1]
        else:
            rel.append(1 if fm[name] == 0 else 0)
        if rel[-1] == 0:
            failed |= F_COEFFS if k < 2 else F_SPEC if k == 2 else F_POINTS
    return {"key": key, "ptau_first_bad": pfirst, "ptau_bad_count": pcount, "relation": rel, "failed": failed,
            "first_row": first_row}


# ---- the pictures ------------------------------------------------------------------------------------------------------
def _move(pic, section, i, d=424242):
    pic.key[section][i] = (pic.key[section][i] + d) % R


@functools.lru_cache(None)
def pictures():
    pics = {}

    def add(name, circuit, flavour=SNARKJS, edit=None, **kw):
        pic = base(circuit, flavour)
        pic.name = name
        for k, v in kw.items():
            setattr(pic, k, v)
        if edit:
            edit(pic)
        pic.report = model(pic)
        pics[name] = pic
        return pic

    both = (("sn", SNARKJS), ("jg", JENSGROTH))
    for cname in circuits():
        for sfx, fl in both:
            assert add(f"clean_{cname}_{sfx}", cname, fl).report["failed"] == 0
    add("clean_toy_section4", "toy", raw_coeffs=True)
    add("clean_chain_section4", "chain", raw_coeffs=True)
    p = add("clean_toy_no_vk", "toy", with_vk=False)
    assert p.report["relation"][7] == -1 and p.report["failed"] == 0
    # the key's description of the dup circuit with its duplicates merged and the cancelling pair dropped: the same maps
    def merged(pic):
        acc = {}
        for m, row, col, v in pic.coeffs:
            acc[m, row, col] = (acc.get((m, row, col), 0) + v) % R
        assert len(acc) == len(pic.coeffs) - 2
        pic.coeffs = [(m, row, col, v) for (m, row, col), v in acc.items() if v]
        assert len(pic.coeffs) == len(acc) - 1
    assert add("dup_merged_key", "dup", edit=merged).report["failed"] == 0

    for cname in ("toy", "chain"):
        c = circuits()[cname]
        # a consistent change of delta: delta1/2 x d, pointsC1 and pointsH1 x 1/d -- a contributed key: it passes
        for sfx, fl in both:
            def contributed(pic, d=987654321):
                di = pow(d, -1, R)
                pic.key["delta1"][0] = pic.key["delta1"][0] * d % R
                pic.key["delta2"][0] = pic.key["delta2"][0] * d % R
                pic.key["pointsC1"] = [x * di % R for x in pic.key["pointsC1"]]
                pic.key["pointsH1"] = [x * di % R for x in pic.key["pointsH1"]]
            assert add(f"delta_changed_{cname}_{sfx}", cname, fl, contributed).report["failed"] == 0
        for i in (0, c.npubs, c.npubs + 1, c.nvars - 1):
            p = add(f"a1_moved_{cname}_{i}", cname, edit=lambda pic, i=i: _move(pic, "pointsA1", i))
            assert p.report["relation"] == [1, 1, 1, 0, 1, 1, 1, 1, 1], p.name
        live = [i for i, x in enumerate(_base(cname, SNARKJS)[0].key["pointsB1"]) if x][-1]

        def b_both(pic, i=live):
            _move(pic, "pointsB1", i)
            _move(pic, "pointsB2", i)
        p = add(f"b1_b2_moved_{cname}", cname, edit=b_both)
        assert p.report["relation"] == [1, 1, 1, 1, 0, 0, 1, 1, 1] and p.report["key"]["relation"] == [1, 1, 1]
        p = add(f"c1_moved_{cname}", cname, edit=lambda pic: _move(pic, "pointsC1", len(pic.key["pointsC1"]) - 1))
        assert p.report["relation"] == [1, 1, 1, 1, 1, 1, 0, 1, 1]
        p = add(f"ic_moved_{cname}", cname, edit=lambda pic: _move(pic, "pointsIC", 1))
        assert p.report["relation"] == [1, 1, 1, 1, 1, 1, 1, 0, 1]
        for sfx, fl in both:
            p = add(f"h1_moved_{cname}_{sfx}", cname, fl, lambda pic: _move(pic, "pointsH1", pic.n - 1))
            assert p.report["relation"] == [1, 1, 1, 1, 1, 1, 1, 1, 0]

        # the coefficients.  The key's points still belong to the r1cs: only COEFFS_* fails
        def coeff_value(pic, raw=False):
            at = next(e for e, (m, *_) in enumerate(pic.coeffs) if m == 1)
            m, row, col, v = pic.coeffs[at]
            pic.coeffs[at] = (m, row, col, (v + 1) % R)
        for raw in (False, True):
            p = add(f"coeff_value_{cname}" + ("_section4" if raw else ""), cname, edit=coeff_value, raw_coeffs=raw)
            assert p.report["relation"][:2] == [1, 0] and p.report["relation"][3:] == [1] * 6
            assert p.report["failed"] == F_COEFFS and p.report["first_row"][0] is None

        def coeff_row(pic):
            at = [e for e, (m, *_) in enumerate(pic.coeffs) if m == 0][1]
            m, row, col, v = pic.coeffs[at]
            pic.coeffs[at] = (m, row + 2, col, v)
        p = add(f"coeff_row_{cname}", cname, edit=coeff_row)
        row = [e for e in _base(cname, SNARKJS)[0].coeffs if e[0] == 0][1][1]
        assert p.report["relation"][:2] == [0, 1] and p.report["first_row"] == [row, None], p.report

        # one r1cs entry changed: the key (coefficients AND points) belongs to another circuit
        def r1cs_entry(pic):
            at = len(pic.r1cs[0]) - 1
            i, w, v = pic.r1cs[0][at]
            pic.r1cs[0][at] = (i, w, (v + 5) % R)
        p = add(f"r1cs_entry_{cname}", cname, edit=r1cs_entry)
        rel = p.report["relation"]
        assert rel[0] == 0 and rel[3] == 0 and rel[5] == 1, rel          # A changed: COEFFS_A, A1 (and C1 or IC)
        assert 0 in (rel[6], rel[7])

        # a ptau from another alpha, from another tau
        def other_alpha(pic):
            tw = _base(pic.circuit, SNARKJS)[1]
            pic.ptau = ptau_logs(tw.tau, tw.alpha + 1, tw.beta, pic.power)
        p = add(f"ptau_other_alpha_{cname}", cname, edit=other_alpha)
        # alpha meets the key through alpha * B_j(tau): pointsIC feels it only if a public wire occurs in B
        b_public = any(w <= c.npubs for _, w, _ in p.r1cs[1])
        assert p.report["relation"] == [1, 1, 0, 1, 1, 1, 0, 0 if b_public else 1, 1], p.name
        if cname == "toy":
            assert not b_public
            p = add("ptau_other_alpha_dup", "dup", edit=other_alpha)
            assert p.report["relation"] == [1, 1, 0, 1, 1, 1, 0, 0, 1]

        def other_tau(pic):
            tw = _base(pic.circuit, SNARKJS)[1]
            pic.ptau = ptau_logs(tw.tau + 1, tw.alpha, tw.beta, pic.power)
        p = add(f"ptau_other_tau_{cname}", cname, edit=other_tau)
        assert p.report["relation"] == [1, 1, 1, 0, 0, 0, 0, 0, 0]

        # the key's flavour flipped against its pointsH1
        def flipped(pic):
            pic.flavour = JENSGROTH
        p = add(f"flavour_flipped_{cname}", cname, SNARKJS, flipped)
        assert p.report["relation"] == [1, 1, 1, 1, 1, 1, 1, 1, 0]

    # a ptau whose tauG2 holds a point outside the order-r subgroup: what reads tauG2 is not run
    small = o.g2_to_bytes(KA.twist_outsiders()["small"])

    def outsider(pic):
        pic.overrides["ptau", "tauG2", 3] = small
    p = add("ptau_tau_g2_outsider", "toy", edit=outsider)
    assert p.report["relation"] == [1, 1, -1, 1, 1, -1, 1, 1, 1] and p.report["failed"] == F_PTAU
    assert p.report["ptau_first_bad"][1] == [None, None, 3]
    p = add("ptau_tau_g2_outsider_chain", "chain",
            edit=lambda pic: pic.overrides.update({("ptau", "tauG2", 300): small, ("ptau", "tauG2", 511): small}))
    assert p.report["ptau_bad_count"][1] == [0, 0, 2] and p.report["relation"][5] == -1
    # a key coefficient that is not canonical: the key audit's finding; COEFFS_* is not run
    for raw in (False, True):
        p = add("coeff_not_canonical" + ("_section4" if raw else ""), "toy", raw_coeffs=raw,
                edit=lambda pic: pic.overrides.update({("key", "coeffs", 2): R.to_bytes(32, "little")}))
        assert p.report["relation"][:2] == [-1, -1] and p.report["failed"] == F_KEY
    # an element defect in the key: the relations over that section are not run, the others are
    p = add("a1_off_curve", "toy", edit=lambda pic: pic.overrides.update({("key", "pointsA1", 5): KA.off_curve(1)}))
    assert p.report["relation"] == [1, 1, 1, -1, 1, 1, 1, 1, 1] and p.report["failed"] == F_KEY

    # cancellation: pointsA1[i] += d, pointsA1[j] += d' with z_i d + z_j d' = 0 (mod r): the relation IS the equation and
    # holds; with the top bit of z_j flipped it does not -- all 128 bits of a multiplier count
    for cname, (i, j) in (("toy", (3, 5)), ("chain", (255, 256))):
        def cancel(pic, flip, i=i, j=j):
            d = 31337
            if flip:
                pic.zw[j] ^= 1 << 127
                assert pic.zw[j]
            zj = pic.zw[j] ^ (1 << 127) if flip else pic.zw[j]
            d2 = (-pic.zw[i] * d) * pow(zj, -1, R) % R
            _move(pic, "pointsA1", i, d)
            _move(pic, "pointsA1", j, d2)
        assert add(f"a1_cancel_{cname}", cname, edit=lambda pic: cancel(pic, False)).report["failed"] == 0
        p = add(f"a1_cancel_bit127_{cname}", cname, edit=lambda pic: cancel(pic, True))
        assert p.report["relation"] == [1, 1, 1, 0, 1, 1, 1, 1, 1]
    return pics


# ---- bytes ---------------------------------------------------------------------------------------------------------------
def coeff_bytes(pic):
    """[(matrix, row, wire, 32 value bytes)]: Montgomery limbs, or the doubly-Montgomery integer of a .zkey's section 4"""
    out = []
    for e, (m, row, col, v) in enumerate(pic.coeffs):
        b = pic.overrides.get(("key", "coeffs", e))
        if b is None:
            b = (v * o.FR_MONT_R * (o.FR_MONT_R if pic.raw_coeffs else 1) % R).to_bytes(32, "little")
        out.append((m, row, col, b))
    return out


def encode(pic, fixed):
    """-> (key sections: name -> bytes, ptau sections: name -> bytes); fixed(group, tuple of logs) -> bytes"""
    key, ptau = {}, {}
    for space, src, dst, names, group in (("key", pic.key, key, KEY_SECTIONS[:12], KA.GROUP),
                                          ("ptau", pic.ptau, ptau, PTAU_SECTIONS, PTAU_GROUP)):
        for name in names:
            g = group[name]
            raw = bytearray(fixed(g, tuple(src[name])))
            for (s, nm, i), b in pic.overrides.items():
                if s == space and nm == name:
                    raw[64 * g * i:64 * g * (i + 1)] = b
            dst[name] = bytes(raw)
    return key, ptau
