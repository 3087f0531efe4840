"""Powers of tau with planted defects, chains of phase-1 records, and the integer model of what g16_ptau_contribute and
g16_ptau_verify must give (tests/test_phase1_cpu.py, tests/test_gpu_phase1.py).  As in tests/phase2_pictures.py everything
lives in LOG SPACE: every point is a known multiple of its generator, a pairing equation e(a gen1, b gen2) == e(c gen1,
d gen2) is a b == c d (mod r), and the model needs no curve arithmetic.  It owes nothing to the code under test.

    new_ptau(power)                      the logarithms of a file of generators
    contribute(pt, t, a, b, s3, c3)      the model of g16_ptau_contribute -> (new file, record)
    chain(power, k)                      a clean file after k contributions -> Picture
    pictures()                           name -> Picture, `report` filled in
    encode(pic, fixed)                   the bytes the library is handed; fixed(group, [logs]) -> point bytes"""
import copy
import functools
from dataclasses import dataclass, field

from oracle import bn254_ref as o
from tests import key_audit_pictures as KA

R = o.R
FILE = ("tauG1", "tauG2", "alphaTauG1", "betaTauG1", "betaG2")
ARRAYS = FILE + ("record tauG1", "record alphaG1", "record betaG1", "record tauG2", "record betaG2", "g1_s", "g1_sx", "g2_spx",
                 "challenges")
GROUP = (1, 2, 1, 1, 2, 1, 1, 1, 2, 2, 1, 1, 2, 2)
RELATIONS = ("ELEMENTS", "FIRST", "TAU_G1", "TAU_G2", "ALPHA", "BETA", "BETA_G2", "POK", "STEP", "LAST")
REC = ("tauG1", "alphaG1", "betaG1", "tauG2", "betaG2")


def new_ptau(power):
    n = 1 << power
    return {"tauG1": [1] * (2 * n - 1), "tauG2": [1] * n, "alphaTauG1": [1] * n, "betaTauG1": [1] * n, "betaG2": [1]}


def contribute(pt, t, a, b, s3, c3):
    """g16_ptau_contribute on logarithms; s3: the proof-of-knowledge secrets, c3: the logarithms of the challenges"""
    new = {"tauG1": [x * pow(t, i, R) % R for i, x in enumerate(pt["tauG1"])],
           "tauG2": [x * pow(t, i, R) % R for i, x in enumerate(pt["tauG2"])],
           "alphaTauG1": [x * a * pow(t, i, R) % R for i, x in enumerate(pt["alphaTauG1"])],
           "betaTauG1": [x * b * pow(t, i, R) % R for i, x in enumerate(pt["betaTauG1"])],
           "betaG2": [pt["betaG2"][0] * b % R]}
    rec = {"tauG1": new["tauG1"][1], "alphaG1": new["alphaTauG1"][0], "betaG1": new["betaTauG1"][0],
           "tauG2": new["tauG2"][1], "betaG2": new["betaG2"][0],
           "pok": [(s % R, x * s % R, x * c % R) for x, s, c in zip((t, a, b), s3, c3)]}
    return new, rec


@dataclass
class Picture:
    name: str
    ptau: dict                                          # logarithms per array of FILE; 0 = the point (0,0)
    records: list                                       # None = no chain given
    challenges: list                                    # per record three logarithms
    multipliers: list
    raw: dict = field(default_factory=dict)             # (array name, index) -> bytes of an element that has no logarithm
    report: dict = None

    @property
    def power(self):
        return len(self.ptau["tauG2"]).bit_length() - 1


def multipliers(power, seed=7):
    rng = o.SplitMix64(seed)
    return [((rng.next() << 64) | rng.next() | 1) for _ in range((2 << power) - 2)]


def chain(power, k, seed=100):
    rng = o.SplitMix64(seed + 10 * power + k)
    pt, recs, chs = new_ptau(power), [], []
    for _ in range(k):
        t, a, b, s0, s1, s2, c0, c1, c2 = (rng.fr() or 1 for _ in range(9))
        pt, rec = contribute(pt, t, a, b, (s0, s1, s2), (c0, c1, c2))
        recs.append(rec)
        chs.append([c0, c1, c2])
    return Picture(f"clean_p{power}_k{k}", pt, recs, chs, multipliers(power))


def arrays_of(pic):
    """the fourteen arrays of the report as lists of logarithms"""
    recs = pic.records or []
    out = [pic.ptau[k] for k in FILE] + [[r[k] for r in recs] for k in REC]
    for f in range(3):
        out.append([r["pok"][x][f] for r in recs for x in range(3)])
    out.append([c for ch in (pic.challenges if pic.records is not None else []) for c in ch])
    return out


def model(pic):
    """the full report g16_ptau_verify must give"""
    arr = arrays_of(pic)
    first_bad = [[None] * 3 for _ in ARRAYS]
    bad_count = [[0] * 3 for _ in ARRAYS]
    first_inf = [None] * len(ARRAYS)
    clean = [True] * len(ARRAYS)
    for a, name in enumerate(ARRAYS):
        for i, x in enumerate(arr[a]):
            b = pic.raw.get((name, i))
            if b is not None:
                k = KA.element_verdict(GROUP[a], b)
                if k is not None:
                    bad_count[a][k] += 1
                    if first_bad[a][k] is None:
                        first_bad[a][k] = i
                    clean[a] = False
            elif x == 0 and first_inf[a] is None:
                first_inf[a], clean[a] = i, False
    z = pic.multipliers
    p = pic.ptau
    n = len(p["tauG2"])
    rel = [-1] * len(RELATIONS)
    rel[0] = 1 if all(clean) else 0
    form = lambda xs, T, m: sum(z[i] * (T * xs[i] - xs[i + 1]) for i in range(m)) % R == 0     # noqa: E731
    if clean[0] and clean[1]:
        rel[1] = int(p["tauG1"][0] == 1 and p["tauG2"][0] == 1)
        rel[2] = int(form(p["tauG1"], p["tauG2"][1], 2 * n - 2))
        rel[3] = int(form(p["tauG2"], p["tauG1"][1], n - 1))
    if clean[2] and clean[1]:
        rel[4] = int(form(p["alphaTauG1"], p["tauG2"][1], n - 1))
    if clean[3] and clean[1]:
        rel[5] = int(form(p["betaTauG1"], p["tauG2"][1], n - 1))
    if clean[3] and clean[4]:
        rel[6] = int(p["betaTauG1"][0] == p["betaG2"][0])
    first_record = [None, None]
    if pic.records is not None:
        recs = pic.records
        run_pok = all(clean[10:14])
        run_step = run_pok and all(clean[5:10])
        if run_pok:
            rel[7] = 1
            for j, r in enumerate(recs):
                if any((s * spx - sx * c) % R for (s, sx, spx), c in zip(r["pok"], pic.challenges[j])):
                    rel[7], first_record[0] = 0, j
                    break
        if run_step:
            rel[8] = 1
            for j, r in enumerate(recs):
                prev = recs[j - 1] if j else dict.fromkeys(REC, 1)
                ok = all((prev[k] * r["pok"][x][2] - r[k] * pic.challenges[j][x]) % R == 0 for x, k in enumerate(REC[:3]))
                ok = ok and all((r["pok"][x][1] * prev[k] - r["pok"][x][0] * r[k]) % R == 0 for x, k in ((0, "tauG2"), (2, "betaG2")))
                if not ok:
                    rel[8], first_record[1] = 0, j
                    break
        if all(clean[:10]):
            last = recs[-1] if recs else dict.fromkeys(REC, 1)
            rel[9] = int((p["tauG1"][1], p["alphaTauG1"][0], p["betaTauG1"][0], p["tauG2"][1], p["betaG2"][0]) ==
                         tuple(last[k] for k in REC))
    return {"failed": sum(1 << k for k, v in enumerate(rel) if v == 0), "relation": rel, "first_record": first_record,
            "first_bad": first_bad, "bad_count": bad_count, "first_infinity": first_inf}


def encode(pic, fixed):
    """-> (the five arrays as bytes, the 1216-byte records or None, the 384 challenge bytes per record)"""
    def pts(group, name, logs):
        psz = 64 if group == 1 else 128
        b = bytearray(fixed(group, tuple(logs))) if logs else bytearray()
        for (nm, i), raw in pic.raw.items():
            if nm == name:
                b[psz * i:psz * (i + 1)] = raw
        return bytes(b)
    arrays = {k: pts(GROUP[a], k, pic.ptau[k]) for a, k in enumerate(FILE)}
    if pic.records is None:
        return arrays, None, None
    recs, chs = [], []
    for j, r in enumerate(pic.records):
        g1 = pts(1, "", [r["tauG1"], r["alphaG1"], r["betaG1"]] + [v for x in range(3) for v in r["pok"][x][:2]])
        g2 = pts(2, "", [r["tauG2"], r["betaG2"]] + [r["pok"][x][2] for x in range(3)])
        rec = g1[:192] + g2[:256]
        for x in range(3):
            rec += g1[192 + 128 * x:320 + 128 * x] + g2[256 + 128 * x:384 + 128 * x]
        for (nm, i), raw in pic.raw.items():
            if nm == "g2_spx" and i // 3 == j:
                at = 448 + 256 * (i % 3) + 128
                rec = rec[:at] + raw + rec[at + 128:]
        recs.append(rec)
        chs.append(pts(2, "", pic.challenges[j]))
    return arrays, recs, chs


@functools.lru_cache(None)
def pictures():
    out = {}

    def add(name, pic):
        pic = copy.deepcopy(pic)
        pic.name = name
        pic.report = model(pic)
        out[name] = pic
        return pic
    for power in (3, 8):
        for k in (0, 1, 2):
            add(f"clean_p{power}_k{k}", chain(power, k))
    base = chain(3, 2)
    nochain = copy.deepcopy(base)
    nochain.records, nochain.challenges = None, []
    add("clean_no_records", nochain)
    m = len(base.ptau["tauG1"]) - 1                       # the last index: only ever in the shifted sum
    for k in (1, 7, m):
        pic = copy.deepcopy(base)
        pic.ptau["tauG1"][k] = pic.ptau["tauG1"][k] * 2 % R
        add(f"tauG1_{k}_doubled", pic)
    other = chain(3, 2, seed=555)
    pic = copy.deepcopy(base)
    pic.ptau["tauG2"] = list(other.ptau["tauG2"])         # another tau: TAU_G1, TAU_G2 fail, and ALPHA, BETA, which read tauG2[1]
    add("tauG2_on_another_tau", pic)
    pic = copy.deepcopy(base)
    pic.ptau["alphaTauG1"] = [base.ptau["alphaTauG1"][0] * x % R for x in other.ptau["tauG1"][:8]]
    add("alpha_on_another_tau", pic)
    pic = copy.deepcopy(base)
    pic.ptau["betaG2"] = [base.ptau["betaG2"][0] * 3 % R]
    add("betaG2_of_another_beta", pic)
    # two defects in the last two elements of tauG1, d and (T - 1) d: the form is (z_(m-1) - z_(m-2)) (T - 1) d
    T, d = base.ptau["tauG2"][1], 12345
    for tag, top in (("equal", 0), ("top_byte", 1 << 120)):
        pic = copy.deepcopy(base)
        pic.ptau["tauG1"][m - 1] = (pic.ptau["tauG1"][m - 1] + d) % R
        pic.ptau["tauG1"][m] = (pic.ptau["tauG1"][m] + (T - 1) * d) % R
        pic.multipliers[m - 2] = pic.multipliers[m - 1] ^ top
        add(f"cancelling_pair_{tag}", pic)
    pic = copy.deepcopy(base)
    pic.raw[("tauG2", 3)] = o.g2_to_bytes(KA.twist_outsiders()["small"])
    add("tauG2_3_outside_the_subgroup", pic)
    pic = copy.deepcopy(base)
    pic.ptau["alphaTauG1"][5] = 0
    add("alpha_5_infinity", pic)
    pic = copy.deepcopy(base)
    s, sx, spx = pic.records[1]["pok"][1]
    pic.records[1]["pok"][1] = (s, sx, spx * 2 % R)       # made with another secret
    add("pok_another_secret", pic)
    pic = copy.deepcopy(base)
    pic.records[0]["alphaG1"] = pic.records[0]["alphaG1"] * 5 % R     # after-values that skip a step
    add("step_skipped", pic)
    pic = copy.deepcopy(base)
    pic.records.reverse()
    pic.challenges.reverse()
    add("records_swapped", pic)
    pic = copy.deepcopy(base)
    pic.records, pic.challenges = pic.records[:1], pic.challenges[:1]
    add("last_is_not_the_files", pic)
    pic = copy.deepcopy(base)
    pic.ptau["tauG1"][0] = 2
    add("first_not_the_generator", pic)
    return out
