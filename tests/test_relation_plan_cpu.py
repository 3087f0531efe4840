"""relation_plan.hpp on the CPU: what the key audit, the circuit audit, the contribution chain and the ptau check decide
as data -- their arrays, which relation reads which array, run[], the fold of the product results into a report and
the finding texts -- held to the Python side of the same rules: the report tables of nim_groth16_amd/_lib.py and the
log-space models of the picture tests (phase1_pictures, phase2_pictures, circuit_audit_pictures, key_audit_pictures).

Everything comes from one run of a stand-alone program (tests/cpu_kernels/relation_plan_main.cpp) under
AddressSanitizer and UndefinedBehaviorSanitizer; nothing is loaded into this process."""
import os
import subprocess

import pytest

from nim_groth16_amd import _lib as L
from tests import circuit_audit_pictures as CA
from tests import key_audit_pictures as KA
from tests import phase1_pictures as P1
from tests import phase2_pictures as P2

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpu_kernels")
NEED_RECORDS, NEED_VK, NEED_MULTIPLIERS = 1, 2, 4
NONE = -1


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("relation_plan") / "relation_plan_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(HERE, "relation_plan_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
    out = {}
    for line in r.stdout.splitlines():
        kind, *rest = line.split("\t")
        out.setdefault(kind, []).append(rest)
    return out


def arrays_of(lines, checker):
    rows = [r for r in lines["array"] if r[0] == checker]
    assert [int(r[1]) for r in rows] == list(range(len(rows)))
    return [(r[2], int(r[3]), int(r[4])) for r in rows]               # name, group, scanned for (0,0)


def relations_of(lines, checker):
    rows = [r for r in lines["relation"] if r[0] == checker]
    assert [int(r[1]) for r in rows] == list(range(len(rows)))
    return [(int(r[2]), int(r[3]), int(r[4])) for r in rows]          # reads, need, failed


def mask(indices):
    return sum(1 << a for a in indices)


# ---- the relations as the models hold them: {relation index: (arrays read, need)} ---------------------------------------
def chain_reads():
    return {P2.RELATIONS.index(name): (mask(reads), 0) for name, reads in P2.READS.items()}


def ptau_reads():
    """the comment block of g16_ptau_verify (include/g16hip.h) and phase1_pictures.model"""
    r = P1.RELATIONS.index
    return {r("FIRST"): (mask((0, 1)), 0), r("TAU_G1"): (mask((0, 1)), 0), r("TAU_G2"): (mask((0, 1)), 0),
            r("ALPHA"): (mask((2, 1)), 0), r("BETA"): (mask((3, 1)), 0), r("BETA_G2"): (mask((3, 4)), 0),
            r("POK"): (mask(range(10, 14)), NEED_RECORDS), r("STEP"): (mask(range(5, 14)), NEED_RECORDS),
            r("LAST"): (mask(range(0, 10)), NEED_RECORDS)}


def circuit_reads():
    """key section s at bit s, ptau section p behind them"""
    nkey = len(CA.KEY_SECTIONS)
    out = {}
    for name, (key, ptau) in CA.READS.items():
        m = mask(CA.KEY_SECTIONS.index(s) for s in key) | mask(nkey + CA.PTAU_SECTIONS.index(s) for s in ptau)
        out[CA.RELATIONS.index(name)] = (m, NEED_VK if name == "IC" else 0)
    return out


def key_reads():
    """AUDIT_RELATIONS: "a~b" reads sections a and b; the batched one needs the multipliers"""
    out = {}
    for k, name in enumerate(L.AUDIT_RELATIONS):
        a, b = name.split("~")
        out[k] = (mask((KA.SECTIONS.index(a), KA.SECTIONS.index(b))), NEED_MULTIPLIERS if k == 0 else 0)
    return out


READS = {"key": key_reads, "circuit": circuit_reads, "chain": chain_reads, "ptau": ptau_reads}
NARRAYS = {"key": len(L.AUDIT_SECTIONS), "circuit": len(L.AUDIT_SECTIONS) + len(L.PTAU_SECTIONS),
           "chain": len(L.CHAIN_ARRAYS), "ptau": len(L.PTAU_REPORT_ARRAYS)}


# ---- arrays ---------------------------------------------------------------------------------------------------------------
def test_array_names_and_groups(lines):
    key = arrays_of(lines, "key")
    assert tuple(n for n, _, _ in key) == L.AUDIT_SECTIONS == KA.SECTIONS
    assert {n: g for n, g, _ in key if g} == KA.GROUP and [n for n, g, _ in key if not g] == ["coeffs"]
    assert [s for _, _, s in key] == [1] * 6 + [0] * 7                  # the spec points: spec_infinity
    circuit = arrays_of(lines, "circuit")
    assert tuple(n for n, _, _ in circuit) == L.PTAU_SECTIONS == CA.PTAU_SECTIONS
    assert {n: g for n, g, _ in circuit} == L.PTAU_GROUP == CA.PTAU_GROUP and not any(s for _, _, s in circuit)
    chain = arrays_of(lines, "chain")
    assert tuple(n for n, _, _ in chain) == L.CHAIN_ARRAYS == P2.ARRAYS
    assert tuple(g for _, g, _ in chain) == P2.ARRAY_GROUP
    assert [s for _, _, s in chain] == [1] * 7 + [0, 0]                 # up to the final delta2
    ptau = arrays_of(lines, "ptau")
    assert tuple(n for n, _, _ in ptau) == L.PTAU_REPORT_ARRAYS == P1.ARRAYS
    assert tuple(g for _, g, _ in ptau) == P1.GROUP and all(s for _, _, s in ptau)
    assert arrays_of(lines, "key_contribute") == [("delta1", 1, 0), ("delta2", 2, 0), ("pointsC1", 1, 0),
                                                  ("pointsH1", 1, 0), ("challenge", 2, 0)]
    file5 = [("ptau " + n, L.PTAU_GROUP[n]) for n in L.PTAU_SECTIONS]
    assert arrays_of(lines, "ptau_contribute") == [(n, g, 1) for n, g in file5] + [("challenges", 2, 1)]
    assert arrays_of(lines, "circuit_setup") == [(n, g, 0) for n, g in file5]


# ---- relations --------------------------------------------------------------------------------------------------------------
def test_read_masks_are_the_models(lines):
    for checker, model in READS.items():
        got = relations_of(lines, checker)
        want = model()
        assert {k: (r, n) for k, (r, n, _) in enumerate(got) if r or n} == want, checker
    assert relations_of(lines, "chain")[0][:2] == (0, 0) and relations_of(lines, "ptau")[0][:2] == (0, 0)    # ELEMENTS
    assert len(relations_of(lines, "key")) == len(L.AUDIT_RELATIONS)
    assert len(relations_of(lines, "circuit")) == len(L.CIRCUIT_RELATIONS) == len(CA.RELATIONS)
    assert len(relations_of(lines, "chain")) == len(L.CHAIN_RELATIONS) == len(P2.RELATIONS)
    assert len(relations_of(lines, "ptau")) == len(L.PTAU_RELATIONS) == len(P1.RELATIONS)


def test_failed_bits(lines):
    assert [f for _, _, f in relations_of(lines, "key")] == [L.AUDIT_RELATION] * 3
    assert [f for _, _, f in relations_of(lines, "circuit")] == [L.CIRCUIT_COEFFS] * 2 + [L.CIRCUIT_SPEC] + [L.CIRCUIT_POINTS] * 6
    assert [f for _, _, f in relations_of(lines, "chain")] == [1 << k for k in range(len(L.CHAIN_RELATIONS))]
    assert [f for _, _, f in relations_of(lines, "ptau")] == [1 << k for k in range(len(L.PTAU_RELATIONS))]
    # the last relation fails, the first was not run, the others hold
    assert sorted(lines["fold_fixed"]) == [["circuit", str(L.CIRCUIT_POINTS)], ["key", str(L.AUDIT_RELATION)]]


def test_run_for_every_single_dirty_array_and_every_flag(lines):
    seen = {c: set() for c in READS}
    for checker, clean, have, *run in lines["run"]:
        clean, have = int(clean), int(have)
        reads, n = READS[checker](), NARRAYS[checker]
        nrel = len(relations_of(lines, checker))
        dirty = [a for a in range(n) if not clean >> a & 1]
        assert len(dirty) <= 1
        want = [int(all(clean >> a & 1 for a in range(n) if reads.get(k, (0, 0))[0] >> a & 1) and
                    not reads.get(k, (0, 0))[1] & ~have) for k in range(nrel)]
        assert [int(x) for x in run] == want, (checker, dirty, have)
        seen[checker].add((tuple(dirty), have))
    for checker, cases in seen.items():
        assert cases == {(d, h) for d in [()] + [(a,) for a in range(NARRAYS[checker])] for h in (0, 1, 2, 4, 7)}, checker
    # with its flag off a gated relation is not run although every array is clean
    all_clean = {(c, int(h)): [int(x) for x in run] for c, clean, h, *run in lines["run"] if int(clean) + 1 == 1 << NARRAYS[c]}
    assert all_clean[("ptau", 0)] == [1] * 7 + [0, 0, 0] and all_clean[("ptau", NEED_RECORDS)] == [1] * 10
    assert all_clean[("circuit", 0)] == [1] * 7 + [0, 1] and all_clean[("circuit", NEED_VK)] == [1] * 9
    assert all_clean[("key", 0)] == [0, 1, 1] and all_clean[("key", NEED_MULTIPLIERS)] == [1, 1, 1]
    assert all_clean[("chain", 0)] == [1] * 7


# ---- fold_report --------------------------------------------------------------------------------------------------------------
def record_rows(checker, j):
    """the rows of record j, counted from the first row of record 0 -> (POK rows, STEP rows), by the index arithmetic of
    the two verifiers: POK_j at 2j and STEP_j at 2j + 1 of the chain; 8 rows per ptau record, POK 0..2 and STEP 3..7"""
    if checker == "chain":
        return [2 * j], [2 * j + 1]
    return [8 * j + q for q in range(3)], [8 * j + q for q in range(3, 8)]


def test_fold_report(lines):
    cases = set()
    for checker, count, not_run, zeros, failed, first0, first1, *relation in lines["fold"]:
        count, not_run = int(count), int(not_run)
        zeros = {int(z) for z in zeros.split(",") if z}
        names = (L.CHAIN_RELATIONS if checker == "chain" else L.PTAU_RELATIONS)
        pok, step = names.index("POK"), names.index("STEP")
        want_rel, want_first, want_failed = [1] * len(names), [NONE, NONE], 0
        for which, k in enumerate((pok, step)):
            if k == not_run:
                want_rel[k] = -1
                continue
            bad = [j for j in range(count) if zeros & set(record_rows(checker, j)[which])]
            if bad:
                want_rel[k], want_first[which], want_failed = 0, bad[0], want_failed | 1 << k
        assert ([int(x) for x in relation], [int(first0), int(first1)], int(failed)) == (want_rel, want_first, want_failed), \
            (checker, count, not_run, sorted(zeros))
        cases.add((checker, count, not_run, len(zeros) > 1))
        if len(zeros) == 1:
            cases.add((checker, count, "row", min(zeros) % (2 if checker == "chain" else 8)))
    for checker, per_record in (("chain", 2), ("ptau", 8)):
        assert {(checker, n, -1, False) for n in (0, 1, 3)} <= cases
        assert {(checker, n, k, True) for n in (3,) for k in (-1, 1 if checker == "chain" else 7, 2 if checker == "chain" else 8)} <= cases
        assert {(checker, n, "row", q) for n in (1, 3) for q in range(per_record)} <= cases


# ---- findings -------------------------------------------------------------------------------------------------------------------
def test_finding_texts_are_those_of_the_reports(lines):
    seen = set()
    for name, first, check, count, text in lines["finding"]:
        first, check, count = int(first), int(check), int(count)
        prefix, bare = ("ptau ", name[5:]) if name.startswith("ptau ") else ("", name)
        bad_count = [[0, 0, 0]]
        first_bad = [[None, None, None]]
        bad_count[0][check], first_bad[0][check] = count, first
        assert L._element_findings((bare,), first_bad, bad_count, prefix=prefix) == [text]
        assert L._element_findings((bare,), first_bad, bad_count, [None], prefix) == [text]
        seen.add((prefix, first, check, count))
    assert seen == {(p, f, k, c) for p in ("", "ptau ") for f in (0, 7, 123456789012) for k in range(3) for c in (1, 2, 17)}
    for name, first, text in lines["infinity"]:
        prefix, bare = ("ptau ", name[5:]) if name.startswith("ptau ") else ("", name)
        assert L._element_findings((bare,), [[None] * 3], [[0] * 3], [int(first)], prefix) == [text]
    assert len(lines["infinity"]) == 9
    assert text.endswith("[123456789012] is the point at infinity")
    # (0,0) is 64 or 128 zero bytes: a one in the last byte, a clean point, a one inside a G2 point, a clean G2 point
    assert lines["is_infinity"] == [["0", "1", "0", "1"]]


def test_reports_spell_their_findings_as_before():
    """the four report classes through the one helper: the lines of findings() for one defect of each kind"""
    n = None
    key = L.KeyReport(1 | 16, 1 << 3, [1, 0, -1], [[n] * 3] * 7 + [[5, n, 9]] + [[n] * 3] * 5,
                      [[0] * 3] * 7 + [[1, 0, 3]] + [[0] * 3] * 5)
    assert key.findings() == ["pointsA1[5] is not a canonical encoding", "pointsA1[9] is not in the order-r subgroup (and 2 more)",
                              "beta1~beta2: not the same multiples of the two generators", "beta2 is the point at infinity"]
    circuit = L.CircuitReport(key, [[n] * 3, [n, 2, n]] + [[n] * 3] * 3, [[0] * 3, [0, 17, 0]] + [[0] * 3] * 3,
                              [1] * 9, 3, [n, n])
    assert circuit.findings() == key.findings() + ["ptau tauG2[2] is not on the curve (and 16 more)"]
    ptau = L.PtauReport(1, [0] + [1] * 9, [n, n], [[n] * 3] * 13 + [[n, n, 4]], [[0] * 3] * 13 + [[0, 0, 1]],
                        [n] * 12 + [0, n])
    assert ptau.findings() == ["g2_spx[0] is the point at infinity", "challenges[4] is not in the order-r subgroup"]
    chain = L.ChainReport(1, [0] + [1] * 6, [n, n], [[0, n, n]] + [[n] * 3] * 8, [[2, 0, 0]] + [[0] * 3] * 8, [1] + [n] * 8)
    assert chain.findings() == ["delta_after[0] is not a canonical encoding (and 1 more)",
                                "delta_after[1] is the point at infinity"]
