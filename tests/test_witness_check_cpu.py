"""The witness check without a GPU: the C ABI declares it and the binding lists it, the integer model of
tests/witness_pictures.py agrees with synthetic.checkWitness and with the oracle's toy circuit, and the list selection of
witness_plan.hpp (the function the list kernel walks the bitmap with) is held to a sort, as a stand-alone program under
AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import re
import subprocess

import pytest

from oracle import bn254_ref as o
from tests import witness_pictures as WP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "cpu_kernels")
NAMES = ("g16_r1cs_create", "g16_r1cs_destroy", "g16_r1cs_info", "g16_witness_check")
NONE = 0xffffffff


def test_header_declares_and_binding_lists_the_calls():
    from nim_groth16_amd._lib import SYMBOLS
    text = open(os.path.join(ROOT, "include", "g16hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b(int32_t|void)\s+%s\s*\(" % name, code), f"{name} has no prototype in include/g16hip.h"
        assert name in SYMBOLS, f"{name} is missing from SYMBOLS"
    for macro, value in (("G16_WITNESS_CANONICAL", "1u"), ("G16_WITNESS_ONE", "2u"), ("G16_WITNESS_CONSTRAINTS", "4u"),
                         ("G16_WITNESS_LIST", "16")):
        assert re.search(r"#define\s+%s\s+%s\b" % (macro, value), code), macro
    assert "g16_witness_report" in code and "typedef struct g16_r1cs g16_r1cs;" in code


def test_report_struct_matches_the_header_layout():
    import ctypes

    from nim_groth16_amd._lib import WITNESS_LIST, WitnessReportC
    sz = ctypes.sizeof(ctypes.c_size_t)
    assert WITNESS_LIST == 16
    assert WitnessReportC.noncanonical_count.offset == 8 and WitnessReportC.first_bad.offset == 8 + 3 * sz
    assert ctypes.sizeof(WitnessReportC) == 8 + 3 * sz + 16 * sz + 96


def _pictures():
    """(name, circuit, residue witness): every planted picture of the GPU test at its smallest sizes, and the operands"""
    out = []
    for n in (1, 31, 33, 65):
        for many in (False, True):
            pc = WP.planted(WP.plain_specs(n), seed=n, many_values=many, pad_to=0 if many else 1100)
            for name, which in WP.sizes_pictures(pc).items():
                out.append((f"{n}_{many}_{name}", pc.circuit, WP.broken(pc, which), set(which)))
    pc = WP.planted(WP.bin_specs(), seed=9, nbase=40)
    out.append(("bins", pc.circuit, pc.witness, set()))
    some = sorted(pc.fresh)[::5]
    out.append(("bins_broken", pc.circuit, WP.broken(pc, some), set(some)))
    c, z = WP.operands()
    out.append(("operands", c, z, {1, 2, 6}))
    return out


def test_model_agrees_with_synthetic_check_witness():
    from nim_groth16_amd.synthetic import checkWitness
    for name, c, z, want_bad in _pictures():
        for form in (WP.MONT, WP.STD):
            rep = WP.model(c, z, form)
            assert rep["noncanonical_count"] == 0 and not rep["failed"] & WP.F_ONE, name
            bad = [i for i in range(c.ncons) if not checkWitness(c, z, rows=[i])]
            assert set(bad) == want_bad, name
            assert rep["bad_count"] == len(bad) and rep["first_bad"] == bad[:16], name
            assert (rep["constraints"] == 1) == checkWitness(c, z) == (rep["failed"] == 0), name
            if bad:
                A, B, C = c.constraints[bad[0]]
                assert (rep["az"], rep["bz"], rep["cz"]) == (WP.lc(A, z), WP.lc(B, z), WP.lc(C, z))
            else:
                assert (rep["az"], rep["bz"], rep["cz"]) == (0, 0, 0)


def test_model_on_the_oracle_toy_circuit():
    from tests.circuit_audit_pictures import circuits
    toy = o.toy_r1cs()
    c = circuits()["toy"]
    assert c.constraints == toy.constraints
    for form in (WP.MONT, WP.STD):
        assert WP.model(c, o.TOY_WITNESS, form)["failed"] == 0
        z = list(o.TOY_WITNESS)
        z[6] += 1                                  # 7 * 11: constraints 1 (its C) and 2 (its B)
        rep = WP.model(c, z, form)
        assert rep["first_bad"] == [1, 2] and rep["failed"] == WP.F_CONSTRAINTS
        assert (rep["az"], rep["bz"], rep["cz"]) == (7, 11, 78)


def test_model_canonical_precedence_and_one():
    c, z = WP.operands()
    for form in (WP.MONT, WP.STD):
        raw = bytearray(WP.encode(z, form))
        raw[32 * 3:32 * 4] = o.R.to_bytes(32, "little")
        raw[32 * 4:32 * 5] = b"\xff" * 32
        rep = WP.model(c, bytes(raw), form)
        assert rep == {"failed": WP.F_CANONICAL, "constraints": -1, "noncanonical_count": 2, "first_noncanonical": 3,
                       "bad_count": 0, "first_bad": [], "az": 0, "bz": 0, "cz": 0}
    rep = WP.model(c, WP.encode([(1 + o.R).to_bytes(32, "little")] + z[1:], WP.STD), WP.STD)
    assert rep["failed"] == WP.F_CANONICAL | WP.F_ONE and rep["first_noncanonical"] == 0
    rep = WP.model(c, [2] + z[1:], WP.STD)
    assert rep["failed"] == WP.F_ONE | WP.F_CONSTRAINTS and rep["constraints"] == 0 and rep["bad_count"] == 3
    # the Montgomery pattern of the standard 1 is not the Montgomery 1
    assert WP.model(c, WP.encode(z, WP.STD), WP.MONT)["failed"] & WP.F_ONE


# ---- the list selection ------------------------------------------------------------------------------------------------
def _cases():
    """(constraints, lanes, set bits): sizes 0, 1, 15, 16, 17 and all; bits at word, trip and workgroup edges"""
    cases = []
    for ncons in (1, 63, 64, 65, 257, 1000, 64 * 256 - 1, 64 * 256, 64 * 256 + 1, 3 * 64 * 256 + 77):
        edges = sorted({i for b in (0, 64, 128, 256, 64 * 255, 64 * 256, 2 * 64 * 256, ncons) for i in (b - 1, b, b + 1)
                        if 0 <= i < ncons})
        sets = [[], [0], [ncons - 1], edges, list(range(ncons)), list(range(ncons - 1, -1, -7))]
        for k in (15, 16, 17):
            if k <= ncons:
                sets.append(list(range(k)))                                  # the first words settle it
                sets.append(list(range(ncons - k, ncons)))                   # ... the last ones
                sets.append(sorted({j * (ncons - 1) // (k - 1) for j in range(k)}))
        sets += [[e] for e in edges]
        for lanes in (256, 4, 1):
            if lanes == 256 or ncons <= 1000:
                cases += [(ncons, lanes, sorted(set(s))) for s in sets]
    return cases


def test_list_selection_is_a_sort(tmp_path):
    exe = str(tmp_path / "witness_plan_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(HERE, "witness_plan_main.cpp"), "-o", exe])
    cases = _cases()
    text = "".join(f"{n} {lanes} {len(s)} " + " ".join(map(str, s)) + "\n" for n, lanes, s in cases)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-4000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    for (n, lanes, s), line in zip(cases, lines):
        read, *got = map(int, line.split())
        want = sorted(s)[:16]
        assert got == want + [NONE] * (16 - len(want)), (n, lanes, s[:20])
        nwords = (n + 63) // 64
        if len(s) >= 16:                           # early exit: no trip is started after the one that holds the 16th
            trip = s[15] // 64 // lanes
            assert read == min((trip + 1) * lanes, nwords), (n, lanes)
        else:
            assert read == nwords, (n, lanes)


@pytest.mark.parametrize("name", ["witness_check.hip", "witness_plan.hpp"])
def test_unit_is_part_of_the_build(name):
    assert os.path.exists(os.path.join(ROOT, "nim_groth16_amd", "csrc", name))
    mk = open(os.path.join(ROOT, "nim_groth16_amd", "csrc", "Makefile")).read()
    assert "witness_check.o" in mk and "witness_plan.hpp" in mk
