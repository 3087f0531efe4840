"""The integer model of the circuit audit (tests/circuit_audit_pictures.py) held to itself, the header's declaration of
the call, and the .ptau reader and writer.  No GPU."""
import os
import re
import struct

import pytest

from oracle import bn254_ref as o
from tests import circuit_audit_pictures as CA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = o.R


def horner(cs, x):
    acc = 0
    for c in reversed(cs):
        acc = (acc * x + c) % R
    return acc


@pytest.mark.parametrize("circuit", list(CA.circuits()))
@pytest.mark.parametrize("flavour", [CA.SNARKJS, CA.JENSGROTH])
def test_clean_key_every_form_is_zero(circuit, flavour):
    """the oracle's own setup in log space against the powers of its own tau"""
    pic = CA.base(circuit, flavour)
    fm = CA.forms(pic)
    assert fm["COEFFS_A"] == (0, None) and fm["COEFFS_B"] == (0, None)
    assert all(fm[name] == 0 for name in CA.RELATIONS[2:]), fm
    rep = CA.model(pic)
    assert rep["relation"] == [1] * 9 and rep["failed"] == 0 and rep["first_row"] == [None, None]
    assert rep["key"]["failed"] == 0 and rep["key"]["relation"] == [1, 1, 1]
    # other multipliers, the same verdict
    pic.zw = [z ^ 0x55 or 1 for z in pic.zw]
    pic.zh = [z ^ 0xaa or 1 for z in pic.zh]
    assert CA.model(pic)["failed"] == 0


@pytest.mark.parametrize("circuit", ["toy", "dup", "nopriv", "chain"])
def test_coefficients_are_the_polynomials_at_tau(circuit):
    """sum_i z_i A_i(tau) == Horner at tau of coef_n(A z), in plain integers; the same for the H vector of both
    flavours against the definitions of pointsH1 (fake_setup.nim:290-304)"""
    pic, tw = CA._base(circuit, CA.SNARKJS)
    n, tau = pic.n, tw.tau % R
    D = o.Domain(n)
    lag = [o.eval_lagrange_poly_at(D, k, tau) for k in range(n)]
    for k in range(3):
        ent = CA.with_dummies(pic, k)
        col = [0] * pic.nvars                                    # A_i(tau) = sum over column i of value * L_row(tau)
        for row, w, v in ent:
            col[w] = (col[w] + v * lag[row]) % R
        assert CA.dot(pic.zw, col) == horner(CA.coef(CA.matvec(ent, pic.zw, n)), tau)
        if k == 0:
            assert col == pic.key["pointsA1"]
        if k == 1:
            assert col == pic.key["pointsB1"] == pic.key["pointsB2"]
    D2 = o.Domain(2 * n)
    sn = sum(y * o.eval_lagrange_poly_at(D2, 2 * i + 1, tau) for i, y in enumerate(pic.zh)) % R
    assert sn == horner(CA.h_coefficients(CA.SNARKJS, pic.zh), tau)
    z_tau = (pow(tau, n, R) - 1) % R
    jg = sum(y * pow(tau, i, R) for i, y in enumerate(pic.zh)) * z_tau % R
    assert jg == horner(CA.h_coefficients(CA.JENSGROTH, pic.zh), tau)
    # the ptau is the powers of that tau
    assert pic.ptau["tauG1"][:4] == [1, tau, tau * tau % R, pow(tau, 3, R)] and len(pic.ptau["tauG1"]) == 4 * n - 1
    assert horner(CA.coef(CA.matvec(CA.with_dummies(pic, 0), pic.zw, n)), tau) == \
        CA.dot(CA.coef(CA.matvec(CA.with_dummies(pic, 0), pic.zw, n)), pic.ptau["tauG1"])


def test_pictures_cover_the_issue():
    pics = CA.pictures()
    assert len({p.name for p in pics.values()}) == len(pics) > 50
    assert {p.circuit for p in pics.values()} == set(CA.circuits())
    # each defect changes exactly its relations (the builder asserts the verdicts); here: the bits of `failed`
    for name, p in pics.items():
        rel, want = p.report["relation"], 0
        want |= CA.F_KEY if p.report["key"]["failed"] else 0
        want |= CA.F_PTAU if any(c != [0, 0, 0] for c in p.report["ptau_bad_count"]) else 0
        want |= CA.F_COEFFS if 0 in rel[:2] else 0
        want |= CA.F_SPEC if rel[2] == 0 else 0
        want |= CA.F_POINTS if 0 in rel[3:] else 0
        assert p.report["failed"] == want, name
        assert all(z and z <= CA.Z_MAX for z in p.zw + p.zh), name
    # the duplicated pair and the cancelling pair are in the r1cs the library is handed
    dup = pics["clean_dup_sn"]
    assert len({(i, w) for i, w, _ in dup.r1cs[0]}) == len(dup.r1cs[0]) - 1
    assert sorted(v for i, w, v in dup.r1cs[1] if (i, w) == (2, 4)) == [5, R - 5]
    assert pics["clean_nopriv_sn"].key["pointsC1"] == [] and pics["clean_nopriv_sn"].report["relation"][6] == 1
    assert pics["clean_chain_sn"].nvars == 512 and pics["clean_chain_sn"].n == 512
    # the cancellation pair differs from its failing twin in one bit of one multiplier
    a, b = pics["a1_cancel_chain"], pics["a1_cancel_bit127_chain"]
    assert [x ^ y for x, y in zip(a.zw, b.zw) if x != y] == [1 << 127]


def test_header_declares_the_call():
    text = open(os.path.join(ROOT, "include", "g16hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint32_t\s+g16_circuit_audit\s*\(", code)
    for word in ("g16_r1cs_desc", "g16_ptau_desc", "g16_circuit_report", "G16_CIRCUIT_RELATIONS"):
        assert word in code, word
    assert "g16_circuit_audit" in text[text.index("CANNOT establish"):text.index("int32_t g16_key_audit")]
    assert "1/(2^128 - 1)" in text[text.index("circuit audit:"):] and "contribution chain" in text
    from nim_groth16_amd import _lib
    assert _lib.CIRCUIT_RELATIONS == CA.RELATIONS and _lib.PTAU_SECTIONS == CA.PTAU_SECTIONS
    enums = re.findall(r"enum\s*\{(.*?)\}", code, flags=re.S)
    names = lambda body: [x.split("=")[0].strip() for x in body.split(",")]        # noqa: E731
    assert names(enums[0])[0] == "G16_SEC_ALPHA1"                                  # the sections' enum stays first
    assert names(enums[1]) == ["G16_PTAU_" + re.sub(r"(?<=[a-z])(?=[A-Z])", "_", s).upper() for s in CA.PTAU_SECTIONS]
    assert names(enums[2]) == ["G16_REL_" + s for s in CA.RELATIONS]
    assert int(re.search(r"#define\s+G16_CIRCUIT_RELATIONS\s+(\d+)", code).group(1)) == len(CA.RELATIONS)
    assert (_lib.CIRCUIT_KEY, _lib.CIRCUIT_PTAU, _lib.CIRCUIT_COEFFS, _lib.CIRCUIT_SPEC, _lib.CIRCUIT_POINTS) == \
        (CA.F_KEY, CA.F_PTAU, CA.F_COEFFS, CA.F_SPEC, CA.F_POINTS)
    assert "g16_circuit_audit" in _lib.SYMBOLS


def _ptau(power=2):
    from nim_groth16_amd.files.ptau import Ptau
    rng = o.SplitMix64(12)
    blob = lambda k: b"".join(rng.fr().to_bytes(32, "little") for _ in range(k // 32))     # noqa: E731
    return Ptau(power, blob(64 * ((2 << power) - 1)), blob(128 << power), blob(64 << power), blob(64 << power), blob(128))


def test_ptau_round_trip(tmp_path):
    from nim_groth16_amd.files import parsePtau, writePtau
    pt = _ptau()
    path = str(tmp_path / "a.ptau")
    writePtau(path, pt)
    got = parsePtau(path)
    assert got.power == 2 and got.ceremonyPower == 2
    for name in CA.PTAU_SECTIONS:
        assert getattr(got, name) == getattr(pt, name), name
    assert open(path, "rb").read(4) == b"ptau"
    # a file of a real ceremony carries its contributions (7) and, once prepared, the Lagrange forms (12-15): skipped
    pt.ceremonyPower = 5
    writePtau(path, pt, extraSections=[(7, b"\x01" * 77), (12, b"\x02" * 640)])
    got = parsePtau(path)
    assert got.ceremonyPower == 5 and got.tauG1 == pt.tauG1 and got.betaG2 == pt.betaG2


def test_ptau_rejects_damaged_files(tmp_path):
    from nim_groth16_amd.files import parsePtau, writePtau
    from nim_groth16_amd.files.container import writeContainer
    pt = _ptau()
    path = str(tmp_path / "a.ptau")
    writePtau(path, pt)
    whole = open(path, "rb").read()
    open(path, "wb").write(whole[:-40])                           # the last section runs past the end of the file
    with pytest.raises(AssertionError, match="truncated section"):
        parsePtau(path)
    s1 = struct.pack("<I", 32) + o.P.to_bytes(32, "little") + struct.pack("<II", 2, 2)
    secs = [(1, s1), (2, pt.tauG1), (3, pt.tauG2[:-128]), (4, pt.alphaTauG1), (5, pt.betaTauG1), (6, pt.betaG2)]
    writeContainer("ptau", 1, path, secs)                         # tauG2 one point short
    with pytest.raises(AssertionError, match=r"section 3 \(tauG2\)"):
        parsePtau(path)
    secs[2] = (3, pt.tauG2)
    writeContainer("ptau", 1, path, secs[:4] + secs[5:])          # betaTauG1 missing
    with pytest.raises(AssertionError, match="section 5"):
        parsePtau(path)
    writeContainer("zkey", 1, path, secs)
    with pytest.raises(AssertionError, match="not a `ptau` file"):
        parsePtau(path)
