"""The per-point scaling, the parts that need no GPU: the split a lane makes of its own scalar and the lane arithmetic of
scale_each.cuh, built with g++ (tests/cpu_kernels/scale_each_shim.cpp), against Python integers and the oracle; the header
and the binding list."""
import ctypes
import os
import re
import subprocess

import pytest

from oracle import bn254_ref as o
from tests import inputs as I
from tests import phase1_scalars as PS
from tests import phase2_pictures as PP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = o.R
SHIM_DIR = os.path.join(ROOT, "tests", "cpu_kernels")


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(SHIM_DIR, "libscale_each_shim.so")
    src = os.path.join(SHIM_DIR, "scale_each_shim.cpp")
    if not os.path.exists(so):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", src, "-o", so])
    return ctypes.CDLL(so)


@pytest.fixture(scope="module")
def scalars():
    return PS.edge_scalars() + PS.powers_of_two() + PS.random_scalars(3000, 31)


def o_fixed(group, logs):
    from tests.oracle_c import load_oracle
    return load_oracle().fixed_base(group, I.fr_mont_bytes(list(logs)))


def each(shim, group, pts, ks, mont=False):
    n = len(ks)
    buf = ctypes.create_string_buffer(pts, max(1, len(pts)))
    kb = I.fr_mont_bytes(ks) if mont else I.fr_std_bytes(ks)
    fn = shim.shim_each_points_g1 if group == 1 else shim.shim_each_points_g2
    fn(buf, ctypes.c_uint64(n), kb, ctypes.c_uint32(1 if mont else 0), buf)          # in place
    return buf.raw[:len(pts)]


def test_header_and_symbols():
    from nim_groth16_amd._lib import SYMBOLS
    text = " ".join(open(os.path.join(ROOT, "include", "g16hip.h")).read().replace(" * ", " ").split())
    for name in ("g16_points_scale_each_g1", "g16_points_scale_each_g2"):
        assert re.search(r"int32_t " + name + r"\(g16_ctx\* ctx, const void\* points, size_t n, const void\* scalars, "
                         r"uint32_t flags, void\* out\)", text), name
        assert name in SYMBOLS
    at = text.index("scaling an array of points")
    for word in ("A scalar PER POINT", "k = k1 + k2 lambda on the device", "is not canonical (>= r)"):
        assert word in text[at:], word
    mk = open(os.path.join(ROOT, "nim_groth16_amd", "csrc", "Makefile")).read()
    assert "scale_each_g1.o" in mk and "scale_each_g2.o" in mk


def test_split_identity_and_bound(shim, scalars):
    """k1 + k2 lambda == k (mod r) and |k1|, |k2| < 2^128 for every scalar; the halves are exactly those of the host's
    scale_split (the same rounding), which tests/test_phase2_cpu.py holds on its own"""
    n = len(scalars)
    assert n > 3300 and len(set(scalars)) > 3290
    halves, signs = (ctypes.c_uint64 * (4 * n))(), (ctypes.c_uint32 * n)()
    shim.shim_each_split(I.fr_std_bytes(scalars), ctypes.c_uint64(n), halves, signs)
    longest = 0
    for i, k in enumerate(scalars):
        assert signs[i] < 4, f"{k:#x}: a half does not fit 128 bits"
        k1, k2 = halves[4 * i] | halves[4 * i + 1] << 64, halves[4 * i + 2] | halves[4 * i + 3] << 64
        assert k1 < 1 << 128 and k2 < 1 << 128
        s1, s2 = (-1 if signs[i] & 1 else 1), (-1 if signs[i] & 2 else 1)
        assert (s1 * k1 + s2 * k2 * PP.LAMBDA - k) % R == 0, hex(k)
        # Babai rounding DOWN with quotients that fall short by less than 2 (scale_plan.hpp): within two basis vectors
        # of the exact rounding of the Python model
        e1, e2 = PP.split(k)
        (a1, b1), (a2, b2) = PP.lattice_basis()
        assert any((s1 * k1 - e1, s2 * k2 - e2) == (x * a1 + y * a2, x * b1 + y * b2) for x in (0, 1, 2) for y in (0, 1, 2))
        longest = max(longest, k1, k2)
    assert longest >= 48 * (1 << 128) // 100
    so = os.path.join(SHIM_DIR, "libscale_plan_shim.so")
    if not os.path.exists(so):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC",
                               os.path.join(SHIM_DIR, "scale_plan_shim.cpp"), "-o", so])
    host = ctypes.CDLL(so)
    for i, k in enumerate(scalars):
        h, s = (ctypes.c_uint64 * 4)(), ctypes.c_uint32()
        assert host.shim_scale_split(k.to_bytes(32, "little"), h, ctypes.byref(s)) == 1
        assert list(h) == list(halves[4 * i:4 * i + 4]) and s.value == signs[i], hex(k)


def test_ladder_g1_against_the_oracle(shim, scalars):
    """k_i * P_i for every scalar, the points random multiples of gen1 with (0,0) at every 7th place and filling one lane's
    group of four (lane 9 of the second workgroup: 256 + 9 + 64 j); in place; both scalar forms"""
    n = len(scalars)
    rng = o.SplitMix64(77)
    logs = [0 if i % 7 == 3 or i in (265, 329, 393, 457) else rng.fr() for i in range(n)]
    pts = o_fixed(1, logs)
    exp = o_fixed(1, [k * x % R for k, x in zip(scalars, logs)])
    got = each(shim, 1, pts, scalars)
    for i in range(n):
        assert got[64 * i:64 * i + 64] == exp[64 * i:64 * i + 64], f"point {i}, k = {scalars[i]:#x}"
    assert each(shim, 1, pts[:64 * 300], scalars[:300], mont=True) == exp[:64 * 300]
    # every point the same, every lane another scalar, and the other way round
    one = o_fixed(1, [5])
    assert each(shim, 1, one * 254, PS.powers_of_two()) == o_fixed(1, [5 << i for i in range(254)])
    k = scalars[-1]
    assert each(shim, 1, pts[:64 * 70], [k] * 70) == o_fixed(1, [k * x % R for x in logs[:70]])
    assert each(shim, 1, pts[:64 * 70], [0] * 70) == bytes(64 * 70)
    assert each(shim, 1, b"", []) == b""
    # straight against the Python oracle's ladder
    for i in (0, 1, n - 1):
        p = o.g1_from_bytes(pts[64 * i:64 * i + 64])
        assert o.g1_from_bytes(got[64 * i:64 * i + 64]) == o.G1.mul(scalars[i], p)


def test_ladder_g2_against_the_oracle(shim):
    ks = PS.edge_scalars() + PS.random_scalars(8, 32)
    rng = o.SplitMix64(78)
    logs = [0 if i % 5 == 2 else rng.fr() for i in range(len(ks))]
    pts = o_fixed(2, logs)
    exp = o_fixed(2, [k * x % R for k, x in zip(ks, logs)])
    assert each(shim, 2, pts, ks) == exp
    assert each(shim, 2, pts, ks, mont=True) == exp
    i = len(ks) - 1
    assert o.g2_from_bytes(exp[128 * i:128 * i + 128]) == o.G2.mul(ks[i], o.g2_from_bytes(pts[128 * i:128 * i + 128]))


# ---- g16_ptau_contribute: the header, the record, section 7 of a .ptau, the transcript ---------------------------------------
def test_ptau_contribute_header_and_record():
    from nim_groth16_amd import _lib
    text = " ".join(open(os.path.join(ROOT, "include", "g16hip.h")).read().replace(" * ", " ").split())
    assert re.search(r"int32_t g16_ptau_contribute\(g16_ctx\* ctx, const g16_ptau_desc\* ptau, const void\* t, const void\* a, "
                     r"const void\* b, const void\* s3, uint32_t flags, const void\* challenges_g2, g16_ptau_out\* out, "
                     r"g16_ptau_contribution\* record\)", text)
    assert "g16_ptau_contribute" in _lib.SYMBOLS
    at = text.index("phase-1 contribution: powers of tau nobody knows")
    for word in ("g16_ptau_out", "g16_ptau_contribution", "1216 bytes", "ptau tauG2[3] is not in the order-r subgroup",
                 "power > 25", "640 MiB", "one wait after the element passes and one at the end"):
        assert word in text[at:], word
    assert ctypes.sizeof(_lib.PtauContributionC) == 1216 == _lib.PTAU_CONTRIBUTION_BYTES
    f = _lib.PtauContributionC
    assert (f.tauG1.offset, f.alphaG1.offset, f.betaG1.offset, f.tauG2.offset, f.betaG2.offset, f.pok.offset) == \
        (0, 64, 128, 192, 320, 448)
    assert ctypes.sizeof(_lib.PtauOut) == 5 * ctypes.sizeof(ctypes.c_void_p)
    src = open(os.path.join(ROOT, "nim_groth16_amd", "csrc", "ptau.hip")).read()
    assert "sizeof(g16_ptau_contribution) == 1216" in src


def test_new_ptau_is_all_generators():
    from nim_groth16_amd import phase1
    assert phase1.GEN2 == o.GEN2 and phase1.GEN1 == o.GEN1
    assert phase1.gen1_bytes() == o_fixed(1, [1]) and phase1.gen2_bytes() == o_fixed(2, [1])
    pt = phase1.newPtau(2)
    assert (pt.power, pt.tauG1, pt.tauG2, pt.alphaTauG1, pt.betaTauG1, pt.betaG2) == \
        (2, o_fixed(1, [1] * 7), o_fixed(2, [1] * 4), o_fixed(1, [1] * 4), o_fixed(1, [1] * 4), o_fixed(2, [1]))
    for power in (0, 26):
        with pytest.raises(ValueError, match="power must lie"):
            phase1.newPtau(power)


def test_section_7_round_trip(tmp_path):
    from nim_groth16_amd import phase1
    from nim_groth16_amd.files import contributionsSection, parsePtau, parsePtauContributions, writePtau
    from nim_groth16_amd.files.container import parseContainer, writeContainer
    pt = phase1.newPtau(1)
    path = str(tmp_path / "a.ptau")
    writePtau(path, pt)
    plain = open(path, "rb").read()
    assert parsePtauContributions(path) is None
    records, names = [bytes([j + 1]) * 1216 for j in range(3)], ["first", "", "third é"]
    writePtau(path, pt, extraSections=[(7, contributionsSection(records, names))])
    data = open(path, "rb").read()
    assert data[12:len(plain)] == plain[12:] and len(data) == len(plain) + 12 + 4 + 3 * 1216 + 3 * 4 + 5 + 0 + 8
    assert parsePtauContributions(path) == (records, names)
    back = parsePtau(path)                                                        # the reader of sections 2-6 skips it
    assert (back.tauG1, back.tauG2, back.betaG2, back.power) == (pt.tauG1, pt.tauG2, pt.betaG2, 1)
    sec = parseContainer("ptau", 1, path)
    s7 = bytes(sec[7][0])
    others = [(sid, bytes(v[0])) for sid, v in sorted(sec.items()) if sid != 7]
    for bad, match in ((s7[:3], "shorter"), (s7[:2000], "inside its records"), (s7[:-1], "inside its names"),
                       (s7 + b"x", "left over"), (s7[:-2] + b"\xff\xfe", "UTF-8"), (b"contributions", "truncated")):
        p2 = str(tmp_path / "bad.ptau")
        writeContainer("ptau", 1, p2, others + [(7, bad)])
        with pytest.raises(ValueError, match=match):
            parsePtauContributions(p2)
        parsePtau(p2)
    with pytest.raises(AssertionError):
        contributionsSection([bytes(1215)], [""])


def test_transcript_is_deterministic_and_binds_everything():
    from nim_groth16_amd import phase1
    pok = bytes(range(256)) + bytes(128)
    log = phase1.PtauContributions(power=3)
    tr = phase1.transcript_hash(log, 0, pok)
    assert len(tr) == 64 and tr == phase1.transcript_hash(phase1.PtauContributions(power=3), 0, pok)
    assert tr != phase1.transcript_hash(phase1.PtauContributions(power=4), 0, pok)
    assert tr != phase1.transcript_hash(log, 0, pok[:-1] + b"\x01")
    rec = bytes(448) + pok[:128] + bytes(128) + pok[128:256] + bytes(128) + pok[256:] + bytes(128)
    assert len(rec) == 1216 and phase1.record_pok_g1(rec) == pok
    log.records.append(rec)
    log.names.append("x")
    assert phase1.transcript_hash(log, 0, pok) == tr != phase1.transcript_hash(log, 1, pok)
    other = phase1.PtauContributions(power=3, records=[rec[:-1] + b"\x01"], names=["x"])
    assert phase1.transcript_hash(other, 1, pok) != phase1.transcript_hash(log, 1, pok)
    ch = phase1.challenge_bytes(tr)
    assert len(ch) == 384 and ch == phase1.challenge_bytes(tr) and len({ch[:128], ch[128:256], ch[256:]}) == 3
    assert phase1.challenges(log) == [ch]
    for x in range(3):
        pt = o.g2_from_bytes(ch[128 * x:128 * x + 128])
        assert o.G2.is_on_curve(pt) and not o.G2.is_inf(pt) and o.G2.is_inf(o.G2.mul(R, pt))


def test_ptau_files_new(tmp_path):
    """tools/ptau_files.py new: the file of generators with an empty log; a power out of range is a usage error"""
    import dataclasses
    import sys

    from nim_groth16_amd import phase1
    from nim_groth16_amd.files import parsePtau, parsePtauContributions
    tool = os.path.join(ROOT, "tools", "ptau_files.py")
    path = str(tmp_path / "p0.ptau")
    out = subprocess.run([sys.executable, tool, "new", "3", "-o", path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "new: wrote" in out.stdout, out.stderr
    assert parsePtau(path) == dataclasses.replace(phase1.newPtau(3), ceremonyPower=3)
    assert parsePtauContributions(path) == ([], [])
    out = subprocess.run([sys.executable, tool, "new", "26", "-o", path], capture_output=True, text=True, timeout=300)
    assert out.returncode == 2 and "power must lie in" in out.stderr


# ---- the model of g16_ptau_verify (tests/phase1_pictures.py) ------------------------------------------------------------------
def test_ptau_verify_header_and_symbols():
    from nim_groth16_amd import _lib
    text = " ".join(open(os.path.join(ROOT, "include", "g16hip.h")).read().replace(" * ", " ").split())
    assert re.search(r"int32_t g16_ptau_verify\(g16_ctx\* ctx, const g16_ptau_desc\* ptau, const g16_ptau_contribution\* records, "
                     r"const void\* challenges_g2, size_t count, const void\* multipliers, g16_ptau_report\* out\)", text)
    assert "g16_ptau_verify" in _lib.SYMBOLS
    for word in ("g16_ptau_report", "1/(2^128 - 1)", "ONE tau", "G16_PTAUV_TAU_G2", "multiplier"):
        assert word in text[text.index("The check of a .ptau"):], word
    from tests import phase1_pictures as P1
    assert _lib.PTAU_REPORT_ARRAYS == P1.ARRAYS and _lib.PTAU_RELATIONS == P1.RELATIONS
    assert len(_lib.PTAU_REPORT_ARRAYS) == 14 and len(_lib.PTAU_RELATIONS) == 10
    assert "self-consistency (`snarkjs powersoftau verify`) is g16_ptau_verify's" in text


def test_ptau_model_over_the_pictures():
    from tests import phase1_pictures as P1
    pics = P1.pictures()
    rel = {name: pic.report["relation"] for name, pic in pics.items()}
    ok = [1] * 10
    for name, r in rel.items():
        assert (r == ok) == (name.startswith("clean_p") or name == "cancelling_pair_equal"), (name, r)
        assert pics[name].report["failed"] == sum(1 << k for k, v in enumerate(r) if v == 0)
    assert rel["clean_no_records"] == [1] * 7 + [-1] * 3
    for k in (1, 7, 14):
        assert rel[f"tauG1_{k}_doubled"][2] == 0 and rel[f"tauG1_{k}_doubled"][4:7] == [1, 1, 1]
    assert rel["tauG1_1_doubled"] == [1, 1, 0, 0, 1, 1, 1, 1, 1, 0]        # tauG1[1] is also TAU_G2's factor and LAST's value
    assert rel["tauG1_14_doubled"] == [1, 1, 0, 1, 1, 1, 1, 1, 1, 1]       # the last index: the shifted sum alone
    assert rel["tauG2_on_another_tau"] == [1, 1, 0, 0, 0, 0, 1, 1, 1, 0]   # ALPHA and BETA read tauG2[1]; LAST reads it too
    assert rel["alpha_on_another_tau"] == [1, 1, 1, 1, 0, 1, 1, 1, 1, 1]
    assert rel["betaG2_of_another_beta"] == [1, 1, 1, 1, 1, 1, 0, 1, 1, 0]
    assert rel["cancelling_pair_top_byte"] == [1, 1, 0, 1, 1, 1, 1, 1, 1, 1]
    assert rel["tauG2_3_outside_the_subgroup"] == [0, -1, -1, -1, -1, -1, 1, 1, 1, -1]
    assert pics["tauG2_3_outside_the_subgroup"].report["first_bad"][1] == [None, None, 3]
    assert rel["alpha_5_infinity"] == [0, 1, 1, 1, -1, 1, 1, 1, 1, -1]
    assert pics["alpha_5_infinity"].report["first_infinity"][2] == 5
    assert rel["pok_another_secret"][7:9] == [0, 0] and pics["pok_another_secret"].report["first_record"] == [1, 1]
    assert rel["step_skipped"] == [1] * 8 + [0, 1] and pics["step_skipped"].report["first_record"] == [None, 0]
    assert rel["records_swapped"][7:] == [1, 0, 0]
    assert rel["last_is_not_the_files"] == [1] * 9 + [0]
    assert rel["first_not_the_generator"][:2] == [1, 0]
    # the model of a contribution against the definition
    new, rec = P1.contribute(P1.new_ptau(2), 3, 5, 7, (11, 13, 17), (19, 23, 29))
    assert new["tauG1"] == [1, 3, 9, 27, 81, 243, 729] and new["alphaTauG1"] == [5, 15, 45, 135] and new["betaG2"] == [7]
    assert rec["pok"] == [(11, 33, 57), (13, 65, 115), (17, 119, 203)] and rec["tauG2"] == 3 and rec["betaG1"] == 7


def test_ptau_model_against_the_real_pairing():
    """the clean picture at power 3 satisfies the equations of the header under the oracle's pairing; a doubled element
    does not"""
    from tests import phase1_pictures as P1
    pics = P1.pictures()
    g1, g2 = lambda k: o.G1.mul(k % R, o.GEN1), lambda k: o.G2.mul(k % R, o.GEN2)     # noqa: E731
    for name, holds in (("clean_p3_k2", True), ("tauG1_7_doubled", False)):
        pic = pics[name]
        a, z = pic.ptau["tauG1"], pic.multipliers
        s0, s1 = sum(x * y for x, y in zip(z, a[:-1])), sum(x * y for x, y in zip(z, a[1:]))
        assert (o.pairing(g1(s0), g2(pic.ptau["tauG2"][1])) == o.pairing(g1(s1), o.GEN2)) == holds
    pic = pics["clean_p3_k2"]
    b, z = pic.ptau["tauG2"], pic.multipliers
    t0, t1 = sum(x * y for x, y in zip(z, b[:-1])), sum(x * y for x, y in zip(z, b[1:]))
    assert o.pairing(g1(pic.ptau["tauG1"][1]), g2(t0)) == o.pairing(o.GEN1, g2(t1))
    assert o.pairing(g1(pic.ptau["betaTauG1"][0]), o.GEN2) == o.pairing(o.GEN1, g2(pic.ptau["betaG2"][0]))
    r0, r1, ch = pic.records[0], pic.records[1], pic.challenges[1]
    s, sx, spx = r1["pok"][0]
    assert o.pairing(g1(s), g2(spx)) == o.pairing(g1(sx), g2(ch[0]))                           # POK
    assert o.pairing(g1(r0["tauG1"]), g2(spx)) == o.pairing(g1(r1["tauG1"]), g2(ch[0]))        # STEP, a G1 value
    assert o.pairing(g1(sx), g2(r0["tauG2"])) == o.pairing(g1(s), g2(r1["tauG2"]))             # STEP, a G2 value
