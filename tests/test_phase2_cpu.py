"""Phase-2 contribution, the parts that need no GPU: the uniform-scalar schedule of scale_plan.hpp and the lane arithmetic
of scale.cuh built with g++ (tests/cpu_kernels/scale_plan_shim.cpp) against Python integers and the oracle; the
endomorphism constants; the transcript of phase2.py; section 10 of a .zkey; the log-space model of the chain."""
import ctypes
import os
import re
import subprocess

import pytest

from oracle import bn254_ref as o
from tests import inputs as I
from tests import phase2_pictures as PP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, P = o.R, o.P
SHIM_DIR = os.path.join(ROOT, "tests", "cpu_kernels")
ENTRY = {0: (1, 0), 1: (0, 1), 2: (1, 1), 3: (1, -1)}      # P, phi P, P + phi P, P - phi P


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(SHIM_DIR, "libscale_plan_shim.so")
    src = os.path.join(SHIM_DIR, "scale_plan_shim.cpp")
    if not os.path.exists(so):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", src, "-o", so])
    return ctypes.CDLL(so)


def le(x):
    return int(x).to_bytes(32, "little")


def plan(shim, k):
    steps = ctypes.create_string_buffer(4 * shim.shim_scale_max_steps())
    info, val = (ctypes.c_int32 * 3)(), ctypes.create_string_buffer(32)
    ok = shim.shim_scale_plan(le(k), steps, info, val)
    st = [(steps.raw[4 * i], steps.raw[4 * i + 1], 1 if steps.raw[4 * i + 2] == 1 else -1) for i in range(info[0])]
    assert all(steps.raw[4 * i + 2] in (1, 255) and steps.raw[4 * i + 1] < 4 for i in range(info[0]))
    return ok, st, list(info), int.from_bytes(val.raw, "little")


def test_header_and_symbols():
    from nim_groth16_amd._lib import SYMBOLS
    text = " ".join(open(os.path.join(ROOT, "include", "g16hip.h")).read().replace(" * ", " ").split())
    for name in ("g16_points_scale_g1", "g16_points_scale_g2", "g16_key_contribute", "g16_contributions_verify"):
        assert re.search(r"int32_t " + name + r"\(g16_ctx\*", text), name
        assert name in SYMBOLS
    for word in ("g16_phase2_key", "g16_contribution", "g16_phase2_out", "g16_chain_report", "1/(2^128 - 1)"):
        assert word in text[text.index("phase-2 contribution: what makes"):], word
    assert "only after a phase-2 contribution" in text and "section 10" in text and "sections 12-15" in text
    assert "ANCHOR" in text


def test_constants_pair_up(shim):
    """lambda gen1 == (beta, 2): the cube roots of unity of the two fields that belong together; the other pairing fails"""
    buf = (ctypes.c_uint64 * 12)()
    shim.shim_scale_consts(buf)
    raw = bytes(buf)
    r, lam, beta = (int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(3))
    assert r == R and (lam, beta) == (PP.LAMBDA, PP.BETA)
    assert pow(lam, 3, R) == 1 != lam and pow(beta, 3, P) == 1 != beta
    assert o.G1.mul(lam, o.GEN1) == (beta, 2)
    assert o.G1.mul(lam * lam % R, o.GEN1) == (beta * beta % P, 2) != (beta, 2)
    rng = o.SplitMix64(3)
    pt = o.G1.mul(rng.fr(), o.GEN1)
    assert o.G1.mul(lam, pt) == (beta * pt[0] % P, pt[1])
    # the Montgomery constants of scale.cuh
    src = open(os.path.join(ROOT, "nim_groth16_amd", "csrc", "scale.cuh")).read()
    limbs = re.findall(r"return u256\{\{((?:0x[0-9a-f]{8}u(?:, )?){8})\}\};", src)
    vals = [sum(int(w.rstrip("u"), 16) << (32 * i) for i, w in enumerate(m.split(", "))) for m in limbs]
    assert vals == [x * o.MONT % P for x in (beta, beta * beta % P, (beta - 1) % P)]


def test_plan_evaluates_to_k(shim):
    """the independent checker of the header and a digit-by-digit walk in Python integers; halves below 2^128; the step
    count within the joint sparse form's bound"""
    rng = o.SplitMix64(11)
    ks = PP.edge_scalars() + [rng.fr() for _ in range(3000)]
    total = longest = 0
    for k in ks:
        ok, steps, (nsteps, ndbl, tail), val = plan(shim, k)
        assert ok == 1 and val == k, hex(k)
        halves, signs = (ctypes.c_uint64 * 4)(), ctypes.c_uint32()
        assert shim.shim_scale_split(le(k), halves, ctypes.byref(signs)) == 1
        k1, k2 = halves[0] | halves[1] << 64, halves[2] | halves[3] << 64
        assert k1 < 1 << 128 and k2 < 1 << 128
        longest = max(longest, k1, k2)
        s1, s2 = (-1 if signs.value & 1 else 1), (-1 if signs.value & 2 else 1)
        assert (s1 * k1 + s2 * k2 * PP.LAMBDA - k) % R == 0
        c1 = c2 = dbl = 0
        for j, (d, e, s) in enumerate(steps):
            assert (d == 0) == (j == 0)
            c1, c2, dbl = c1 << d, c2 << d, dbl + d
            c1, c2 = c1 + s * ENTRY[e][0], c2 + s * ENTRY[e][1]
        c1, c2, dbl = c1 << tail, c2 << tail, dbl + tail
        assert (c1, c2) == (s1 * k1, s2 * k2) and dbl == ndbl
        # at most one column per bit of the longer half, plus one; never more doublings than that
        length = max(k1.bit_length(), k2.bit_length())
        assert nsteps <= length + 1 <= 129 and ndbl <= length and nsteps <= shim.shim_scale_max_steps()
        assert (nsteps == 0) == (k == 0)
        if k not in PP.edge_scalars():
            total += nsteps
    # the joint sparse form has density 1/2: the mean over 3000 random scalars (halves of ~126 bits, standard deviation of
    # one count ~ 4, of the mean ~ 0.1) lies well inside [0.47, 0.53] of 127
    assert 0.47 * 127 <= total / 3000 <= 0.53 * 127, total / 3000
    assert (shim.shim_scale_block(), shim.shim_scale_group()) == (64, 4)
    # the constructed scalars reach the edge of what the decomposition gives: halves of 127 bits, 0.48 * 2^128 and more
    assert longest >= 48 * (1 << 128) // 100, longest.bit_length()


def test_python_split_agrees(shim):
    for k in PP.edge_scalars():
        k1, k2 = PP.split(k)
        assert abs(k1) < 1 << 127 and abs(k2) < 1 << 127


def test_lane_arithmetic_against_the_oracle(shim):
    """scale_lane of scale.cuh, every workgroup and lane of the grid in turn: the endomorphism ladder over the plan, the
    grouped affine conversion with (0,0) members, in place"""
    rng = o.SplitMix64(5)
    logs = [rng.fr() for _ in range(70)]
    for i in (0, 5, 69):
        logs[i] = 0
    pts = o_fixed(1, logs)
    for k in PP.edge_scalars() + [rng.fr()]:
        buf = ctypes.create_string_buffer(pts, len(pts))
        shim.shim_scale_points_g1(buf, ctypes.c_uint64(len(logs)), le(k), buf)
        assert buf.raw == o_fixed(1, [k * x % R for x in logs]), hex(k)
    logs2 = [rng.fr(), 0, rng.fr(), rng.fr(), rng.fr()]
    pts2 = o_fixed(2, logs2)
    for k in (0, 1, R - 1, rng.fr()):
        buf = ctypes.create_string_buffer(pts2, len(pts2))
        shim.shim_scale_points_g2(buf, ctypes.c_uint64(len(logs2)), le(k), buf)
        assert buf.raw == o_fixed(2, [k * x % R for x in logs2]), hex(k)
    # straight against the Python oracle's ladder
    k = rng.fr()
    buf = ctypes.create_string_buffer(pts[:64 * 3], 64 * 3)
    shim.shim_scale_points_g1(buf, ctypes.c_uint64(3), le(k), buf)
    for i in range(3):
        assert o.g1_from_bytes(buf.raw[64 * i:64 * i + 64]) == o.G1.mul(k, o.g1_from_bytes(pts[64 * i:64 * i + 64]))


def o_fixed(group, logs):
    from tests.oracle_c import load_oracle
    return load_oracle().fixed_base(group, I.fr_mont_bytes(list(logs)))


def test_hash_to_g2():
    from nim_groth16_amd import phase2
    assert phase2.TWIST_B == o.TWIST_B and phase2.COFACTOR_G2 == 2 * P - R
    seen = set()
    for j in range(6):
        h = bytes([j]) * 64
        pt = phase2.hash_to_g2(h)
        assert not o.G2.is_inf(pt) and o.G2.is_on_curve(pt) and o.G2.is_inf(o.G2.mul(R, pt))
        assert pt == phase2.hash_to_g2(h) and o.g2_to_bytes(pt) == phase2.g2_to_bytes(pt) == phase2.challenge_bytes(h)
        seen.add(pt)
    assert len(seen) == 6
    a = (5, 7)
    root = phase2.fp2_sqrt(o.fp2_sqr(a))
    assert root in (a, o.fp2_neg(a))
    assert phase2.g2_mul(12345, o.GEN2) == o.G2.mul(12345, o.GEN2)


def _snarkjs_file(tmp_path):
    """the .zkey of tests/snarkjs_layout.py (sections out of order, a section 10 of 200 zero bytes) -> (path, its ZKey)"""
    from nim_groth16_amd.files import parseZKey
    from tests.test_files_cpu import _snarkjs_like
    zpath = _snarkjs_like(tmp_path, (1, 2, 4, 3, 9, 8, 5, 6, 7, 10), False)[0]
    return zpath, parseZKey(zpath)


def test_section_10_round_trip(tmp_path):
    import copy

    from nim_groth16_amd import phase2
    from nim_groth16_amd.files import parseContributions, parseZKey, writeZKey
    zk = copy.deepcopy(_snarkjs_file(tmp_path)[1])
    path = str(tmp_path / "a.zkey")
    writeZKey(path, zk)
    plain = open(path, "rb").read()
    assert parseContributions(path) is None
    cs = phase2.cs_hash(zk)
    assert len(cs) == 64 and cs == phase2.cs_hash(parseZKey(path)) == phase2.cs_hash(parseZKey(path, rawCoeffs=True))
    log = phase2.Contributions(cs_hash=cs)
    for j, name in enumerate(("first", "", "third é")):
        rec = bytes([j + 1]) * 320
        log.transcripts.append(phase2.transcript_hash(log, j, rec[64:128], rec[128:192]))
        log.records.append(rec)
        log.names.append(name)
    zk.contributions = log
    writeZKey(path, zk)
    data = open(path, "rb").read()
    assert data[12:len(plain)] == plain[12:] and len(data) > len(plain)          # sections 1-9 as before, one more
    got = parseContributions(path)
    assert got == log
    back = parseZKey(path)                                                        # the prover's reader skips it
    assert back.contributions is None and back.pPoints == zk.pPoints and back.specPoints == zk.specPoints
    assert phase2.challenges(got)[1] is True
    got.transcripts[1] = bytes(64)
    assert phase2.challenges(got)[1] is False
    # malformed sections
    from nim_groth16_amd.files.container import parseContainer, writeContainer
    sec = parseContainer("zkey", 1, path)
    s10 = bytes(sec[10][0])
    others = [(sid, bytes(v[0])) for sid, v in sec.items() if sid != 10]
    for bad, match in ((s10[:40], "shorter"), (s10[:-1], "truncated"), (s10 + b"x", "left over"),
                       (s10[:68 + 384] + b"\x01" + s10[68 + 385:], "type")):
        p2 = str(tmp_path / "bad.zkey")
        writeContainer("zkey", 1, p2, others + [(10, bad)])
        with pytest.raises(ValueError, match=match):
            parseContributions(p2)
        parseZKey(p2)


def test_parse_zkey_still_skips_a_foreign_section_10(tmp_path):
    from nim_groth16_amd.files import parseContributions
    from nim_groth16_amd.files.container import parseContainer
    path, zk = _snarkjs_file(tmp_path)
    assert zk.header.nvars == 5 and zk.contributions is None and len(zk.pPoints.pointsH1) == 64 * 4
    assert len(parseContainer("zkey", 1, path)[10][0]) > 64                      # a log of another hand
    with pytest.raises(ValueError):
        parseContributions(path)                                                  # 200 zero bytes are not a log of ours


def test_chain_model_over_the_pictures():
    pics = PP.pictures()
    assert len(pics) >= 40
    import functools
    fixed = functools.lru_cache(None)(lambda g, logs: o_fixed(g, logs))
    ok = [1] * 7
    for name, pic in pics.items():
        if pic.report is None:                                                    # completed from the element's bytes
            PP.encode(pic, fixed)
        rep = pic.report
        assert rep["failed"] == sum(1 << k for k, v in enumerate(rep["relation"]) if v == 0)
        assert (rep["relation"] == ok) == name.startswith("honest"), name
    # the model of a contribution against the definition: delta up, C1 / H1 down, the record's two equations
    key = PP.key_part("toy")
    new, rec = PP.contribute(key, 7, 11, 13)
    assert new["delta1"] == 7 and [x * 7 % R for x in new["pointsC1"]] == key["pointsC1"]
    assert rec == {"delta_after": 7, "g1_s": 11, "g1_sx": 77, "g2_spx": 91}
    assert pics["records_swapped_toy"].report["first_record"] == [None, 0]
    assert pics["off_curve_g2_spx"].report["relation"] == [0, -1, -1, 1, 1, 1, 1]
