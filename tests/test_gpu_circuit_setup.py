"""g16_points_intt_g1/g2 and g16_circuit_setup on the GPU.  Everything is byte-exact.  The expected values come from plain
integers and from calls that are already held to the oracle and are not the code under test: the oracle's inverse NTT
over logarithms turned into points by the C oracle's fixed-base multiplier; g16_fake_setup (fakeCircuitSetup) for the toxic
waste (alpha, beta, gamma = 1, delta, tau); fakePtau for the powers of that tau.  The formulas themselves are held to the
oracle's fake_circuit_setup in tests/test_circuit_setup_cpu.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import bn254_ref as o
from tests import circuit_audit_pictures as CA
from tests import inputs as I
from tests import key_audit_pictures as KA

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = o.R
SECTIONS = ("alpha1", "beta1", "delta1", "beta2", "gamma2", "delta2", "pointsIC", "pointsA1", "pointsB1", "pointsB2",
            "pointsC1", "pointsH1")
PSZ = {1: 64, 2: 128}


# ---- the group inverse NTT ---------------------------------------------------------------------------------------------
def _intt(ctx, orc, group, logs):
    """the transform of fixed_base(logs) must be fixed_base(the inverse NTT of logs in integers); -> the integer result"""
    n = len(logs)
    log2n = n.bit_length() - 1
    want = o.inverse_ntt([x % R for x in logs], o.Domain(n))
    got = ctx.points_intt(group, orc.fixed_base(group, I.fr_mont_bytes(logs)), log2n)
    exp = orc.fixed_base(group, I.fr_mont_bytes(want))
    if got != exp:
        k = next(k for k in range(n) if got[PSZ[group] * k:PSZ[group] * (k + 1)] != exp[PSZ[group] * k:PSZ[group] * (k + 1)])
        raise AssertionError(f"G{group}, 2^{log2n}: output {k} differs (the first of them)")
    return want


@pytest.mark.parametrize("group,log2n", [(1, 0), (1, 1), (1, 2), (1, 3), (1, 6), (1, 11), (2, 0), (2, 1), (2, 2), (2, 3),
                                         (2, 6), (2, 8)])
def test_points_intt_random(ctx, orc, group, log2n):
    rng = o.SplitMix64(100 * group + log2n)
    _intt(ctx, orc, group, [rng.fr() for _ in range(1 << log2n)])


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("log2n", [3, 6])
def test_points_intt_exceptional(ctx, orc, group, log2n):
    n = 1 << log2n
    omega = o.Domain(n).domainGen
    # tau = 1 = omega^0: all inputs equal, every output but the first at infinity
    assert _intt(ctx, orc, group, [1] * n) == [1] + [0] * (n - 1)
    # tau = omega^j: the output is gen at k = j and infinity elsewhere: sums cancel in every stage
    for j in (0, 1, n - 1):
        tau = pow(omega, j, R)
        assert _intt(ctx, orc, group, [pow(tau, k, R) for k in range(n)]) == [1 if k == j else 0 for k in range(n)]
    # tau = 0: gen, then infinities; every output is gen / n
    out = _intt(ctx, orc, group, [1] + [0] * (n - 1))
    assert out == [o.inv_fr(n)] * n
    # nothing but (0,0); and (0,0) scattered among random points
    assert _intt(ctx, orc, group, [0] * n) == [0] * n
    rng = o.SplitMix64(7 + group + log2n)
    logs = [rng.fr() for _ in range(n)]
    for k in (0, 2, 3, n // 2, n - 1):
        logs[k] = 0
    _intt(ctx, orc, group, logs)
    # two equal and two opposite neighbours: the first stage doubles and cancels
    logs[0], logs[n // 2], logs[1], logs[1 + n // 2] = 5, 5, 9, R - 9
    _intt(ctx, orc, group, logs)


def test_points_intt_arguments(ctx):
    from nim_groth16_amd import G16Error
    from nim_groth16_amd._lib import G16_EINVAL
    with pytest.raises(G16Error, match="log2n out of range") as e:
        ctx._check(ctx._lib.g16_points_intt_g1(ctx._h, ctypes.create_string_buffer(64), 25, ctypes.create_string_buffer(64)))
    assert e.value.code == G16_EINVAL
    with pytest.raises(G16Error, match="null pointer") as e:
        ctx._check(ctx._lib.g16_points_intt_g2(ctx._h, None, 0, ctypes.create_string_buffer(128)))
    assert e.value.code == G16_EINVAL


# ---- whole keys ----------------------------------------------------------------------------------------------------------
def heavy_circuit() -> CA.Circuit:
    """The constant wire holds 4 entries of A in every one of 40 constraints (160 > 128: the last bin of
    spmv_params.hpp, beyond the largest single-lane bin of 4 and the first cooperative bin of 8), wire 1 six of B in all
    (the first cooperative bin), wire 23 occurs nowhere, wire 22 only with the value 0; values: 0 given explicitly, small
    ones, r - 1 and full 254-bit ones."""
    rng = o.SplitMix64(4242)
    nvars, ncons = 24, 40
    cons = []
    for i in range(ncons):
        A = [(0, 0), (0, 3), (0, R - 1), (0, rng.fr())] + [(1 + rng.next() % 21, rng.fr()) for _ in range(3)]
        B = [(2 + rng.next() % 20, rng.fr() if i % 3 else 1 + rng.next() % 7) for _ in range(2)]
        if i < 6:
            B.append((1, rng.fr()))
        C = [(rng.next() % 22, rng.fr()), (2 + rng.next() % 20, R - 1)]
        if i % 8 == 0:
            C.append((22, 0))
        cons.append((A, B, C))
    return CA.Circuit(nvars, 2, cons)


def _circuit(name) -> CA.Circuit:
    return heavy_circuit() if name == "heavy" else CA.circuits()[name]


def _r1cs(c: CA.Circuit):
    from nim_groth16_amd.fake_setup import R1CS
    return R1CS(c.nvars, c.npubs, 0, c.nvars - c.npubs - 1, c.constraints)


_made = {}


def _waste(name):
    tw = CA.toxic(3000 + len(name))
    return tw


def _ptau(ctx, name, extra=1):
    """the powers of the circuit's tau a ceremony would publish, power = log2 of the domain + extra"""
    from nim_groth16_amd.fake_setup import fakePtau
    if (name, extra) not in _made:
        tw = _waste(name)
        _made[name, extra] = fakePtau(tw.tau, tw.alpha, tw.beta, _circuit(name).log2_domain + extra, ctx)
    return _made[name, extra]


def _fake(ctx, name, flavour, delta):
    """g16_fake_setup's key for (alpha, beta, gamma = 1, delta, tau): the expected value"""
    from nim_groth16_amd.fake_setup import ToxicWaste, fakeCircuitSetup
    if ("fake", name, flavour, delta) not in _made:
        tw = _waste(name)
        _made["fake", name, flavour, delta] = fakeCircuitSetup(_r1cs(_circuit(name)),
                                                               ToxicWaste(tw.alpha, tw.beta, 1, delta, tw.tau), flavour, ctx)
    return _made["fake", name, flavour, delta]


def _sections(zk) -> dict:
    out = {k: getattr(zk.specPoints, k) for k in SECTIONS[:6]}
    out["pointsIC"] = zk.pointsIC
    out.update({k: getattr(zk.pPoints, k) for k in SECTIONS[7:]})
    return {k: bytes(v) for k, v in out.items()}


def _assert_same_key(got, want, what):
    g, w = _sections(got), _sections(want)
    for s in SECTIONS:
        assert len(g[s]) == len(w[s]), (what, s)
        assert g[s] == w[s], (what, s)
    assert (got.header.nvars, got.header.npubs, got.header.logDomainSize, got.header.flavour) == \
        (want.header.nvars, want.header.npubs, want.header.logDomainSize, want.header.flavour)


@pytest.mark.parametrize("name", ["toy", "chain", "dup", "nopriv", "heavy"])
def test_whole_keys(ctx, name):
    """circuitSetup(r1cs, fakePtau(tau, alpha, beta, L + 1)) == fakeCircuitSetup(toxic = (alpha, beta, 1, delta, tau)) in
    every one of the twelve sections, both flavours, delta NULL and given"""
    from nim_groth16_amd.setup import circuitSetup
    c = _circuit(name)
    tw = _waste(name)
    for flavour in (CA.SNARKJS, CA.JENSGROTH):
        for delta in (None, tw.delta):
            got = circuitSetup(_r1cs(c), _ptau(ctx, name), flavour, delta, ctx)
            _assert_same_key(got, _fake(ctx, name, flavour, 1 if delta is None else delta), (name, flavour, delta))
    if name == "nopriv":
        assert got.pPoints.pointsC1 == b""
    if name == "heavy":                                       # wire 23 is in no matrix, wire 22 only with the value 0
        pp = got.pPoints
        for w in (22, 23):
            assert pp.pointsA1[64 * w:64 * w + 64] == bytes(64) and pp.pointsB1[64 * w:64 * w + 64] == bytes(64)
            assert pp.pointsB2[128 * w:128 * w + 128] == bytes(128) and pp.pointsC1[64 * (w - 3):64 * (w - 2)] == bytes(64)
        lens = np.bincount([w for con in c.constraints for w, _ in con[0]], minlength=c.nvars)
        assert lens[0] > 128 and 4 < sum(1 for con in c.constraints for w, _ in con[1] if w == 1) <= 8


def _descs(c: CA.Circuit, pt, flavour, std):
    """the two descriptions of g16_circuit_setup from triplets in file order, values in either form -> (r1cs, ptau, keep)"""
    from nim_groth16_amd._lib import SCALARS_MONT, SCALARS_STD, R1csDesc
    from nim_groth16_amd.files.zkey import ptauDesc
    rd = R1csDesc()
    rd.nvars, rd.npubs, rd.nconstraints, rd.flavour = c.nvars, c.npubs, c.ncons, flavour
    rd.flags = SCALARS_STD if std else SCALARS_MONT
    keep = []
    for k, ent in enumerate(c.triplets()):
        rows = np.array([e[0] for e in ent], dtype=np.uint32)
        cols = np.array([e[1] for e in ent], dtype=np.uint32)
        vals = ctypes.create_string_buffer((I.fr_std_bytes if std else I.fr_mont_bytes)([e[2] for e in ent]) or b"\0")
        keep += [rows, cols, vals]
        rd.nnz[k] = len(ent)
        if ent:
            rd.row[k], rd.col[k] = rows.ctypes.data, cols.ctypes.data
            rd.val[k] = ctypes.cast(vals, ctypes.c_void_p).value
    pd, pkeep = ptauDesc(pt)
    return rd, pd, keep + [pkeep]


def _assert_points(pts: dict, want, what):
    w = _sections(want)
    for s in SECTIONS:
        assert pts[s] == w[s], (what, s)


def test_values_in_standard_form(ctx):
    for name in ("toy", "chain", "dup", "nopriv", "heavy"):
        c, tw = _circuit(name), _waste(name)
        rd, pd, keep = _descs(c, _ptau(ctx, name), CA.SNARKJS, std=True)
        log2, pts = ctx.circuit_setup(rd, pd, I.fr_std_bytes([tw.delta]))
        assert log2 == c.log2_domain
        _assert_points(pts, _fake(ctx, name, CA.SNARKJS, tw.delta), name)
        del keep


def test_a_ptau_larger_than_needed(ctx):
    from nim_groth16_amd.setup import circuitSetup
    for name, flavour in (("toy", CA.SNARKJS), ("dup", CA.JENSGROTH)):
        got = circuitSetup(_r1cs(_circuit(name)), _ptau(ctx, name, extra=3), flavour, None, ctx)
        _assert_same_key(got, _fake(ctx, name, flavour, 1), name)


# ---- the closed loop: setup -> audit -> prove -> verify --------------------------------------------------------------------
def _toy(ctx):
    from nim_groth16_amd.fake_setup import R1CS
    from nim_groth16_amd.setup import circuitSetup
    r1cs = R1CS(8, 1, 1, 3, o.toy_r1cs().constraints)
    pt = _ptau(ctx, "toy")
    return r1cs, pt, circuitSetup(r1cs, pt, ctx=ctx)


def test_the_key_passes_the_circuit_audit_and_proves(ctx):
    from nim_groth16_amd import Mask, Witness, extractVKey, generateProofWithMask, loadProvingKey, verifyProof
    from nim_groth16_amd.files.zkey import auditCircuit
    r1cs, pt, zk = _toy(ctx)
    rep = auditCircuit(zk, r1cs, pt, ctx)
    assert rep.failed == 0 and rep.relation == [1] * 9 and rep.key.relation == [1, 1, 1], str(rep)
    pk = loadProvingKey(zk, ctx)
    try:
        pr = generateProofWithMask(0, False, zk, Witness("bn128", 8, I.fr_mont_bytes(o.TOY_WITNESS)), Mask(21, 22), ctx, pkey=pk)
    finally:
        pk.destroy()
    assert verifyProof(extractVKey(zk), pr, ctx)


def test_both_clis_make_the_same_key_and_verify(ctx, tmp_path):
    from nim_groth16_amd.files import parseZKey, writePtau, writeR1CS, writeWitness
    from tests.test_gpu_native_cli import _build
    r1cs, pt, zk = _toy(ctx)
    rpath, ppath, wpath = (str(tmp_path / n) for n in ("toy.r1cs", "toy.ptau", "toy.wtns"))
    writeR1CS(rpath, r1cs)
    writePtau(ppath, pt, extraSections=[(7, b"contributions")])
    writeWitness(wpath, o.TOY_WITNESS)
    # the key alone
    tool = os.path.join(ROOT, "tools", "prove_files.py")
    only = str(tmp_path / "only.zkey")
    out = subprocess.run([sys.executable, tool, "--setup-ptau", ppath, "-r", rpath, "-z", only], capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0 and "circuit setup: wrote" in out.stdout, out.stderr
    # the key, then a proof from it
    zpy = str(tmp_path / "py.zkey")
    out = subprocess.run([sys.executable, tool, "--setup-ptau", ppath, "-r", rpath, "-z", zpy, "-w", wpath, "-o",
                          str(tmp_path / "py_proof.json"), "-i", str(tmp_path / "py_public.json"), "-n", "-y"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "verification succeeded" in out.stdout, out.stderr
    assert open(only, "rb").read() == open(zpy, "rb").read()
    exe = _build(tmp_path)
    znat = str(tmp_path / "native.zkey")
    out = subprocess.run([exe, "-u", "-r", rpath, "--ptau", ppath, "-z", znat, "-w", wpath, "-o",
                          str(tmp_path / "nat_proof.json"), "-i", str(tmp_path / "nat_public.json"), "-n", "-y"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "verification succeeded" in out.stdout, out.stderr
    a, b = parseZKey(zpy), parseZKey(znat)
    _assert_same_key(a, zk, "prove_files.py --setup-ptau")
    _assert_same_key(b, zk, "g16prove --ptau")
    assert sorted(a.coeffs) == sorted(b.coeffs) == sorted(zk.coeffs)         # the tools list the A and B entries in their own order
    assert open(tmp_path / "py_proof.json").read() == open(tmp_path / "nat_proof.json").read()   # trivial mask: one proof
    # a delta of the tool's own: another key, which still verifies; and the flags that do not go together
    out = subprocess.run([exe, "-u", "-r", rpath, "--ptau", ppath, "--delta-seed", "7", "-z", str(tmp_path / "d.zkey"), "-w",
                          wpath, "-o", str(tmp_path / "d_proof.json"), "-i", str(tmp_path / "d_public.json"), "-n", "-y"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "verification succeeded" in out.stdout, out.stderr
    d = parseZKey(str(tmp_path / "d.zkey"))
    assert d.specPoints.delta1 != zk.specPoints.delta1 and d.pPoints.pointsA1 == zk.pPoints.pointsA1
    out = subprocess.run([exe, "-z", znat, "-w", wpath, "--ptau", ppath], capture_output=True, text=True, timeout=600)
    assert out.returncode != 0 and "go together" in out.stderr


# ---- refusals, and no state change ---------------------------------------------------------------------------------------
def test_refusals(ctx):
    from nim_groth16_amd import G16Error
    from nim_groth16_amd._lib import G16_EINVAL, PTAU_SECTIONS
    c, pt = _circuit("toy"), _ptau(ctx, "toy")
    want = _fake(ctx, "toy", CA.SNARKJS, 1)

    def refused(match, edit=None, delta=None, ptau=pt):
        rd, pd, keep = _descs(c, ptau, CA.SNARKJS, std=False)
        if edit:
            edit(rd, pd, keep)
        with pytest.raises(G16Error, match=match) as e:
            ctx.circuit_setup(rd, pd, delta)
        assert e.value.code == G16_EINVAL, match
        del keep
        rd, pd, keep = _descs(c, pt, CA.SNARKJS, std=False)                   # ... and a good call still gives the right key
        _assert_points(ctx.circuit_setup(rd, pd)[1], want, match)
        del keep

    def planted(section, index, raw):
        from dataclasses import replace
        b = bytearray(getattr(pt, section))
        b[len(raw) * index:len(raw) * (index + 1)] = raw
        return replace(pt, **{section: bytes(b)})

    refused(r"too short", lambda r, p, k: setattr(p, "power", c.log2_domain))
    for name in PTAU_SECTIONS:
        refused(r"null ptau section", lambda r, p, k, name=name: setattr(p, name, None))
    refused(r"null matrix pointer", lambda r, p, k: r.val.__setitem__(1, None))
    refused(r"delta must not be zero", delta=bytes(32))
    refused(r"delta is not canonical", delta=R.to_bytes(32, "little"))
    refused(r"nvars must exceed npubs", lambda r, p, k: setattr(r, "npubs", c.nvars))
    refused(r"matrix 1 entry 1 out of range", lambda r, p, k: k[4].__setitem__(1, c.nvars))      # k[4]: the wires of B
    refused(r"matrix 0 entry 0 out of range", lambda r, p, k: k[0].__setitem__(0, c.ncons))      # k[0]: the rows of A

    def big_value(r, p, k):
        vals = bytearray(ctypes.string_at(r.val[2], 32 * r.nnz[2]))
        vals[32:64] = R.to_bytes(32, "little")
        k.append(ctypes.create_string_buffer(bytes(vals), len(vals)))
        r.val[2] = ctypes.cast(k[-1], ctypes.c_void_p).value
    refused(r"matrix 2 entry 1: value is not canonical", big_value)
    # ptau elements: a tauG1 element whose x is x + p, a tauG2 element of small order (on the twist, outside the subgroup)
    el = pt.tauG1[64 * 5:64 * 6]
    alias = (int.from_bytes(el[:32], "little") + o.P).to_bytes(32, "little") + el[32:]
    refused(r"ptau tauG1\[5\] is not a canonical encoding", ptau=planted("tauG1", 5, alias))
    small = o.g2_to_bytes(KA.twist_outsiders()["small"])
    refused(r"ptau tauG2\[3\] is not in the order-r subgroup", ptau=planted("tauG2", 3, small))
    refused(r"ptau alphaTauG1\[2\] is not on the curve", ptau=planted("alphaTauG1", 2, KA.off_curve(1)))


def test_setup_touches_no_state(ctx):
    """g16_prove on a resident key gives the same bytes before and after a setup call on the same context"""
    from nim_groth16_amd import Mask, Witness, generateProofWithMask, loadProvingKey
    from nim_groth16_amd.setup import circuitSetup
    zk = _fake(ctx, "toy", CA.SNARKJS, _waste("toy").delta)
    wt = Witness("bn128", 8, I.fr_mont_bytes(o.TOY_WITNESS))
    pk = loadProvingKey(zk, ctx)
    try:
        before = generateProofWithMask(0, False, zk, wt, Mask(11, 12), ctx, pkey=pk)
        circuitSetup(_r1cs(_circuit("chain")), _ptau(ctx, "chain"), CA.SNARKJS, 5, ctx)
        ctx.points_intt(2, _ptau(ctx, "toy").tauG2[:128 * 8], 3)
        after = generateProofWithMask(0, False, zk, wt, Mask(11, 12), ctx, pkey=pk)
        assert (before.pi_a, before.pi_b, before.pi_c) == (after.pi_a, after.pi_b, after.pi_c)
    finally:
        pk.destroy()
