"""g16_circuit_audit on the GPU against the integer model of tests/circuit_audit_pictures.py (held to itself in
tests/test_circuit_audit_model_cpu.py): every report must equal the model entry for entry.  The keys and the powers of
tau are the model's logarithms turned into points by the C oracle's fixed-base multiplier -- nothing the library
computed goes into what it is asked to judge.  Circuits: the toy R1CS (8 wires, domain 8), the same with a duplicated and
a cancelling pair of entries, one without a private wire, and the squaring chain of 512 wires (domain 512, an H vector
of 1024: arrays that span workgroups)."""
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
_points = {}


def _fixed(orc):
    def fixed(group, logs):
        if (group, logs) not in _points:
            _points[group, logs] = orc.fixed_base(group, I.fr_mont_bytes(list(logs))) if logs else b""
        return _points[group, logs]
    return fixed


def _cbuf(x: bytes):
    return ctypes.create_string_buffer(x, len(x)) if x else ctypes.create_string_buffer(1)


def _descs(pic: CA.Picture, orc, std_values=False):
    """-> (PkeyDesc, VkeyDesc or None, section 4 or None, R1csDesc, PtauDesc, keepalive)"""
    from nim_groth16_amd._lib import SCALARS_MONT, SCALARS_STD, PkeyDesc, PtauDesc, R1csDesc, VkeyDesc
    s, t = CA.encode(pic, _fixed(orc))
    coeffs = CA.coeff_bytes(pic)
    packed = b"".join(m.to_bytes(4, "little") + r_.to_bytes(4, "little") + c.to_bytes(4, "little") + bytes(4) + v
                      for m, r_, c, v in coeffs)
    names = ("pointsA1", "pointsB1", "pointsB2", "pointsC1", "pointsH1", None, "alpha1", "beta1", "delta1", "beta2",
             "delta2", "gamma2", "pointsIC")
    bufs = [_cbuf(packed if n is None else s[n]) for n in names]
    a = [ctypes.cast(b, ctypes.c_void_p) for b in bufs]
    desc = PkeyDesc(pic.nvars, pic.npubs, pic.log2_domain, pic.flavour, a[0], a[1], a[2],
                    a[3] if s["pointsC1"] else None, a[4], None if pic.raw_coeffs else a[5],
                    0 if pic.raw_coeffs else len(coeffs), a[6], a[7], a[8], a[9], a[10], 0, 1)
    vk = VkeyDesc(pic.npubs, a[6], a[9], a[11], a[10], a[12]) if pic.with_vk else None
    s4 = KA.Key(pic.nvars, pic.npubs, pic.log2_domain, s, coeffs).section4() if pic.raw_coeffs else None
    rd = R1csDesc()
    rd.nvars, rd.npubs, rd.nconstraints, rd.flavour = pic.nvars, pic.npubs, pic.ncons, pic.flavour
    rd.flags = SCALARS_STD if std_values else SCALARS_MONT
    keep = [bufs]
    for k, ent in enumerate(pic.r1cs):
        rows = np.array([e[0] for e in ent], dtype=np.uint32)
        cols = np.array([e[1] for e in ent], dtype=np.uint32)
        vals = _cbuf((I.fr_std_bytes if std_values else I.fr_mont_bytes)([e[2] for e in ent]))
        keep += [rows, cols, vals]
        rd.nnz[k] = len(ent)
        if ent:
            rd.row[k], rd.col[k] = rows.ctypes.data, cols.ctypes.data
            rd.val[k] = ctypes.cast(vals, ctypes.c_void_p).value
    pbufs = [_cbuf(t[name]) for name in CA.PTAU_SECTIONS]
    pd = PtauDesc(pic.power, *[ctypes.cast(b, ctypes.c_void_p) for b in pbufs])
    keep.append(pbufs)
    return desc, vk, s4, rd, pd, keep


def _audit(ctx, orc, pic, **kw):
    desc, vk, s4, rd, pd, keep = _descs(pic, orc, **kw)
    rep = ctx.circuit_audit(desc, vk, s4, rd, pd, pic.zw, pic.zh)
    del keep
    return rep


FAMILIES = {"clean": ("clean_", "dup_", "delta_changed_"), "a1": ("a1_",), "points": ("b1_", "c1_", "ic_", "h1_"),
            "coeffs": ("coeff_", "r1cs_"), "ptau": ("ptau_", "flavour_")}


@pytest.mark.parametrize("size", ["small", "chain"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_pictures(ctx, orc, family, size):
    pics = CA.pictures()
    assert sorted(n for n in pics if n.startswith(tuple(p for f in FAMILIES.values() for p in f))) == sorted(pics)
    mine = {n: p for n, p in pics.items() if n.startswith(FAMILIES[family]) and (p.circuit == "chain") == (size == "chain")}
    assert len(mine) >= 3
    for name, pic in mine.items():
        rep = _audit(ctx, orc, pic)
        assert rep.as_dict() == pic.report, (name, rep.as_dict(), pic.report)
        assert rep.ok == (pic.report["failed"] == 0)


def test_r1cs_values_in_standard_form(ctx, orc):
    for name in ("clean_dup_sn", "r1cs_entry_toy", "clean_nopriv_jg"):
        pic = CA.pictures()[name]
        assert _audit(ctx, orc, pic, std_values=True).as_dict() == pic.report, name


def test_key_report_is_the_key_audits(ctx, orc):
    """the first part of the report: byte for byte what g16_key_audit says about the same key"""
    for name in ("clean_toy_sn", "a1_off_curve", "coeff_not_canonical_section4", "b1_b2_moved_toy", "clean_toy_no_vk"):
        pic = CA.pictures()[name]
        desc, vk, s4, rd, pd, keep = _descs(pic, orc)
        alone = ctx.key_audit(desc, vk, section4=s4, multipliers=pic.zw)
        assert ctx.circuit_audit(desc, vk, s4, rd, pd, pic.zw, pic.zh).key.as_dict() == alone.as_dict(), name
        del keep


def test_report_text(ctx, orc):
    pics = CA.pictures()
    assert str(_audit(ctx, orc, pics["clean_toy_sn"])) == "circuit audit: ok"
    assert str(_audit(ctx, orc, pics["clean_toy_no_vk"])) == "circuit audit: ok (not run: IC)"
    text = str(_audit(ctx, orc, pics["c1_moved_toy"]))
    assert text.startswith("circuit audit: FAILED") and "pointsC1 does not belong to the circuit" in text
    row = pics["coeff_row_chain"].report["first_row"][0]
    assert f"coeffs: matrix A differs from the r1cs first at row {row}" in str(_audit(ctx, orc, pics["coeff_row_chain"]))
    assert "ptau tauG2[3] is not in the order-r subgroup" in str(_audit(ctx, orc, pics["ptau_tau_g2_outsider"]))
    assert "ptau tauG2[300] is not in the order-r subgroup (and 1 more)" in \
        str(_audit(ctx, orc, pics["ptau_tau_g2_outsider_chain"]))
    assert "pointsA1[5] is not on the curve" in str(_audit(ctx, orc, pics["a1_off_curve"]))


def test_arguments(ctx, orc):
    from nim_groth16_amd import G16Error
    from nim_groth16_amd._lib import G16_EINVAL
    pic = CA.pictures()["clean_toy_sn"]

    def refused(match, edit=None, zw=None, zh=None, pic=pic):
        desc, vk, s4, rd, pd, keep = _descs(pic, orc)
        if edit:
            edit(desc, rd, pd)
        with pytest.raises(G16Error, match=match) as e:
            ctx.circuit_audit(desc, vk, s4, rd, pd, zw or pic.zw, zh or pic.zh)
        assert e.value.code == G16_EINVAL, match
        del keep

    def zero(zs, i):
        out = list(zs)
        out[i] = 0
        return out
    refused(r"wire: multiplier 5 is zero", zw=zero(pic.zw, 5))
    refused(r"h: multiplier 3 is zero", zh=zero(pic.zh, 3))
    for name in CA.PTAU_SECTIONS:
        refused(r"null ptau section", lambda d, r, p, name=name: setattr(p, name, None))
    refused(r"null", lambda d, r, p: r.val.__setitem__(1, None))
    refused(r"other wire counts", lambda d, r, p: setattr(r, "nvars", pic.nvars + 1))
    refused(r"other wire counts", lambda d, r, p: setattr(r, "npubs", pic.npubs - 1))
    refused(r"log2_domain", lambda d, r, p: setattr(r, "nconstraints", 6))          # 6 + 2 + 1 = 9: a domain of 16
    refused(r"flavour", lambda d, r, p: setattr(r, "flavour", 0))
    refused(r"too short", lambda d, r, p: setattr(p, "power", pic.log2_domain))     # tau^(2n-1) is not in it
    refused(r"sharded", lambda d, r, p: (setattr(d, "shard_index", 0), setattr(d, "shard_count", 2)))
    refused(r"bad proving-key description", lambda d, r, p: setattr(d, "pointsA1", None))    # the key's own shape rules
    for k, (field, val) in ((0, (0, pic.ncons)), (1, (1, pic.nvars))):               # a row, a column out of range
        bad = CA.base("toy")
        ent = list(bad.r1cs[1][1])
        ent[field] = val
        bad.r1cs[1][1] = tuple(ent)
        refused(r"matrix 1 entry 1 out of range", pic=bad)
    bad = CA.base("toy")
    i, w, _ = bad.r1cs[2][2]
    bad.r1cs[2][2] = (i, w, CA.R)                                                    # fr_mont_bytes reduces: plant r itself
    desc, vk, s4, rd, pd, keep = _descs(bad, orc)
    vals = bytearray(ctypes.string_at(rd.val[2], 32 * rd.nnz[2]))
    vals[64:96] = CA.R.to_bytes(32, "little")
    vbuf = _cbuf(bytes(vals))
    rd.val[2] = ctypes.cast(vbuf, ctypes.c_void_p).value
    with pytest.raises(G16Error, match=r"matrix 2 entry 2: value is not canonical") as e:
        ctx.circuit_audit(desc, vk, s4, rd, pd, bad.zw, bad.zh)
    assert e.value.code == G16_EINVAL
    del keep


def _toy_files(ctx, tmp):
    """the toy circuit's .r1cs, .zkey, .ptau and .wtns, key and powers of tau made on the GPU from one toxic waste"""
    from nim_groth16_amd.fake_setup import R1CS, ToxicWaste, fakeCircuitSetup, fakePtau
    from nim_groth16_amd.files import writePtau, writeR1CS, writeWitness, writeZKey
    rng = o.SplitMix64(5)
    tw = ToxicWaste(*[rng.fr() or 1 for _ in range(5)])
    r1cs = R1CS(8, 1, 1, 3, o.toy_r1cs().constraints)
    zk = fakeCircuitSetup(r1cs, tw, 1, ctx)
    pt = fakePtau(tw.tau, tw.alpha, tw.beta, 4, ctx)
    paths = [str(tmp / n) for n in ("toy.r1cs", "toy.zkey", "toy.ptau", "toy.wtns")]
    writeR1CS(paths[0], r1cs)
    writeZKey(paths[1], zk)
    writePtau(paths[2], pt, extraSections=[(7, b"contributions")])
    writeWitness(paths[3], o.TOY_WITNESS)
    return r1cs, zk, pt, paths


def test_clean_key_and_the_audit_touches_no_state(ctx, tmp_path):
    """a key and a ptau made by the library from one toxic waste pass, for the key's own gamma and delta; a proof of the
    key equals g16_prove's bytes before and after the audit"""
    from nim_groth16_amd import Mask, Witness, generateProofWithMask, loadProvingKey
    from nim_groth16_amd.files.zkey import auditCircuit
    r1cs, zk, pt, _ = _toy_files(ctx, tmp_path)
    wt = Witness("bn128", 8, I.fr_mont_bytes(o.TOY_WITNESS))
    pk = loadProvingKey(zk, ctx)
    try:
        before = generateProofWithMask(0, False, zk, wt, Mask(11, 12), ctx, pkey=pk)
        rep = auditCircuit(zk, r1cs, pt, ctx)                     # multipliers drawn afresh
        assert rep.ok and rep.relation == [1] * 9 and rep.key.relation == [1, 1, 1] and str(rep) == "circuit audit: ok"
        after = generateProofWithMask(0, False, zk, wt, Mask(11, 12), ctx, pkey=pk)
        assert (before.pi_a, before.pi_b, before.pi_c) == (after.pi_a, after.pi_b, after.pi_c)
    finally:
        pk.destroy()
    pk2 = loadProvingKey(zk, ctx)                                 # ... and a key created after it
    try:
        again = generateProofWithMask(0, False, zk, wt, Mask(11, 12), ctx, pkey=pk2)
        assert (before.pi_a, before.pi_b, before.pi_c) == (again.pi_a, again.pi_b, again.pi_c)
    finally:
        pk2.destroy()


def test_audit_circuit_raw_and_parsed_agree(ctx, tmp_path):
    from nim_groth16_amd.fake_setup import ToxicWaste, fakeCircuitSetup, fakePtau
    from nim_groth16_amd.files import parsePtau, parseZKey, writePtau, writeZKey
    from nim_groth16_amd.files.zkey import auditCircuit
    from nim_groth16_amd.synthetic import squaringChain
    rng = o.SplitMix64(9)
    r1cs, _ = squaringChain((1 << 9) - 2, seed=4)
    tw = ToxicWaste(*[rng.fr() or 1 for _ in range(5)])
    zk = fakeCircuitSetup(r1cs, tw, 1, ctx)
    zpath, ppath = str(tmp_path / "k.zkey"), str(tmp_path / "p.ptau")
    writeZKey(zpath, zk)
    writePtau(ppath, fakePtau(tw.tau, tw.alpha, tw.beta, 11, ctx))       # a longer ceremony than the circuit needs
    pt = parsePtau(ppath)
    parsed, raw = parseZKey(zpath), parseZKey(zpath, rawCoeffs=True)
    zs = ([(rng.fr() & KA.Z_MAX) or 1 for _ in range(512)], [(rng.fr() & KA.Z_MAX) or 1 for _ in range(512)])
    a, b = auditCircuit(parsed, r1cs, pt, ctx, multipliers=zs), auditCircuit(raw, r1cs, pt, ctx, multipliers=zs)
    assert a.ok and a.as_dict() == b.as_dict() and a.relation == [1] * 9
    # pointsA1[300] replaced by its neighbour, one file coefficient moved to another wire: both keys say the same
    for k in (parsed, raw):
        k.pPoints.pointsA1 = k.pPoints.pointsA1[:64 * 300] + k.pPoints.pointsA1[64 * 301:64 * 302] + k.pPoints.pointsA1[64 * 301:]
    e = next(e for e, ent in enumerate(parsed.coeffs) if ent[0] == 0 and ent[1] >= 7)
    m, r_, c, v = parsed.coeffs[e]
    parsed.coeffs[e] = (m, r_, c + 1, v)
    s4 = bytearray(raw.coeffsSection4)
    s4[4 + 44 * e + 8:4 + 44 * e + 12] = (c + 1).to_bytes(4, "little")
    raw.coeffsSection4 = bytes(s4)
    a, b = auditCircuit(parsed, r1cs, pt, ctx, multipliers=zs), auditCircuit(raw, r1cs, pt, ctx, multipliers=zs)
    assert a.as_dict() == b.as_dict() and not a.ok
    assert a.relation == [0, 1, 1, 0, 1, 1, 1, 1, 1] and a.first_row == [r_, None] and a.key.ok
    assert "pointsA1 does not belong to the circuit" in str(a)
    assert f"matrix A differs from the r1cs first at row {r_}" in str(a)


def test_python_cli_audits_the_circuit_before_it_proves(ctx, tmp_path):
    _, zk, _, (rpath, zpath, ppath, wpath) = _toy_files(ctx, tmp_path)
    tool = os.path.join(ROOT, "tools", "prove_files.py")
    proof = str(tmp_path / "proof.json")
    out = subprocess.run([sys.executable, tool, "-z", zpath, "-w", wpath, "-o", proof, "-i", str(tmp_path / "public.json"),
                          "-n", "-y", "--audit-circuit", rpath, ppath], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    assert "circuit audit: ok" in out.stdout and "verification succeeded" in out.stdout and os.path.exists(proof)
    assert out.stdout.index("circuit audit: ok") < out.stdout.index("verification succeeded")
    # pointsC1[0] replaced by another point of the subgroup: every element check passes, the key proves another statement
    raw = open(zpath, "rb").read()
    old = zk.pPoints.pointsC1[:64]
    assert raw.count(old) == 1
    bad = str(tmp_path / "moved_c1.zkey")
    open(bad, "wb").write(raw.replace(old, zk.specPoints.alpha1))
    proof2 = str(tmp_path / "proof_bad.json")
    out = subprocess.run([sys.executable, tool, "-z", bad, "-w", wpath, "-o", proof2, "-i", str(tmp_path / "public_bad.json"),
                          "-n", "--audit-circuit", rpath, ppath], capture_output=True, text=True, timeout=600)
    assert out.returncode == 2
    assert "circuit audit: FAILED" in out.stdout and "pointsC1 does not belong to the circuit" in out.stdout
    assert not os.path.exists(proof2)


def test_native_cli_audits_the_circuit_before_it_proves(ctx, tmp_path):
    from tests.test_gpu_native_cli import _build
    _, zk, _, (rpath, zpath, ppath, wpath) = _toy_files(ctx, tmp_path)
    exe = _build(tmp_path)
    flags = ["--audit-circuit-r1cs", rpath, "--audit-circuit-ptau", ppath]
    proof = str(tmp_path / "proof.json")
    out = subprocess.run([exe, "-z", zpath, "-w", wpath, "-o", proof, "-i", str(tmp_path / "public.json"), "-n", "-y"] + flags,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    assert "circuit audit: ok" in out.stdout and "verification succeeded" in out.stdout
    assert out.stdout.index("circuit audit: ok") < out.stdout.index("verification succeeded")
    plain = subprocess.run([exe, "-z", zpath, "-w", wpath, "-o", str(tmp_path / "proof0.json"), "-i",
                            str(tmp_path / "public0.json"), "-n"], capture_output=True, text=True, timeout=600)
    assert plain.returncode == 0 and "circuit audit" not in plain.stdout
    assert open(proof).read() == open(tmp_path / "proof0.json").read()     # the audit changes nothing about the proof
    raw = open(zpath, "rb").read()
    old = zk.pPoints.pointsH1[64 * 7:64 * 8]
    assert raw.count(old) == 1
    bad = str(tmp_path / "moved_h1.zkey")
    open(bad, "wb").write(raw.replace(old, zk.specPoints.beta1))
    proof2 = str(tmp_path / "proof_bad.json")
    out = subprocess.run([exe, "-z", bad, "-w", wpath, "-o", proof2, "-i", str(tmp_path / "public_bad.json"), "-n"] + flags,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 2
    assert "circuit audit: FAILED" in out.stdout and "pointsH1 does not belong to the circuit" in out.stdout
    assert not os.path.exists(proof2) and not os.path.exists(tmp_path / "public_bad.json")
    out = subprocess.run([exe, "-z", zpath, "-w", wpath, "-n", "--audit-circuit-r1cs", rpath], capture_output=True, text=True,
                         timeout=600)
    assert out.returncode != 0 and "go together" in out.stderr + out.stdout
