"""g16_points_audit_g1/g2, g16_points_pairs_check and g16_key_audit on the GPU against the integer model of
tests/key_audit_pictures.py (held to itself in tests/test_key_audit_model_cpu.py): every report must equal the model
entry for entry.  Array lengths 1, 63, 64, 65, 255, 256, 257, 301 put defects on both sides of every wave and workgroup
boundary of the 256-lane kernels; a defect beside good lanes in one wave makes the lanes of the order-r ladder diverge."""
import ctypes

import pytest

from oracle import bn254_ref as o
from tests import inputs as I
from tests import key_audit_pictures as KA

pytestmark = pytest.mark.gpu


def _desc(key: KA.Key, raw_coeffs: bool, with_vk: bool = True):
    """-> (PkeyDesc, VkeyDesc or None, section 4 or None, keepalive)"""
    from nim_groth16_amd._lib import PkeyDesc, VkeyDesc
    s = key.sections
    packed = b"".join(m.to_bytes(4, "little") + r_.to_bytes(4, "little") + c.to_bytes(4, "little") + bytes(4) + v
                      for m, r_, c, v in key.coeffs)
    names = ("pointsA1", "pointsB1", "pointsB2", "pointsC1", "pointsH1", None, "alpha1", "beta1", "delta1", "beta2",
             "delta2", "gamma2", "pointsIC")
    bufs = [ctypes.create_string_buffer(x, len(x)) if x else ctypes.create_string_buffer(1)
            for x in (packed if n is None else s[n] for n in names)]
    a = [ctypes.cast(b, ctypes.c_void_p) for b in bufs]
    desc = PkeyDesc(key.nvars, key.npubs, key.log2_domain, 1, a[0], a[1], a[2], a[3], a[4],
                    None if raw_coeffs else a[5], 0 if raw_coeffs else len(key.coeffs), a[6], a[7], a[8], a[9], a[10],
                    0, 1)
    vk = VkeyDesc(key.npubs, a[6], a[9], a[11], a[10], a[12]) if with_vk else None
    return desc, vk, (key.section4() if raw_coeffs else None), bufs


def _audit(ctx, pic: KA.KeyPicture):
    desc, vk, s4, keep = _desc(pic.key, pic.raw_coeffs, pic.with_vk)
    rep = ctx.key_audit(desc, vk, section4=s4, multipliers=pic.multipliers)
    del keep
    return rep


@pytest.mark.parametrize("group", [1, 2])
def test_point_arrays(ctx, group):
    pics = [p for p in KA.array_pictures() if p.group == group]
    assert len(pics) > 20
    for p in pics:
        got = ctx.points_audit(group, p.raw)
        assert got == (p.first_bad, p.bad_count), (p.name, got, (p.first_bad, p.bad_count))


@pytest.mark.parametrize("n", [1, 2, 65, 301])
def test_pairs_check(ctx, n):
    pics = [p for p in KA.relation_pictures() if len(p.a) == n]
    assert len(pics) >= 2
    for p in pics:
        assert ctx.pairs_check(p.g1, p.g2, p.multipliers) == bool(p.result), p.name
    assert ctx.pairs_check(b"", b"", []) is True


FAMILIES = {"clean": ("clean",), "points": ("a1_", "h1_", "c1_", "ic_", "alpha1_", "two_"), "g2": ("b2_", "b1_", "gamma2_", "beta2_"),
            "coeffs": ("coeff_",), "relations": ("rel_",)}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_key_pictures(ctx, family):
    pics = KA.key_pictures()
    assert sorted(n for n in pics if n.startswith(tuple(p for f in FAMILIES.values() for p in f))) == sorted(pics)
    mine = {n: p for n, p in pics.items() if n.startswith(FAMILIES[family])}
    assert len(mine) >= 4
    for name, pic in mine.items():
        rep = _audit(ctx, pic)
        assert rep.as_dict() == pic.report, (name, rep.as_dict(), pic.report)
        assert rep.ok == (pic.report["failed"] == 0)


def test_report_text(ctx):
    pics = KA.key_pictures()
    text = str(_audit(ctx, pics["two_sections"]))
    assert "pointsA1[0] is not on the curve (and 1 more)" in text and "pointsB2[2] is not in the order-r subgroup" in text
    text = str(_audit(ctx, pics["rel_delta2_inf"]))
    assert "delta1~delta2" in text and "delta2 is the point at infinity" in text
    assert str(_audit(ctx, pics["clean_no_multipliers"])) == "key audit: ok (not run: pointsB1~pointsB2)"


def test_arguments(ctx):
    from nim_groth16_amd import G16Error
    from nim_groth16_amd._lib import G16_EINVAL
    pic = KA.key_pictures()["clean"]
    zs = list(pic.multipliers)
    zs[5] = 0
    desc, vk, s4, keep = _desc(pic.key, False)
    with pytest.raises(G16Error, match=r"multiplier 5 is zero") as e:
        ctx.key_audit(desc, vk, multipliers=zs)
    assert e.value.code == G16_EINVAL
    rel = KA.relation_pictures()[0]
    z2 = list(rel.multipliers)
    z2[1] = 0
    with pytest.raises(G16Error, match=r"multiplier 1 is zero") as e:
        ctx.pairs_check(rel.g1, rel.g2, z2)
    assert e.value.code == G16_EINVAL
    desc.shard_index, desc.shard_count = 0, 2                  # a sharded description
    with pytest.raises(G16Error, match=r"sharded") as e:
        ctx.key_audit(desc, vk, multipliers=pic.multipliers)
    assert e.value.code == G16_EINVAL
    desc.shard_count = 1
    for edit in ((0, 2), (1, 1 << pic.key.log2_domain), (2, pic.key.nvars)):      # matrix C, row, column out of range
        key = KA.toy_key()
        ent = list(key.coeffs[2])
        ent[edit[0]] = edit[1]
        key.coeffs[2] = tuple(ent)
        for raw in (False, True):
            d2, v2, s42, keep2 = _desc(key, raw)
            with pytest.raises(G16Error, match=r"coefficient entry 2 out of range") as e:
                ctx.key_audit(d2, v2, section4=s42, multipliers=pic.multipliers)
            assert e.value.code == G16_EINVAL
    d2, v2, s42, keep2 = _desc(KA.toy_key(), True)
    with pytest.raises(G16Error, match=r"length of the coefficient section"):
        ctx.key_audit(d2, v2, section4=s42[:-1], multipliers=pic.multipliers)
    del keep, keep2


def _toy_zkey(ctx):
    from nim_groth16_amd.fake_setup import R1CS, ToxicWaste, fakeCircuitSetup
    rng = o.SplitMix64(5)
    tw = ToxicWaste(*[rng.fr() or 1 for _ in range(5)])
    return fakeCircuitSetup(R1CS(8, 1, 1, 3, o.toy_r1cs().constraints), tw, 1, ctx)


def test_clean_key_and_the_audit_touches_no_state(ctx):
    """a proof of the key equals g16_prove's bytes before and after the audit"""
    from nim_groth16_amd import Mask, Witness, generateProofWithMask, loadProvingKey
    from nim_groth16_amd.files.zkey import auditZKey
    zk = _toy_zkey(ctx)
    wt = Witness("bn128", 8, I.fr_mont_bytes(o.TOY_WITNESS))
    pk = loadProvingKey(zk, ctx)
    try:
        before = generateProofWithMask(0, False, zk, wt, Mask(11, 12), ctx, pkey=pk)
        rep = auditZKey(zk, ctx)                                  # multipliers drawn afresh
        assert rep.ok and rep.failed == 0 and rep.relation == [1, 1, 1] and str(rep) == "key audit: ok"
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


def test_audit_zkey_raw_and_parsed_agree(ctx, tmp_path):
    from nim_groth16_amd.files import parseZKey, writeZKey
    from nim_groth16_amd.files.zkey import auditZKey
    from nim_groth16_amd.synthetic import squaringChain
    from nim_groth16_amd.fake_setup import ToxicWaste, fakeCircuitSetup
    rng = o.SplitMix64(9)
    r1cs, _ = squaringChain((1 << 9) - 2, seed=4)                 # 512 wires: the arrays span two workgroups
    zk = fakeCircuitSetup(r1cs, ToxicWaste(*[rng.fr() or 1 for _ in range(5)]), 1, ctx)
    path = str(tmp_path / "k.zkey")
    writeZKey(path, zk)
    parsed, raw = parseZKey(path), parseZKey(path, rawCoeffs=True)
    zs = [(rng.fr() & KA.Z_MAX) or 1 for _ in range(parsed.header.nvars)]
    a, b = auditZKey(parsed, ctx, multipliers=zs), auditZKey(raw, ctx, multipliers=zs)
    assert a.ok and a.as_dict() == b.as_dict()
    # one B2 point replaced by the point of order 10069, one file coefficient by r: both keys say the same
    small = o.g2_to_bytes(KA.twist_outsiders()["small"])
    for k in (parsed, raw):
        k.pPoints.pointsB2 = k.pPoints.pointsB2[:128 * 300] + small + k.pPoints.pointsB2[128 * 301:]
    m, r_, c, _ = parsed.coeffs[7]
    parsed.coeffs[7] = (m, r_, c, KA.R.to_bytes(32, "little"))
    s4 = bytearray(raw.coeffsSection4)
    s4[4 + 44 * 7 + 12:4 + 44 * 8] = KA.R.to_bytes(32, "little")
    raw.coeffsSection4 = bytes(s4)
    a, b = auditZKey(parsed, ctx, multipliers=zs), auditZKey(raw, ctx, multipliers=zs)
    assert a.as_dict() == b.as_dict() and not a.ok
    assert a.failed == KA.SUBGROUP | KA.CANONICAL and a.relation == [-1, 1, 1]
    assert a.first_bad[KA.SECTIONS.index("pointsB2")] == [None, None, 300]
    assert a.first_bad[KA.SECTIONS.index("coeffs")] == [7, None, None]
    assert "pointsB2[300] is not in the order-r subgroup" in str(a) and "coeffs[7] is not a canonical encoding" in str(a)
