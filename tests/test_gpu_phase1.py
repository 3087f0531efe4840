"""The per-point scaling and the phase-1 contribution on the GPU: g16_points_scale_each_g1/g2, g16_ptau_contribute.
Everything is byte-exact; the contributed powers must be fakePtau's for the product of the secrets.  Points are known
multiples of the generators (the C oracle's fixed-base multiplier over integer logarithms), so k_i * P_i is fixed_base(k_i * log_i mod
r); a handful of points go through oracle.G1.mul / G2.mul directly.  The scalars: tests/phase1_scalars.py."""
import ctypes

import pytest

from oracle import bn254_ref as o
from tests import inputs as I
from tests import phase1_scalars as PS

pytestmark = pytest.mark.gpu
R = o.R
PSZ = {1: 64, 2: 128}
TILE, GROUP_STRIDE, GROUP = 256, 64, 4   # SCALE_BLOCK * SCALE_GROUP points per workgroup; a lane's four points lie 64 apart


def _each(ctx, orc, group, logs, ks, mont=True):
    """k_i * fixed_base(log_i) must be fixed_base(k_i * log_i); a zero logarithm is the point (0,0)"""
    assert len(logs) == len(ks)
    pts = orc.fixed_base(group, I.fr_mont_bytes(logs)) if logs else b""
    kb = I.fr_mont_bytes(ks) if mont else I.fr_std_bytes(ks)
    got = ctx.points_scale_each(group, pts, kb, mont=mont)
    exp = orc.fixed_base(group, I.fr_mont_bytes([k * x % R for k, x in zip(ks, logs)])) if logs else b""
    if got != exp:
        p = PSZ[group]
        i = next(i for i in range(len(logs)) if got[p * i:p * (i + 1)] != exp[p * i:p * (i + 1)])
        raise AssertionError(f"G{group}, n = {len(logs)}: output {i} differs (the first of them), k = {ks[i]:#x}")
    return pts, got


def _logs(n, seed, zeros=()):
    rng = o.SplitMix64(seed)
    logs = [rng.fr() or 1 for _ in range(n)]
    for i in zeros:
        logs[i] = 0
    return logs


def _cycle(ks, n):
    return [ks[i % len(ks)] for i in range(n)]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_each_g1_sizes(ctx, orc, n):
    """a lane, a wave and the 64 x 4 tile of a workgroup: one below, at and one above; four workgroups"""
    for mont in (True, False):
        _each(ctx, orc, 1, _logs(n, n), PS.random_scalars(n, 500 + n), mont)


@pytest.mark.parametrize("mont", [True, False])
def test_each_g1_edge_scalars(ctx, orc, mont):
    """every edge scalar in its own lane, at two offsets so that each meets other neighbours in its wave"""
    ks = PS.edge_scalars()
    n = 2 * TILE + 37
    for shift in (0, 29):
        _each(ctx, orc, 1, _logs(n, 5 + shift, zeros=(0, n - 1)), _cycle(ks[shift:] + ks[:shift], n), mont)


def test_each_g1_every_lane_another_length(ctx, orc):
    """s_i = 2^i: every lane of a wave ends its leading zeros somewhere else; then the lengths in descending order"""
    ks = PS.powers_of_two()
    _each(ctx, orc, 1, _logs(len(ks), 71), ks)
    _each(ctx, orc, 1, _logs(len(ks), 72), ks[::-1], mont=False)


def test_each_g1_all_equal_is_the_uniform_scaling(ctx, orc):
    n = TILE + 9
    logs = _logs(n, 81, zeros=(3,))
    for k in (PS.random_scalars(1, 82)[0], R - 1, 1):
        pts, got = _each(ctx, orc, 1, logs, [k] * n)
        assert got == ctx.points_scale(1, pts, I.fr_mont_bytes([k]))
    assert _each(ctx, orc, 1, logs, [0] * n)[1] == bytes(64 * n)


def test_each_g1_infinity(ctx, orc):
    """(0,0) in every fourth slot; at every position of one lane's group of four (lane 5: points 5 + 64 j), filling it,
    filling a whole workgroup and the whole array, and zero scalars at the same places; then each member alone and each
    alone alive"""
    n = TILE + 37
    ks = PS.random_scalars(n, 91)
    members = [5 + GROUP_STRIDE * j for j in range(GROUP)]
    for zeros in (tuple(range(0, n, 4)), tuple(members), tuple(range(TILE)), tuple(range(n))):
        _each(ctx, orc, 1, _logs(n, 92, zeros), ks)
        zs = set(zeros)
        _each(ctx, orc, 1, _logs(n, 93), [0 if i in zs else k for i, k in enumerate(ks)])
    for zeros in [(m,) for m in members] + [tuple(m for m in members if m != keep) for keep in members]:
        _each(ctx, orc, 1, _logs(n, 92, zeros), ks)


def test_each_g1_in_place_and_the_python_oracle(ctx, orc):
    n = 70
    logs, ks = _logs(n, 17, zeros=(2,)), PS.random_scalars(n, 18)
    pts, got = _each(ctx, orc, 1, logs, ks)
    for i in (0, 2, 69):
        assert o.g1_from_bytes(got[64 * i:64 * i + 64]) == o.G1.mul(ks[i], o.g1_from_bytes(pts[64 * i:64 * i + 64]))
    buf = ctypes.create_string_buffer(pts, len(pts))
    ctx._check(ctx._lib.g16_points_scale_each_g1(ctx._h, buf, n, I.fr_std_bytes(ks), 0, buf))     # out == points
    assert buf.raw == got


@pytest.mark.parametrize("n", [1, 65, 257])
def test_each_g2(ctx, orc, n):
    zeros = () if n < 4 else (0, n - 1, 2)
    ks = _cycle(PS.edge_scalars() + PS.random_scalars(40, 700 + n), n)
    _each(ctx, orc, 2, _logs(n, 3 * n, zeros), ks, mont=bool(n & 2))


def test_each_g2_lengths_equal_zero_in_place(ctx, orc):
    ks = PS.powers_of_two()[::9]
    pts, got = _each(ctx, orc, 2, _logs(len(ks), 8, zeros=(1,)), ks)
    i = len(ks) - 1
    assert o.g2_from_bytes(got[128 * i:128 * i + 128]) == o.G2.mul(ks[i], o.g2_from_bytes(pts[128 * i:128 * i + 128]))
    n = 66
    logs, k = _logs(n, 9, zeros=(4, 5, 6, 7)), PS.random_scalars(1, 10)[0]
    pts, got = _each(ctx, orc, 2, logs, [k] * n, mont=False)
    assert got == ctx.points_scale(2, pts, I.fr_mont_bytes([k]))
    assert _each(ctx, orc, 2, logs, [0] * n)[1] == bytes(128 * n)
    buf = ctypes.create_string_buffer(pts, len(pts))
    ctx._check(ctx._lib.g16_points_scale_each_g2(ctx._h, buf, n, I.fr_mont_bytes([k] * n), 1, buf))
    assert buf.raw == got


def test_each_arguments(ctx, orc):
    from nim_groth16_amd import G16Error
    from nim_groth16_amd._lib import G16_EINVAL
    pts = orc.fixed_base(1, I.fr_mont_bytes([5, 6, 7]))
    ks = I.fr_std_bytes([1, 2]) + R.to_bytes(32, "little")
    with pytest.raises(G16Error, match=r"scalar 2 is not canonical \(>= r\)") as e:
        ctx.points_scale_each(1, pts, ks, mont=False)
    assert e.value.code == G16_EINVAL
    with pytest.raises(G16Error, match=r"scalar 0 is not canonical") as e:
        ctx.points_scale_each(2, orc.fixed_base(2, I.fr_mont_bytes([5])), b"\xff" * 32)
    assert e.value.code == G16_EINVAL
    out = ctypes.create_string_buffer(192)
    ok = I.fr_std_bytes([1, 2, 3])
    for fn in (ctx._lib.g16_points_scale_each_g1, ctx._lib.g16_points_scale_each_g2):
        for args, match in (((None, 3, ok, 0, out), "null pointer"), ((pts, 3, None, 0, out), "null pointer"),
                            ((pts, 3, ok, 0, None), "null pointer"), ((pts, 3, ok, 7, out), "flags"),
                            ((pts, 1 << 31, ok, 0, out), "out of range")):
            with pytest.raises(G16Error, match=match) as e:
                ctx._check(fn(ctx._h, *args))
            assert e.value.code == G16_EINVAL
        ctx._check(fn(ctx._h, None, 0, None, 0, None))                                             # n == 0: nothing to do


def test_each_leaves_the_context_as_it_was(ctx, orc):
    """a context proves the same bytes before and after the new calls"""
    from nim_groth16_amd import loadProvingKey
    from tests import circuit_audit_pictures as CA
    from tests.test_gpu_circuit_setup import _fake, _waste
    from tests.test_gpu_phase2 import _proof_bytes
    zk = _fake(ctx, "toy", CA.SNARKJS, _waste("toy").delta)
    pk = loadProvingKey(zk, ctx)
    try:
        before = _proof_bytes(ctx, zk, pk)
        _each(ctx, orc, 1, _logs(300, 1), PS.random_scalars(300, 2))
        _each(ctx, orc, 2, _logs(5, 3), PS.random_scalars(5, 4))
        assert _proof_bytes(ctx, zk, pk) == before
    finally:
        pk.destroy()


# ---- g16_ptau_contribute -----------------------------------------------------------------------------------------------------
SECTIONS = ("tauG1", "tauG2", "alphaTauG1", "betaTauG1", "betaG2")


def _arrays(pt):
    return {k: bytes(getattr(pt, k)) for k in SECTIONS}


def _secrets(seed):
    rng = o.SplitMix64(seed)
    return [rng.fr() or 1 for _ in range(6)]                                    # t, a, b, s_t, s_a, s_b


def _record_model(orc, waste, secrets, challenge_logs):
    """the record of a contribution (t, a, b; s_t, s_a, s_b) that leads to the powers of `waste` = (tau, alpha, beta), with
    challenge points c_x gen2: all of it fixed-base multiples of known logarithms"""
    tau, alpha, beta = waste
    g1 = orc.fixed_base(1, I.fr_mont_bytes([tau, alpha, beta]))
    g2 = orc.fixed_base(2, I.fr_mont_bytes([tau, beta]))
    out = g1 + g2
    for x, s, c in zip(secrets[:3], secrets[3:], challenge_logs):
        out += orc.fixed_base(1, I.fr_mont_bytes([s, x * s % R])) + orc.fixed_base(2, I.fr_mont_bytes([x * c % R]))
    return out


@pytest.mark.parametrize("power", [3, 8])
def test_contribute_equals_fake_ptau(ctx, orc, power):
    """contribute(newPtau(p), t, a, b) == fakePtau(t, a, b, p); a second contribution, in standard form, gives
    fakePtau(t1 t2, a1 a2, b1 b2, p); both records are the model's"""
    from nim_groth16_amd import phase1
    from nim_groth16_amd.fake_setup import fakePtau
    s1, s2 = _secrets(40 + power), _secrets(50 + power)
    clogs = [7, 8, 9]
    ch = orc.fixed_base(2, I.fr_mont_bytes(clogs))
    p0 = _arrays(phase1.newPtau(power))
    assert p0 == _arrays(fakePtau(1, 1, 1, power, ctx))
    enc = lambda v: I.fr_mont_bytes([v])                                          # noqa: E731
    p1, rec1 = ctx.ptau_contribute(p0, enc(s1[0]), enc(s1[1]), enc(s1[2]), I.fr_mont_bytes(s1[3:]), ch)
    assert p1 == _arrays(fakePtau(s1[0], s1[1], s1[2], power, ctx))
    assert rec1 == _record_model(orc, s1[:3], s1, clogs) and len(rec1) == 1216
    std = lambda v: I.fr_std_bytes([v])                                           # noqa: E731
    p2, rec2 = ctx.ptau_contribute(p1, std(s2[0]), std(s2[1]), std(s2[2]), I.fr_std_bytes(s2[3:]), ch, mont=False)
    waste = [x * y % R for x, y in zip(s1[:3], s2[:3])]
    assert p2 == _arrays(fakePtau(waste[0], waste[1], waste[2], power, ctx))
    assert rec2 == _record_model(orc, waste, s2, clogs)


def test_contribute_with_the_transcript(ctx, orc):
    """phase1.contribute twice: the powers of the products, a log of two records whose challenges re-derive, and a
    g2_spx that is t times the hashed challenge point by the Python oracle"""
    from nim_groth16_amd import phase1, phase2
    from nim_groth16_amd.fake_setup import fakePtau
    s1, s2 = _secrets(61), _secrets(62)
    pt, log = phase1.contribute(phase1.newPtau(3), None, *s1[:3], name="alice", ctx=ctx, pok_secrets=s1[3:])
    pt, log = phase1.contribute(pt, log, *s2[:3], name="bob", ctx=ctx, pok_secrets=s2[3:])
    waste = [x * y % R for x, y in zip(s1[:3], s2[:3])]
    assert _arrays(pt) == _arrays(fakePtau(waste[0], waste[1], waste[2], 3, ctx))
    assert log.names == ["alice", "bob"] and [len(r) for r in log.records] == [1216, 1216]
    ch = phase1.challenges(log)
    assert len(ch) == 2 and ch[0] != ch[1] and len(set(ch[1][128 * x:128 * x + 128] for x in range(3))) == 3
    tr = phase1.transcript_hash(log, 1, phase1.record_pok_g1(log.records[1]))
    want = o.G2.mul(s2[0], phase2.hash_to_g2(tr + b"\0"))
    assert o.g2_from_bytes(log.records[1][448 + 128:448 + 256]) == want
    assert log.records[1][:64] == pt.tauG1[64:128] and log.records[1][320:448] == pt.betaG2
    drawn, _ = phase1.contribute(phase1.newPtau(3), ctx=ctx)                       # secrets nobody knows
    assert drawn.tauG1[:64] == pt.tauG1[:64] and drawn.tauG1[64:128] != phase1.gen1_bytes()


def test_contribute_refusals(ctx, orc):
    from nim_groth16_amd import G16Error, phase1
    from nim_groth16_amd._lib import G16_EINVAL, PtauContributionC, PtauDesc, PtauOut
    p0 = _arrays(phase1.newPtau(3))
    one, s3, ch = I.fr_mont_bytes([1]), I.fr_mont_bytes([2, 3, 4]), orc.fixed_base(2, I.fr_mont_bytes([7, 8, 9]))

    def refused(match, fn):
        with pytest.raises(G16Error, match=match) as e:
            fn()
        assert e.value.code == G16_EINVAL, match

    def planted(section, index, raw):
        psz = len(raw)
        b = bytearray(p0[section])
        b[psz * index:psz * (index + 1)] = raw
        return {**p0, section: bytes(b)}
    refused("t must be non-zero", lambda: ctx.ptau_contribute(p0, bytes(32), one, one, s3, ch))
    refused("a must be non-zero and canonical", lambda: ctx.ptau_contribute(p0, one, R.to_bytes(32, "little"), one, s3, ch, mont=False))
    refused("b must be non-zero", lambda: ctx.ptau_contribute(p0, one, one, bytes(32), s3, ch))
    refused("s must be non-zero", lambda: ctx.ptau_contribute(p0, one, one, one, s3[:64] + bytes(32), ch))
    refused(r"ptau alphaTauG1\[7\] is the point at infinity", lambda: ctx.ptau_contribute(planted("alphaTauG1", 7, bytes(64)), one, one, one, s3, ch))
    refused(r"challenges\[1\] is the point at infinity", lambda: ctx.ptau_contribute(p0, one, one, one, s3, ch[:128] + bytes(128) + ch[256:]))
    small = KA_small_order_g2()
    refused(r"ptau tauG2\[3\] is not in the order-r subgroup", lambda: ctx.ptau_contribute(planted("tauG2", 3, small), one, one, one, s3, ch))
    refused(r"challenges\[2\] is not in the order-r subgroup", lambda: ctx.ptau_contribute(p0, one, one, one, s3, ch[:256] + small))
    off = I.fr_mont_bytes([1]) + I.fr_mont_bytes([1])                            # (1, 1) in Montgomery limbs: not on y^2 = x^3 + 3
    refused(r"ptau tauG1\[14\] is not on the curve", lambda: ctx.ptau_contribute(planted("tauG1", 14, off), one, one, one, s3, ch))
    alias = (o.P + 1).to_bytes(32, "little") + p0["betaTauG1"][32:64]
    refused(r"ptau betaTauG1\[0\] is not a canonical encoding", lambda: ctx.ptau_contribute(planted("betaTauG1", 0, alias), one, one, one, s3, ch))
    refused("power out of range", lambda: ctx.ptau_contribute(p0, one, one, one, s3, ch, power=26))    # refused before any read
    refused("power out of range", lambda: ctx.ptau_contribute(p0, one, one, one, s3, ch, power=0))
    keep = [ctypes.create_string_buffer(v, len(v)) for v in p0.values()]
    desc = PtauDesc(3, *[ctypes.cast(b, ctypes.c_void_p) for b in keep])
    outb = [ctypes.create_string_buffer(len(v)) for v in p0.values()]
    out, rec = PtauOut(*[ctypes.cast(b, ctypes.c_void_p) for b in outb]), PtauContributionC()
    fn = ctx._lib.g16_ptau_contribute
    refused("null argument", lambda: ctx._check(fn(ctx._h, None, one, one, one, s3, 1, ch, ctypes.byref(out), ctypes.byref(rec))))
    refused("null argument", lambda: ctx._check(fn(ctx._h, ctypes.byref(desc), one, one, one, s3, 1, ch, ctypes.byref(out), None)))
    refused("null argument", lambda: ctx._check(fn(ctx._h, ctypes.byref(desc), one, one, one, None, 1, ch, ctypes.byref(out), ctypes.byref(rec))))
    refused("null output pointer", lambda: ctx._check(fn(ctx._h, ctypes.byref(desc), one, one, one, s3, 1, ch, ctypes.byref(PtauOut()), ctypes.byref(rec))))
    refused("null ptau pointer", lambda: ctx._check(fn(ctx._h, ctypes.byref(PtauDesc(3)), one, one, one, s3, 1, ch, ctypes.byref(out), ctypes.byref(rec))))
    refused("flags", lambda: ctx._check(fn(ctx._h, ctypes.byref(desc), one, one, one, s3, 5, ch, ctypes.byref(out), ctypes.byref(rec))))
    ctx._check(fn(ctx._h, ctypes.byref(desc), one, one, one, s3, 1, ch, ctypes.byref(out), ctypes.byref(rec)))   # and the legal call
    assert [b.raw for b in outb] == list(p0.values())                               # t = a = b = 1: the same powers


def KA_small_order_g2():
    """a point of the twist outside the order-r subgroup, as the key audit's pictures plant it"""
    from tests import key_audit_pictures as KA
    return o.g2_to_bytes(KA.twist_outsiders()["small"])


# ---- the loop: generators -> contributions -> circuit setup -> proof -------------------------------------------------------
def test_the_loop_on_the_toy_circuit(ctx, orc):
    """newPtau, two contributions, circuitSetup: the key is fakeCircuitSetup's for the toxic waste (a1 a2, b1 b2, 1, 1,
    t1 t2) byte for byte, and a proof from it verifies; the context proves the same bytes before and after a
    contribution"""
    from nim_groth16_amd import Mask, Witness, extractVKey, generateProofWithMask, loadProvingKey, phase1, verifyProof
    from nim_groth16_amd.fake_setup import R1CS, ToxicWaste, fakeCircuitSetup
    from nim_groth16_amd.setup import circuitSetup
    from tests import circuit_audit_pictures as CA
    from tests.test_gpu_circuit_setup import _assert_same_key
    from tests.test_gpu_phase2 import _proof_bytes
    s1, s2 = _secrets(71), _secrets(72)
    pt, log = phase1.contribute(phase1.newPtau(4), None, *s1[:3], ctx=ctx, pok_secrets=s1[3:])
    pt, log = phase1.contribute(pt, log, *s2[:3], ctx=ctx, pok_secrets=s2[3:])
    rep = phase1.verifyPtau(pt, log, ctx=ctx)
    assert rep.ok and rep.relation == [1] * 10, str(rep)
    r1cs = R1CS(8, 1, 1, 3, o.toy_r1cs().constraints)
    zk = circuitSetup(r1cs, pt, ctx=ctx)
    t, a, b = (x * y % R for x, y in zip(s1[:3], s2[:3]))
    _assert_same_key(zk, fakeCircuitSetup(r1cs, ToxicWaste(a, b, 1, 1, t), CA.SNARKJS, ctx), "the loop")
    pk = loadProvingKey(zk, ctx)
    try:
        before = _proof_bytes(ctx, zk, pk)
        phase1.contribute(pt, log, ctx=ctx)
        assert _proof_bytes(ctx, zk, pk) == before
        assert phase1.verifyPtau(pt, log, ctx=ctx).ok
        assert _proof_bytes(ctx, zk, pk) == before
        pr = generateProofWithMask(0, False, zk, Witness("bn128", 8, I.fr_mont_bytes(o.TOY_WITNESS)), Mask(21, 22), ctx, pkey=pk)
    finally:
        pk.destroy()
    assert verifyProof(extractVKey(zk), pr, ctx)


def test_the_loop_on_files(ctx, tmp_path):
    """tools/ptau_files.py new + contribute twice + verify (exit 2 on a doubled element), then prove_files.py --setup-ptau
    on the result: a verified proof, and no toxic waste in any command"""
    import os
    import subprocess
    import sys

    from nim_groth16_amd import phase1
    from nim_groth16_amd.fake_setup import R1CS
    from nim_groth16_amd.files import parsePtau, parsePtauContributions, writeR1CS, writeWitness
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tool, prove = os.path.join(root, "tools", "ptau_files.py"), os.path.join(root, "tools", "prove_files.py")
    p0, p1, p2, rpath, wpath = (str(tmp_path / n) for n in ("p0.ptau", "p1.ptau", "p2.ptau", "toy.r1cs", "toy.wtns"))

    def run(*args):
        return subprocess.run([sys.executable, *args], capture_output=True, text=True, timeout=600)
    out = run(tool, "new", "4", "-o", p0)
    assert out.returncode == 0 and "new: wrote" in out.stdout, out.stderr
    out = run(tool, "contribute", p0, "-o", p1, "--name", "alice")
    assert out.returncode == 0 and "contribution 1 (alice): wrote" in out.stdout, out.stderr
    out = run(tool, "contribute", p1, "-o", p2)
    assert out.returncode == 0 and "contribution 2: wrote" in out.stdout, out.stderr
    records, names = parsePtauContributions(p2)
    assert names == ["alice", ""] and records[0] == parsePtauContributions(p1)[0][0]
    pt = parsePtau(p2)
    assert records[1][:64] == pt.tauG1[64:128] != parsePtau(p1).tauG1[64:128] and pt.tauG1[:64] == phase1.gen1_bytes()
    out = run(tool, "verify", p2)
    assert out.returncode == 0 and "ptau: ok" in out.stdout and "2 records" in out.stdout, out.stdout + out.stderr
    # the same file with tauG1[9] doubled (still on the curve): exit code 2, TAU_G1 named
    from nim_groth16_amd.files import contributionsSection, writePtau
    g = o.G1.mul(2, o.g1_from_bytes(pt.tauG1[64 * 9:64 * 10]))
    pt.tauG1 = pt.tauG1[:64 * 9] + o.g1_to_bytes(g) + pt.tauG1[64 * 10:]
    bad = str(tmp_path / "bad.ptau")
    writePtau(bad, pt, extraSections=[(7, contributionsSection(records, names))])
    out = run(tool, "verify", bad)
    assert out.returncode == 2 and "ptau: FAILED" in out.stdout and "TAU_G1 fails" in out.stdout, out.stdout + out.stderr
    writeR1CS(rpath, R1CS(8, 1, 1, 3, o.toy_r1cs().constraints))
    writeWitness(wpath, o.TOY_WITNESS)
    out = run(prove, "--setup-ptau", p2, "-r", rpath, "-z", str(tmp_path / "toy.zkey"), "-w", wpath, "-o",
              str(tmp_path / "proof.json"), "-i", str(tmp_path / "public.json"), "-y")
    assert out.returncode == 0 and "verification succeeded" in out.stdout, out.stdout + out.stderr


# ---- g16_ptau_contribute in chunks ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [1, 5, 8])
def test_contribute_in_chunks(ctx, orc, chunk, monkeypatch):
    """the chunk loop of the long arrays with a chunk of 1, 5 and 8 points at power 3 (tauG1 has 15: a restart scalar
    t^at per chunk, a short last chunk, the buffers reused): the same powers as in one piece"""
    from nim_groth16_amd import phase1
    from nim_groth16_amd.fake_setup import fakePtau
    x = _secrets(33)
    ch = orc.fixed_base(2, I.fr_mont_bytes([7, 8, 9]))
    enc = lambda v: I.fr_mont_bytes([v])                                          # noqa: E731
    p0 = _arrays(fakePtau(5, 6, 7, 3, ctx))
    whole, rec = ctx.ptau_contribute(p0, enc(x[0]), enc(x[1]), enc(x[2]), I.fr_mont_bytes(x[3:]), ch)
    assert whole == _arrays(fakePtau(5 * x[0] % R, 6 * x[1] % R, 7 * x[2] % R, 3, ctx))
    monkeypatch.setenv("G16_PTAU_CHUNK", str(chunk))
    assert ctx.ptau_contribute(p0, enc(x[0]), enc(x[1]), enc(x[2]), I.fr_mont_bytes(x[3:]), ch) == (whole, rec)


# ---- g16_ptau_verify -------------------------------------------------------------------------------------------------------------
def _pictures():
    from tests import phase1_pictures as P1
    return P1.pictures()


@pytest.mark.parametrize("name", sorted(_pictures()))
def test_verify_gives_the_models_report(ctx, orc, name):
    """every picture of tests/phase1_pictures.py: exactly the report of the log-space model"""
    import functools

    from tests import phase1_pictures as P1
    pic = _pictures()[name]
    fixed = functools.lru_cache(None)(lambda g, logs: orc.fixed_base(g, I.fr_mont_bytes(list(logs))))
    arrays, recs, chs = P1.encode(pic, fixed)
    rep = ctx.ptau_verify(arrays, recs, chs, pic.multipliers)
    assert rep.as_dict() == pic.report, (name, str(rep))
    assert rep.ok == (pic.report["failed"] == 0)


def test_verify_a_contributed_file_with_its_transcript(ctx, orc):
    """what g16_ptau_contribute wrote, with the challenges re-derived from the records: everything holds; the records of
    first step of another chain: STEP fails at record 0, and POK at record 1, whose challenges hash record 0"""
    from nim_groth16_amd import phase1
    s1, s2 = _secrets(81), _secrets(82)
    pt, log = phase1.contribute(phase1.newPtau(3), None, *s1[:3], ctx=ctx, pok_secrets=s1[3:])
    pt, log = phase1.contribute(pt, log, *s2[:3], ctx=ctx, pok_secrets=s2[3:])
    rep = phase1.verifyPtau(pt, log, ctx=ctx)
    assert rep.relation == [1] * 10 and rep.ok, str(rep)
    assert phase1.verifyPtau(pt, None, ctx=ctx).relation == [1] * 7 + [-1] * 3
    assert phase1.verifyPtau(phase1.newPtau(3), phase1.PtauContributions(power=3), ctx=ctx).relation == [1] * 10
    _, other = phase1.contribute(phase1.newPtau(3), None, *s2[:3], ctx=ctx, pok_secrets=s2[3:])
    log.records[0] = other.records[0][:448] + log.records[0][448:]              # after-values of another first step
    rep = phase1.verifyPtau(pt, log, ctx=ctx)
    assert rep.relation == [1] * 7 + [0, 0, 1] and rep.first_record == [1, 0], str(rep)


def test_verify_refusals(ctx, orc):
    from nim_groth16_amd import G16Error, phase1
    from nim_groth16_amd._lib import G16_EINVAL, PtauContributionC, PtauDesc, PtauReportC
    p0 = _arrays(phase1.newPtau(3))
    z = [3] * 14

    def refused(match, fn):
        with pytest.raises(G16Error, match=match) as e:
            fn()
        assert e.value.code == G16_EINVAL, match
    refused("multiplier 9 is zero", lambda: ctx.ptau_verify(p0, None, None, z[:9] + [0] + z[10:]))
    refused("multiplier 0 is zero", lambda: ctx.ptau_verify(p0, [], [], [0] + z[1:]))
    refused("power out of range", lambda: ctx.ptau_verify(p0, None, None, z, power=26))
    refused("power out of range", lambda: ctx.ptau_verify(p0, None, None, z, power=0))
    keep = [ctypes.create_string_buffer(v, len(v)) for v in p0.values()]
    desc = PtauDesc(3, *[ctypes.cast(b, ctypes.c_void_p) for b in keep])
    rep, zb, fn = PtauReportC(), bytes([1]) * (16 * 14), ctx._lib.g16_ptau_verify
    refused("null argument", lambda: ctx._check(fn(ctx._h, None, None, None, 0, zb, ctypes.byref(rep))))
    refused("null argument", lambda: ctx._check(fn(ctx._h, ctypes.byref(desc), None, None, 0, None, ctypes.byref(rep))))
    refused("null argument", lambda: ctx._check(fn(ctx._h, ctypes.byref(desc), None, None, 0, zb, None)))
    refused("null argument", lambda: ctx._check(fn(ctx._h, ctypes.byref(desc), None, None, 1, zb, ctypes.byref(rep))))
    refused("null argument", lambda: ctx._check(fn(ctx._h, ctypes.byref(desc), (PtauContributionC * 1)(), None, 1, zb, ctypes.byref(rep))))
    refused("null ptau pointer", lambda: ctx._check(fn(ctx._h, ctypes.byref(PtauDesc(3)), None, None, 0, zb, ctypes.byref(rep))))
    assert ctx.ptau_verify(p0, None, None, z).relation == [1] * 7 + [-1] * 3     # and the legal call
