"""Phase-2 contribution on the GPU: g16_points_scale_g1/g2, g16_key_contribute, g16_contributions_verify.  Everything is
byte-exact.  Points are known multiples of the generators (the C oracle's fixed-base multiplier over integer logarithms,
itself held to the Python oracle), so k * P is fixed_base(k * log mod r); a handful of points go through oracle.G1.mul /
G2.mul directly.  The chain's expected reports come from the log-space model of tests/phase2_pictures.py."""
import ctypes

import pytest

from oracle import bn254_ref as o
from tests import circuit_audit_pictures as CA
from tests import inputs as I
from tests import key_audit_pictures as KA
from tests import phase2_pictures as PP

pytestmark = pytest.mark.gpu
R = o.R
PSZ = {1: 64, 2: 128}
TILE = 256                  # SCALE_BLOCK * SCALE_GROUP: the points of one workgroup; one inversion group = 4 points 64 apart
GROUP_STRIDE, GROUP = 64, 4


def _scale(ctx, orc, group, logs, k, mont=True):
    """k * fixed_base(logs) must be fixed_base(k * logs); a zero logarithm is the point (0,0)"""
    pts = orc.fixed_base(group, I.fr_mont_bytes(logs)) if logs else b""
    kb = I.fr_mont_bytes([k]) if mont else I.fr_std_bytes([k])
    got = ctx.points_scale(group, pts, kb, mont=mont)
    exp = orc.fixed_base(group, I.fr_mont_bytes([k * x % R for x in logs])) if logs else b""
    if got != exp:
        p = PSZ[group]
        i = next(i for i in range(len(logs)) if got[p * i:p * (i + 1)] != exp[p * i:p * (i + 1)])
        raise AssertionError(f"G{group}, n = {len(logs)}, k = {k:#x}: output {i} differs (the first of them)")
    return pts, got


def _logs(n, seed, zeros=()):
    rng = o.SplitMix64(seed)
    logs = [rng.fr() or 1 for _ in range(n)]
    for i in zeros:
        logs[i] = 0
    return logs


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 513])
def test_scale_g1_sizes(ctx, orc, n):
    """one lane of one workgroup up to three workgroups; one below, at and one above a lane's four points and a
    workgroup's 256"""
    k = o.SplitMix64(900 + n).fr()
    for mont in (True, False):
        _scale(ctx, orc, 1, _logs(n, n), k, mont)


@pytest.mark.parametrize("mont", [True, False])
def test_scale_g1_edge_scalars(ctx, orc, mont):
    logs = _logs(70, 5, zeros=(0, 69))
    for k in PP.edge_scalars():
        _scale(ctx, orc, 1, logs, k, mont)


def test_scale_g1_against_the_python_oracle(ctx, orc):
    logs = _logs(5, 17, zeros=(2,))
    k = o.SplitMix64(18).fr()
    pts, got = _scale(ctx, orc, 1, logs, k)
    for i in range(5):
        p = o.g1_from_bytes(pts[64 * i:64 * i + 64])
        assert o.g1_from_bytes(got[64 * i:64 * i + 64]) == o.G1.mul(k, p)


def test_scale_g1_infinity_in_a_group(ctx, orc):
    """(0,0) first, last, at every position of one inversion group (lane 5 of the second workgroup: points 256 + 5 + 64 j),
    in every pair of them, filling the whole group, and filling a whole workgroup"""
    n = 2 * TILE + 37
    k = o.SplitMix64(44).fr()
    members = [TILE + 5 + GROUP_STRIDE * j for j in range(GROUP)]
    cases = [(0,), (n - 1,), tuple(members), tuple(range(TILE, 2 * TILE)), tuple(range(n))]
    cases += [(m,) for m in members]
    cases += [(a, b) for a in members for b in members if a < b]
    cases += [tuple(m for m in members if m != keep) for keep in members]
    for zeros in cases:
        _scale(ctx, orc, 1, _logs(n, 61, zeros), k)
    # the tail: a group whose last members lie beyond n
    for n2 in (TILE + 5 + 1, TILE + 5 + GROUP_STRIDE + 1):
        _scale(ctx, orc, 1, _logs(n2, 62, (TILE + 5,)), k)


@pytest.mark.parametrize("n", [0, 1, 4, 5, 65, 257])
def test_scale_g2(ctx, orc, n):
    k = o.SplitMix64(700 + n).fr()
    zeros = () if n < 4 else (0, n - 1, 2)
    _scale(ctx, orc, 2, _logs(n, 3 * n, zeros), k, mont=bool(n & 1))


def test_scale_g2_edge_scalars_and_the_python_oracle(ctx, orc):
    logs = _logs(6, 8, zeros=(1,))
    for j, k in enumerate(PP.edge_scalars()):
        _scale(ctx, orc, 2, logs, k, mont=bool(j & 1))
    k = o.SplitMix64(19).fr()
    pts, got = _scale(ctx, orc, 2, logs[:2], k)
    for i in range(2):
        assert o.g2_from_bytes(got[128 * i:128 * i + 128]) == o.G2.mul(k, o.g2_from_bytes(pts[128 * i:128 * i + 128]))
    _scale(ctx, orc, 2, [0] * 5, k)


def test_scale_arguments(ctx, orc):
    from nim_groth16_amd import G16Error
    from nim_groth16_amd._lib import G16_EINVAL
    pts = orc.fixed_base(1, I.fr_mont_bytes([5, 6]))
    with pytest.raises(G16Error, match="not canonical") as e:
        ctx.points_scale(1, pts, R.to_bytes(32, "little"))
    assert e.value.code == G16_EINVAL
    out = ctypes.create_string_buffer(128)
    for args, match in (((None, 2, bytes(32), 1, out), "null pointer"), ((pts, 2, None, 1, out), "null pointer"),
                        ((pts, 2, bytes(32), 1, None), "null pointer"), ((pts, 2, bytes(32), 7, out), "flags"),
                        ((pts, 1 << 31, bytes(32), 1, out), "out of range")):
        with pytest.raises(G16Error, match=match) as e:
            ctx._check(ctx._lib.g16_points_scale_g1(ctx._h, *args))
        assert e.value.code == G16_EINVAL
    assert ctx.points_scale(1, pts, bytes(32)) == bytes(128)              # k = 0: all infinity


# ---- g16_key_contribute ----------------------------------------------------------------------------------------------------
def _fixed(ctx):
    import functools

    @functools.lru_cache(None)
    def fixed(group, logs):
        return ctx.fixed_base(group, I.fr_mont_bytes(list(logs))) if logs else b""
    return fixed


def _part(zk):
    from nim_groth16_amd.setup import _phase2Part
    return _phase2Part(zk)


@pytest.mark.parametrize("name", ["toy", "chain"])
def test_contribute_equals_setup_with_delta(ctx, orc, name):
    """circuitSetup(delta = None) then contributions d1, d2 == circuitSetup(delta = d1), (delta = d1 d2), byte for byte,
    both flavours; the record equals its integer model"""
    from nim_groth16_amd.setup import circuitSetup
    from tests.test_gpu_circuit_setup import _circuit, _ptau, _r1cs
    rng = o.SplitMix64(77 + len(name))
    d1, d2, s, c = (rng.fr() or 1 for _ in range(4))
    ch = orc.fixed_base(2, I.fr_mont_bytes([c]))
    for flavour in (CA.SNARKJS, CA.JENSGROTH):
        mk = lambda delta: _part(circuitSetup(_r1cs(_circuit(name)), _ptau(ctx, name), flavour, delta, ctx))   # noqa: E731
        k0 = mk(None)
        k1, rec1 = ctx.key_contribute(k0, I.fr_mont_bytes([d1]), I.fr_mont_bytes([s]), ch)
        assert k1 == mk(d1), (name, flavour)
        assert rec1 == k1["delta1"] + orc.fixed_base(1, I.fr_mont_bytes([s, d1 * s % R])) + \
            orc.fixed_base(2, I.fr_mont_bytes([d1 * c % R]))
        k2, rec2 = ctx.key_contribute(k1, I.fr_std_bytes([d2]), I.fr_std_bytes([s]), ch, mont=False)
        assert k2 == mk(d1 * d2 % R), (name, flavour)
        assert rec2[:64] == k2["delta1"] and rec2[64:128] == rec1[64:128]


def test_closed_loop(ctx):
    """setup -> contribute -> the circuit audit passes -> prove -> the contributed verification key accepts, the
    uncontributed one does not; the chain of two contributions verifies"""
    from nim_groth16_amd import Mask, Witness, extractVKey, generateProofWithMask, loadProvingKey, verifyProof
    from nim_groth16_amd.files.zkey import auditCircuit
    from nim_groth16_amd.setup import contribute, verifyContributions
    from tests.test_gpu_circuit_setup import _toy
    r1cs, pt, zk0 = _toy(ctx)
    zk1 = contribute(zk0, 12345, 678, "first", ctx)
    zk2 = contribute(zk1, name="second", ctx=ctx)
    assert zk0.contributions is None and len(zk2.contributions.records) == 2 and zk2.contributions.names == ["first", "second"]
    rep = auditCircuit(zk2, r1cs, pt, ctx)
    assert rep.failed == 0, str(rep)
    chain = verifyContributions(zk0, zk2, ctx=ctx)
    assert chain.ok and chain.relation == [1] * 7 and chain.transcript == 1, str(chain)
    assert str(chain) == "contribution chain: ok"
    pk = loadProvingKey(zk2, ctx)
    try:
        pr = generateProofWithMask(0, False, zk2, Witness("bn128", 8, I.fr_mont_bytes(o.TOY_WITNESS)), Mask(21, 22), ctx, pkey=pk)
    finally:
        pk.destroy()
    assert verifyProof(extractVKey(zk2), pr, ctx)
    assert not verifyProof(extractVKey(zk0), pr, ctx)
    # a record from another transcript: the stored hash no longer follows from its predecessors
    import copy
    bad = copy.deepcopy(zk2)
    bad.contributions.transcripts[0] = bytes(64)
    rep = verifyContributions(zk0, bad, ctx=ctx)
    assert not rep.ok and rep.transcript == 0 and "transcript" in str(rep)


# ---- g16_contributions_verify ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PP.pictures()))
def test_chain_pictures(ctx, name):
    pic = PP.pictures()[name]
    ini, fin, recs, chs = PP.encode(pic, _fixed_of(ctx))
    rep = ctx.contributions_verify(ini, fin, recs, chs, pic.zc, pic.zh)
    assert rep.as_dict() == {**pic.report, "transcript": None}, (name, str(rep))
    assert rep.ok == (pic.report["failed"] == 0)


_fixed_cache = {}


def _fixed_of(ctx):
    if "f" not in _fixed_cache:
        _fixed_cache["f"] = _fixed(ctx)
    return _fixed_cache["f"]


def _proof_bytes(ctx, zk, pk):
    from nim_groth16_amd import Mask, Witness, generateProofWithMask
    pr = generateProofWithMask(0, False, zk, Witness("bn128", 8, I.fr_mont_bytes(o.TOY_WITNESS)), Mask(11, 12), ctx, pkey=pk)
    return pr.pi_a, pr.pi_b, pr.pi_c


def test_refusals_leave_the_context_as_it_was(ctx, orc):
    from nim_groth16_amd import G16Error, loadProvingKey
    from nim_groth16_amd._lib import G16_EINVAL, ChainReportC, ContributionC, Phase2Key, Phase2Out
    from tests.test_gpu_circuit_setup import _fake, _waste
    zk = _fake(ctx, "toy", CA.SNARKJS, _waste("toy").delta)
    pk = loadProvingKey(zk, ctx)
    try:
        before = _proof_bytes(ctx, zk, pk)
        key = _part(zk)
        one, ch = I.fr_mont_bytes([1]), orc.fixed_base(2, I.fr_mont_bytes([9]))

        def refused(match, fn):
            with pytest.raises(G16Error, match=match) as e:
                fn()
            assert e.value.code == G16_EINVAL, match
        refused("d must be non-zero", lambda: ctx.key_contribute(key, bytes(32), one, ch))
        refused("d must be non-zero and canonical", lambda: ctx.key_contribute(key, R.to_bytes(32, "little"), one, ch, mont=False))
        refused("s must be non-zero", lambda: ctx.key_contribute(key, one, bytes(32), ch))
        refused("challenge is the point at infinity", lambda: ctx.key_contribute(key, one, one, bytes(128)))
        refused("delta1 is the point at infinity", lambda: ctx.key_contribute({**key, "delta1": bytes(64)}, one, one, ch))
        small = o.g2_to_bytes(KA.twist_outsiders()["small"])
        refused(r"challenge\[0\] is not in the order-r subgroup", lambda: ctx.key_contribute(key, one, one, small))
        h1 = bytearray(key["pointsH1"])
        h1[64 * 3:64 * 4] = KA.off_curve(1)
        refused(r"pointsH1\[3\] is not on the curve", lambda: ctx.key_contribute({**key, "pointsH1": bytes(h1)}, one, one, ch))
        c1 = KA.raise_by_p(1, key["pointsC1"][:64], 0) + key["pointsC1"][64:]
        refused(r"pointsC1\[0\] is not a canonical encoding", lambda: ctx.key_contribute({**key, "pointsC1": c1}, one, one, ch))
        pkd, keep = ctx._phase2_key(key)
        refused("null argument", lambda: ctx._check(ctx._lib.g16_key_contribute(ctx._h, ctypes.byref(pkd), one, one, 1, ch, None)))
        refused("null argument", lambda: ctx._check(ctx._lib.g16_key_contribute(ctx._h, None, one, one, 1, ch,
                                                                                 ctypes.byref(Phase2Out()))))
        refused("null output pointer", lambda: ctx._check(ctx._lib.g16_key_contribute(ctx._h, ctypes.byref(pkd), one, one, 1, ch,
                                                                                       ctypes.byref(Phase2Out()))))
        # the chain
        nc1, nh1 = len(key["pointsC1"]) // 64, len(key["pointsH1"]) // 64
        zc, zh = [3] * nc1, [5] * nh1
        refused("c1: multiplier 2 is zero", lambda: ctx.contributions_verify(key, key, [], [], [3, 3, 0] + [3] * (nc1 - 3), zh))
        refused("h1: multiplier 0 is zero", lambda: ctx.contributions_verify(key, key, [], [], zc, [0] + [5] * (nh1 - 1)))
        short = {**key, "pointsH1": key["pointsH1"][:-64]}
        refused("other point counts", lambda: ctx.contributions_verify(key, short, [], [], zc, zh[:-1]))
        rep = ChainReportC()
        refused("null argument", lambda: ctx._check(ctx._lib.g16_contributions_verify(
            ctx._h, ctypes.byref(pkd), ctypes.byref(pkd), None, None, 1, bytes(16 * nc1), bytes(16 * nh1), ctypes.byref(rep))))
        refused("null argument", lambda: ctx._check(ctx._lib.g16_contributions_verify(
            ctx._h, ctypes.byref(pkd), None, (ContributionC * 1)(), None, 0, None, None, ctypes.byref(rep))))
        assert ctx.contributions_verify(key, key, [], [], zc, zh).ok           # a chain of no records
        del keep, Phase2Key
        assert _proof_bytes(ctx, zk, pk) == before
    finally:
        pk.destroy()


# ---- tools/prove_files.py ----------------------------------------------------------------------------------------------------
def test_prove_files_contributes_and_verifies_the_chain(ctx, tmp_path):
    """--contribute twice, then --verify-contributions through subprocesses: exit 0 and a proof; a key with two points of
    pointsH1 swapped, and a log with a record of another key: exit 2 and no proof"""
    import os
    import subprocess
    import sys

    from nim_groth16_amd.files import parseContributions, parseZKey, writeWitness, writeZKey
    from tests.test_gpu_circuit_setup import _toy
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tool = os.path.join(root, "tools", "prove_files.py")
    zk0 = _toy(ctx)[2]
    init, c1, c2, wpath = (str(tmp_path / n) for n in ("init.zkey", "c1.zkey", "c2.zkey", "toy.wtns"))
    writeZKey(init, zk0)
    writeWitness(wpath, o.TOY_WITNESS)

    def run(*args):
        return subprocess.run([sys.executable, tool, *args], capture_output=True, text=True, timeout=600)
    out = run("-z", init, "--contribute", "--contribute-name", "alice", "--contribute-out", c1)
    assert out.returncode == 0 and "contribution 1 (alice): wrote" in out.stdout, out.stderr
    assert open(init, "rb").read() != open(c1, "rb").read() and parseContributions(init) is None
    # the second one in place, checked against the initial key and proved from in the same run
    open(c2, "wb").write(open(c1, "rb").read())
    proof = str(tmp_path / "proof.json")
    out = run("-z", c2, "--contribute", "--verify-contributions", init, "-w", wpath, "-o", proof, "-i",
              str(tmp_path / "public.json"), "-y")
    assert out.returncode == 0 and "contribution chain: ok" in out.stdout and "verification succeeded" in out.stdout, \
        out.stdout + out.stderr
    log = parseContributions(c2)
    assert log.names == ["alice", ""] and len(log.records) == 2 and os.path.exists(proof)
    zk2 = parseZKey(c2)
    assert zk2.specPoints.delta1 == log.records[1][:64] != zk0.specPoints.delta1
    assert zk2.pPoints.pointsA1 == zk0.pPoints.pointsA1 and zk2.pPoints.pointsH1 != zk0.pPoints.pointsH1
    # tampered: two points of pointsH1 swapped (each still on the curve)
    zk2.contributions = log
    h1 = zk2.pPoints.pointsH1
    zk2.pPoints.pointsH1 = h1[64:128] + h1[:64] + h1[128:]
    bad, proof2 = str(tmp_path / "bad.zkey"), str(tmp_path / "proof2.json")
    writeZKey(bad, zk2)
    out = run("-z", bad, "--verify-contributions", init, "-w", wpath, "-o", proof2, "-i", str(tmp_path / "p2.json"))
    assert out.returncode == 2 and "contribution chain: FAILED" in out.stdout and "pointsH1" in out.stdout, out.stdout + out.stderr
    assert not os.path.exists(proof2)
    # the first key's chain does not lead to the second key
    out = run("-z", c2, "--verify-contributions", c1)
    assert out.returncode == 2 and "transcript" in out.stdout, out.stdout + out.stderr
