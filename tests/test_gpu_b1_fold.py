"""pointsB1 folded into pointsA1 on the GPU: MSM(w, B1) = MSM(w, A1) + MSM(w, B1 - A1), and a key keeps the differences
(or nothing) in place of pointsB1 where few enough of them are live (b1_fold_form, nim_groth16_amd/csrc/key_plan.hpp;
tests/test_b1_fold_cpu.py holds the rule and the point difference on the CPU).

Every proof here is compared with the C oracle's bit for bit, the key's form and its two counts with a recount of the
key's bytes on the host, and every key is proved once more in a child process under G16_B1_FOLD=0, which must give the
same bytes.

Which form a circuit gets.  The fake setup, like snarkjs, adds one dummy row to the A matrix per public wire (wires
0 .. npubs: fake_setup.nim:59-63), so pointsA1 and pointsB1 differ on those wires in EVERY key.  A circuit made of
symmetric products only -- the squaring chain, mixedCircuit(lin_pct=0) -- therefore has npubs + 1 = 2 live differences,
not none: its form is DELTA with two live points, and EMPTY is reached only by a key whose two arrays are equal
throughout, which is built here by copying pointsA1 over pointsB1 (the C oracle is given the same arrays; such a key does
not satisfy the pairing equation, so only the proof bytes are compared for it)."""
import copy
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("squaring", "mixed_lin5", "poseidon", "hand", "equal_arrays")
WANT_FORM = {"squaring": "DELTA", "mixed_lin5": "DELTA", "poseidon": "PLAIN", "hand": "DELTA", "equal_arrays": "EMPTY"}


def hand_built():
    """A few rows by hand, then boolean rows so that B1 has enough live points for the differences to be the sparser set.
      wires: 0 = one, 1 = out (public), 2 = x, 3 = y, 4 = z, 5 = u, 6.. = bits
      x * (-x) = -y      x's column of B is minus its column of A: B1_x = -A1_x, the doubling branch of the difference
      y * y    = z       symmetric
      z * 1    = out - u z in A only (B1_z at infinity), wire 0 in B here and in A's dummy row (a general difference),
                         u in neither A nor B (both points at infinity)
      b * b    = b       symmetric, 60 of them"""
    from nim_groth16_amd.bn128 import primeR as R
    from nim_groth16_amd.fake_setup import R1CS
    nbits = 60
    cons = [([(2, 1)], [(2, R - 1)], [(3, R - 1)]),
            ([(3, 1)], [(3, 1)], [(4, 1)]),
            ([(4, 1)], [(0, 1)], [(1, 1), (5, R - 1)])]
    bits = [i % 3 == 0 for i in range(nbits)]
    for i in range(nbits):
        cons.append(([(6 + i, 1)], [(6 + i, 1)], [(6 + i, 1)]))
    x, u = 7, 5
    wit = [1, x ** 4 + u, x, x * x, x ** 4, u] + [int(b) for b in bits]
    return R1CS(nWires=6 + nbits, nPubOut=1, nPubIn=0, nPrivIn=2 + nbits, constraints=cons), wit


def circuit(name):
    from nim_groth16_amd.synthetic import mixedCircuit, poseidonMerkle, squaringChain
    if name in ("squaring", "equal_arrays"):
        return squaringChain((1 << 8) - 2, seed=4)
    if name == "mixed_lin5":
        return mixedCircuit((1 << 10) - 2, seed=4, lin_pct=5)
    if name == "poseidon":
        return poseidonMerkle(10, seed=4)
    return hand_built()


def make_key(name, ctx):
    """-> (zkey, witness as ints, witness as Montgomery bytes, mask r, mask s)"""
    from nim_groth16_amd import bn128 as F
    from nim_groth16_amd.fake_setup import ToxicWaste, fakeCircuitSetup
    from nim_groth16_amd.synthetic import SplitMix64
    r1cs, wit = circuit(name)
    rng = SplitMix64(5 + CASES.index(name))
    zk = fakeCircuitSetup(r1cs, ToxicWaste(*[rng.fr() for _ in range(5)]), 1, ctx)
    if name == "equal_arrays":
        zk = copy.copy(zk)
        zk.pPoints = copy.copy(zk.pPoints)
        zk.pPoints.pointsB1 = zk.pPoints.pointsA1
    return zk, wit, F.frSeqToMontBytes(wit), rng.fr(), rng.fr()


def prove_all(ctx):
    """every case's proof and form through g16_prove: what the child process under G16_B1_FOLD=0 prints"""
    from nim_groth16_amd import loadProvingKey
    from nim_groth16_amd import bn128 as F
    out = {}
    for name in CASES:
        zk, _wit, wb, r, s = make_key(name, ctx)
        pk = loadProvingKey(zk, ctx)
        try:
            proof = pk.prove(wb, r=F.frToMontBytes(r), s=F.frToMontBytes(s))
            out[name] = {"proof": b"".join(proof).hex(), "fold": pk.b1_fold(), "inf": pk.inf_counts()}
        finally:
            pk.destroy()
    return out


def recount(zk):
    """the two counts of the rule from the key's bytes: 64-byte comparisons, as the key-creation kernel makes them"""
    a1, b1 = zk.pPoints.pointsA1, zk.pPoints.pointsB1
    n = len(a1) // 64
    live_b1 = sum(b1[64 * i:64 * i + 64] != bytes(64) for i in range(n))
    live_delta = sum(a1[64 * i:64 * i + 64] != b1[64 * i:64 * i + 64] for i in range(n))
    return live_b1, live_delta


def rule(live_b1, live_delta, n, pct=10):
    """b1_fold_form restated (tests/test_b1_fold_cpu.py holds it against the C++): the issue's threshold, and against a
    B1 that runs compacted the differences must leave most waves of 64 entries empty"""
    if live_delta == 0:
        return "EMPTY"
    if live_delta * 100 > live_b1 * (100 - pct):
        return "PLAIN"
    compacted = n > live_b1 and (n - live_b1) * 100 >= pct * n
    return "PLAIN" if compacted and live_delta * 64 > live_b1 else "DELTA"


@pytest.fixture(scope="module")
def keys(ctx):
    """name -> (zkey, witness ints, witness bytes, r, s): every setup once"""
    return {name: make_key(name, ctx) for name in CASES}


@pytest.fixture(scope="module")
def folded(ctx):
    assert "G16_B1_FOLD" not in os.environ and "G16_INF_COMPACT" not in os.environ
    return prove_all(ctx)


@pytest.fixture(scope="module")
def unfolded():
    """the same proofs from a process of its own under G16_B1_FOLD=0 (the knobs are read once per process)"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("G16_")}
    env["G16_B1_FOLD"] = "0"
    script = ("import json, sys; sys.path.insert(0, %r)\n"
              "from nim_groth16_amd import Context\n"
              "from tests.test_gpu_b1_fold import prove_all\n"
              "print('PROOFS ' + json.dumps(prove_all(Context(0))))\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("PROOFS ")]
    assert len(line) == 1, r.stdout[-2000:]
    return json.loads(line[0][len("PROOFS "):])


@pytest.mark.parametrize("name", CASES)
def test_proof_equals_the_oracles_and_the_key_has_its_form(ctx, orc, keys, folded, unfolded, name):
    from oracle import bn254_ref as o
    from tests.parity import check_gpu_proof, oracle_proof
    zk, wit, wb, r, s = keys[name]
    got = bytes.fromhex(folded[name]["proof"])
    proof = (got[0:64], got[64:192], got[192:256])
    if name == "equal_arrays":                      # not a key of any circuit: the five MSMs and the mask algebra only
        ref, _oz, _ = oracle_proof(orc, zk, wit, wb, r, s)
        assert (o.g1_from_bytes(proof[0]), o.g2_from_bytes(proof[1]), o.g1_from_bytes(proof[2])) == \
            (ref.pi_a, ref.pi_b, ref.pi_c)
    else:
        check_gpu_proof(orc, zk, wit, wb, r, s, proof, ctx)
    live_b1, live_delta = recount(zk)
    print(name, "live_b1", live_b1, "live_delta", live_delta, folded[name]["fold"])
    assert folded[name]["fold"] == {"form": WANT_FORM[name], "live_b1": live_b1, "live_delta": live_delta}
    assert rule(live_b1, live_delta, len(zk.pPoints.pointsA1) // 64) == WANT_FORM[name]
    if name in ("squaring", "equal_arrays"):
        assert live_delta == (zk.header.npubs + 1 if name == "squaring" else 0)   # the public wires' dummy rows alone
    # G16_B1_FOLD=0: pointsB1 as it is, the same proof, and the same report of the key's points at infinity
    assert unfolded[name]["fold"]["form"] == "PLAIN"
    assert unfolded[name]["proof"] == folded[name]["proof"]
    assert unfolded[name]["inf"] == folded[name]["inf"]


def test_hand_built_key_takes_every_branch_of_the_difference(keys):
    """what the hand-built rows were built for, recounted from the key: a wire with B1 = -A1, one with B1 at infinity
    and A1 not, one with both at infinity, one general pair, and equal pairs"""
    from oracle import bn254_ref as o
    zk = keys["hand"][0]
    a1 = [o.g1_from_bytes(zk.pPoints.pointsA1[i:i + 64]) for i in range(0, len(zk.pPoints.pointsA1), 64)]
    b1 = [o.g1_from_bytes(zk.pPoints.pointsB1[i:i + 64]) for i in range(0, len(zk.pPoints.pointsB1), 64)]
    G = o.G1
    assert b1[2] == G.neg(a1[2]) and not G.is_inf(a1[2])                      # x
    assert G.is_inf(b1[4]) and not G.is_inf(a1[4])                            # z
    assert G.is_inf(b1[5]) and G.is_inf(a1[5])                                # u
    assert not G.is_inf(b1[0]) and not G.is_inf(a1[0]) and b1[0] != a1[0] and b1[0] != G.neg(a1[0])   # one
    assert b1[3] == a1[3] and all(b1[i] == a1[i] and not G.is_inf(a1[i]) for i in range(6, len(a1)))


@pytest.mark.parametrize("name", ["equal_arrays", "mixed_lin5", "squaring"])
def test_two_shards_on_one_device_equal_the_unsharded_proof(ctx, keys, folded, name):
    """An EMPTY key, a DELTA key whose live differences are spread over both halves, and one -- the squaring chain --
    whose only live differences are wires 0 and 1: by its own range the second shard of that key would find none and
    take EMPTY where the first takes DELTA, so there the form itself, and not only the counts, pins the whole-range
    decision."""
    from nim_groth16_amd import loadProvingKey
    from nim_groth16_amd import bn128 as F
    zk, _wit, wb, r, s = keys[name]
    rb, sb = F.frToMontBytes(r), F.frToMontBytes(s)
    want = bytes.fromhex(folded[name]["proof"])
    shards = [loadProvingKey(zk, ctx, shard_index=k, shard_count=2) for k in range(2)]
    try:
        if name == "squaring":
            live_b1, live_delta = recount(zk)
            half = len(zk.pPoints.pointsA1) // 128
            a1, b1 = zk.pPoints.pointsA1, zk.pPoints.pointsB1
            assert live_delta > 0 and a1[64 * half:] == b1[64 * half:]     # no live difference in the second half
        # decided over the whole wire range: both shards report the unsharded key's form and counts
        assert [k.b1_fold() for k in shards] == [folded[name]["fold"]] * 2
        recs = b"".join(k.prove_partials(wb) for k in shards)
        for k in shards:
            assert b"".join(k.prove_combine(recs, 2, rb, sb)) == want
    finally:
        for k in shards:
            k.destroy()


def test_pool_and_group_prove_the_same_bytes(ctx, keys, folded):
    from nim_groth16_amd import DeviceGroup, ProverPool, loadGroupKey, loadProvingKey
    from nim_groth16_amd import bn128 as F
    zk, _wit, wb, r, s = keys["equal_arrays"]
    rb, sb = F.frToMontBytes(r), F.frToMontBytes(s)
    want = bytes.fromhex(folded["equal_arrays"]["proof"])
    pk = loadProvingKey(zk, ctx)
    pool = ProverPool(pk, depth=2)
    try:
        assert b"".join(pool.collect(pool.submit(wb, r=rb, s=sb))) == want
    finally:
        pool.close()
        pk.destroy()
    grp = DeviceGroup([0, 0])
    gk = loadGroupKey(zk, grp)
    try:
        assert b"".join(gk.prove(wb, r=rb, s=sb)) == want
    finally:
        gk.destroy()
        grp.close()
