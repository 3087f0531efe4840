"""The sparse run of the B1 differences on the GPU: a DELTA key (pointsB1 folded into pointsA1, tests/test_gpu_b1_fold.py)
with at most B1_SPARSE_MAX = 64 live differences keeps the list of its live wires, and its B1 job forms the bucket sums
from those wires' witness values alone (msm_sparse_accum, nim_groth16_amd/csrc/msm.cuh) instead of gathering a table
entry per entry of the whole witness arrangement.  tests/test_b1_sparse_cpu.py holds the rule and the hit list on the CPU.

Every proof here is compared with the C oracle's bit for bit, and every key is proved once more in a child process under
G16_B1_FOLD=0 (pointsB1 as it is, today's launches), which must give the same bytes.  All keys have < 2^10 constraints.

The hand-built circuits use one kind of row to place a live difference on any wire with any witness value:
    T(e):  e * one = e      wire e in A only, so B1_e = (0,0) != A1_e, and the row holds whatever e is."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPARSE_MAX = 64
CASES = ("squaring", "branches", "at_max", "above_max")
WANT_SPARSE = {"squaring": True, "branches": True, "at_max": True, "above_max": False}


def t_row(e):
    return ([(e, 1)], [(0, 1)], [(e, 1)])


def bool_row(b):
    return ([(b, 1)], [(b, 1)], [(b, 1)])


def branches():
    """Live differences that take every branch of a bucket's sum; N = 256 wires, shards of two split at wire 128.
      wires 0 = one, 1 = out (public; live by the dummy rows of the public wires, as in every key)
      2, 3     T rows, equal scalars: the same bucket in every window, two different points (the general addition)
      4, 5     ONE row (w4 + w5) * one = w4 + w5: D_4 = D_5, equal scalars -- the doubling branch of the mixed addition
      6, 7     w6 * w7 = w8: wire 6 in A only, wire 7 in B only, same row: D_7 = -D_6, equal scalars -- the sum is infinity
      8        in C only: both points at infinity, not live
      9        T row, scalar 0: a live wire without a hit
      10       T row, scalar r - 1
      127, 128 T rows: the last wire of shard 0 and the first of shard 1
      the rest boolean rows b * b = b: symmetric, they give pointsB1 its live points"""
    from nim_groth16_amd.bn128 import primeR as R
    from nim_groth16_amd.fake_setup import R1CS
    from nim_groth16_amd.synthetic import SplitMix64
    N = 256
    rng = SplitMix64(77)
    s_eq, s_dbl, s_neg, s_lo, s_hi = (rng.fr() for _ in range(5))
    wit = [None] * N
    wit[0], wit[1] = 1, rng.fr()
    cons = [t_row(2), t_row(3), ([(4, 1), (5, 1)], [(0, 1)], [(4, 1), (5, 1)]), ([(6, 1)], [(7, 1)], [(8, 1)]),
            t_row(9), t_row(10), t_row(127), t_row(128)]
    wit[2] = wit[3] = s_eq
    wit[4] = wit[5] = s_dbl
    wit[6] = wit[7] = s_neg
    wit[8] = s_neg * s_neg % R
    wit[9], wit[10] = 0, R - 1
    wit[127], wit[128] = s_lo, s_hi
    for b in range(N):
        if wit[b] is None:
            wit[b] = b % 3 == 0 and 1 or 0
            cons.append(bool_row(b))
    live = [0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 127, 128]
    return R1CS(nWires=N, nPubOut=1, nPubIn=0, nPrivIn=N - 2, constraints=cons), wit, live


def t_wires(nlive):
    """nlive live differences exactly: the public wires 0 and 1, and nlive - 2 T rows with scalars of their own; 1000
    wires, the rest boolean rows -- so that under 10 % of pointsB1 is at infinity (B1 as it stands would not run
    compacted) and the rule still says DELTA"""
    from nim_groth16_amd.fake_setup import R1CS
    from nim_groth16_amd.synthetic import SplitMix64
    N = 1000
    rng = SplitMix64(1000 + nlive)
    wit = [1, rng.fr()] + [0] * (N - 2)
    cons, live = [], [0, 1]
    for k in range(nlive - 2):
        e = 2 + 15 * k                      # spread over both halves of the wire range
        wit[e] = rng.fr()
        cons.append(t_row(e))
        live.append(e)
    for b in range(2, N):
        if b not in live:
            wit[b] = b % 2
            cons.append(bool_row(b))
    return R1CS(nWires=N, nPubOut=1, nPubIn=0, nPrivIn=N - 2, constraints=cons), wit, live


def circuit(name):
    """-> (r1cs, witness, the live wires it was built to have or None)"""
    from nim_groth16_amd.synthetic import squaringChain
    if name == "squaring":
        return squaringChain((1 << 8) - 2, seed=4) + ([0, 1],)
    if name == "branches":
        return branches()
    return t_wires(SPARSE_MAX if name == "at_max" else SPARSE_MAX + 1)


def make_key(name, ctx):
    """-> (zkey, witness as ints, witness as Montgomery bytes, mask r, mask s, live wires)"""
    from nim_groth16_amd import bn128 as F
    from nim_groth16_amd.fake_setup import ToxicWaste, fakeCircuitSetup
    from nim_groth16_amd.synthetic import SplitMix64
    r1cs, wit, live = circuit(name)
    rng = SplitMix64(50 + CASES.index(name))
    zk = fakeCircuitSetup(r1cs, ToxicWaste(*[rng.fr() for _ in range(5)]), 1, ctx)
    return zk, wit, F.frSeqToMontBytes(wit), rng.fr(), rng.fr(), live


def prove_all(ctx):
    """every case's proof through g16_prove, with what the key says of itself: what the child process under
    G16_B1_FOLD=0 prints"""
    from nim_groth16_amd import loadProvingKey
    from nim_groth16_amd import bn128 as F
    out = {}
    for name in CASES:
        zk, _wit, wb, r, s, _live = make_key(name, ctx)
        pk = loadProvingKey(zk, ctx)
        try:
            proof = pk.prove(wb, r=F.frToMontBytes(r), s=F.frToMontBytes(s))
            out[name] = {"proof": b"".join(proof).hex(), "fold": pk.b1_fold(), "sparse": pk.b1_sparse()}
        finally:
            pk.destroy()
    return out


@pytest.fixture(scope="module")
def keys(ctx):
    return {name: make_key(name, ctx) for name in CASES}


@pytest.fixture(scope="module")
def proved(ctx):
    assert "G16_B1_FOLD" not in os.environ and "G16_INF_COMPACT" not in os.environ
    return prove_all(ctx)


@pytest.fixture(scope="module")
def unfolded():
    """the same proofs from a process of its own under G16_B1_FOLD=0 (the knobs are read once per process)"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("G16_")}
    env["G16_B1_FOLD"] = "0"
    script = ("import json, sys; sys.path.insert(0, %r)\n"
              "from nim_groth16_amd import Context\n"
              "from tests.test_gpu_b1_sparse import prove_all\n"
              "print('PROOFS ' + json.dumps(prove_all(Context(0))))\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("PROOFS ")]
    assert len(line) == 1, r.stdout[-2000:]
    return json.loads(line[0][len("PROOFS "):])


@pytest.mark.parametrize("name", CASES)
def test_proof_equals_the_oracles_and_the_key_runs_as_the_rule_says(ctx, orc, keys, proved, unfolded, name):
    from tests.parity import check_gpu_proof
    from tests.test_gpu_b1_fold import recount, rule
    zk, wit, wb, r, s, live = keys[name]
    got = bytes.fromhex(proved[name]["proof"])
    check_gpu_proof(orc, zk, wit, wb, r, s, (got[0:64], got[64:192], got[192:256]), ctx)
    # the key is DELTA by the existing rule, recounted from its bytes, and holds exactly the live wires it was built for
    live_b1, live_delta = recount(zk)
    a1, b1 = zk.pPoints.pointsA1, zk.pPoints.pointsB1
    assert [i for i in range(len(a1) // 64) if a1[64 * i:64 * i + 64] != b1[64 * i:64 * i + 64]] == live
    assert rule(live_b1, live_delta, len(a1) // 64) == "DELTA"
    assert proved[name]["fold"] == {"form": "DELTA", "live_b1": live_b1, "live_delta": live_delta}
    # ... and takes the sparse run up to SPARSE_MAX live differences, today's path above
    want = WANT_SPARSE[name]
    assert want == (live_delta <= SPARSE_MAX)
    print(name, "live_delta", live_delta, proved[name]["sparse"])
    assert proved[name]["sparse"] == {"sparse": want, "live": live_delta if want else 0, "max": SPARSE_MAX}
    # G16_B1_FOLD=0: pointsB1 as it is, no sparse run, the same proof
    assert unfolded[name]["fold"]["form"] == "PLAIN" and unfolded[name]["sparse"]["sparse"] is False
    assert unfolded[name]["proof"] == proved[name]["proof"]


def test_the_branch_circuit_holds_the_points_it_was_built_for(keys):
    """recounted from the key: D_4 = D_5, D_7 = -D_6, two different points on wires 2 and 3, and equal witness values on
    each of the three pairs; a zero and an r - 1; a live wire on either side of the two-shard boundary"""
    from oracle import bn254_ref as o
    from nim_groth16_amd.bn128 import primeR as R
    zk, wit = keys["branches"][0], keys["branches"][1]
    G = o.G1
    a1 = [o.g1_from_bytes(zk.pPoints.pointsA1[i:i + 64]) for i in range(0, len(zk.pPoints.pointsA1), 64)]
    b1 = [o.g1_from_bytes(zk.pPoints.pointsB1[i:i + 64]) for i in range(0, len(zk.pPoints.pointsB1), 64)]
    d = [G.add(b, G.neg(a)) for a, b in zip(a1, b1)]
    assert d[4] == d[5] and not G.is_inf(d[4]) and wit[4] == wit[5]
    assert d[7] == G.neg(d[6]) and not G.is_inf(d[6]) and wit[6] == wit[7]
    assert d[2] != d[3] and d[2] != G.neg(d[3]) and wit[2] == wit[3] != 0
    assert G.is_inf(d[8]) and wit[9] == 0 and wit[10] == R - 1 and not G.is_inf(d[9]) and not G.is_inf(d[10])
    assert len(a1) == 256 and not G.is_inf(d[127]) and not G.is_inf(d[128])


@pytest.mark.parametrize("mont", [True, False], ids=["montgomery", "wtns"])
@pytest.mark.parametrize("name", ["branches", "squaring", "at_max"])
def test_two_shards_and_both_witness_layouts_give_the_unsharded_bytes(ctx, keys, proved, name, mont):
    """two shards on one device: each keeps the live wires of its own range (the squaring chain's second shard none),
    the whole-range count decides for both; the witness as Montgomery limbs and as the .wtns file holds it"""
    from nim_groth16_amd import loadProvingKey
    from nim_groth16_amd import bn128 as F
    zk, wit, wb, r, s, live = keys[name]
    rb, sb = F.frToMontBytes(r), F.frToMontBytes(s)
    w = wb if mont else F.frSeqToStdBytes(wit)
    want = bytes.fromhex(proved[name]["proof"])
    half = len(wit) // 2
    pk = loadProvingKey(zk, ctx)
    shards = [loadProvingKey(zk, ctx, shard_index=k, shard_count=2) for k in range(2)]
    try:
        assert b"".join(pk.prove(w, mont=mont, r=rb, s=sb)) == want
        assert [k.b1_sparse() for k in shards] == [
            {"sparse": True, "live": sum(i < half for i in live), "max": SPARSE_MAX},
            {"sparse": True, "live": sum(i >= half for i in live), "max": SPARSE_MAX}]
        recs = b"".join(k.prove_partials(w, mont=mont) for k in shards)
        for k in shards:
            assert b"".join(k.prove_combine(recs, 2, rb, sb)) == want
    finally:
        for k in shards + [pk]:
            k.destroy()


def test_pool_and_group_prove_the_same_bytes(ctx, keys, proved):
    from nim_groth16_amd import DeviceGroup, ProverPool, loadGroupKey, loadProvingKey
    from nim_groth16_amd import bn128 as F
    zk, _wit, wb, r, s, _live = keys["branches"]
    rb, sb = F.frToMontBytes(r), F.frToMontBytes(s)
    want = bytes.fromhex(proved["branches"]["proof"])
    pk = loadProvingKey(zk, ctx)
    pool = ProverPool(pk, depth=2)
    try:
        tickets = [pool.submit(wb, r=rb, s=sb) for _ in range(2)]
        assert [b"".join(pool.collect(t)) for t in tickets] == [want, want]
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
