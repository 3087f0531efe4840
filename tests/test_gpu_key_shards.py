"""Every shard of a sharded key: what it reports and what it proves.

A key created with shard_count = G holds the index ranges [N i / G, N (i + 1) / G) of its point sets (wires for A1, B1,
B2 and C1, domain indices for H1).  For the smallest keys that reach every form of pointsB1 (tests/test_gpu_b1_fold.py:
the hand-built rows, DELTA through the doubling and the general branch of the difference; the same 66 wires with pointsA1
copied over pointsB1, EMPTY; the 2^8 squaring chain, DELTA with two live differences) and for G in 1, 2, 3 and 7 -- 66
wires in 7 ranges of unequal length -- every shard is created and held to a recount of the key's bytes on the host:
  * g16_pkey_b1_fold is the whole key's on every shard;
  * g16_pkey_inf_counts is the shard's: the (0,0) points of A1, of pointsB1 itself (whatever the key keeps in its place),
    of B2, of C1 without the public wires the library pads it with, of H1; the wires dead in both B sets; and whether A1
    and the B pair run on compacted entry lists (G16_INF_COMPACT at its default of 10 %);
  * the partials of all shards, combined on any of them, are the C oracle's proof bit for bit."""
import copy
import os

import pytest

from tests.test_gpu_b1_fold import circuit, recount, rule

pytestmark = pytest.mark.gpu
KEYS = ("hand", "hand_equal_arrays", "squaring")
SHARD_COUNTS = (1, 2, 3, 7)
PCT = 10            # G16_INF_COMPACT's default


def chunk(N, i, G):
    """the range of shard i of G (nim_groth16_amd/distributed.py, msm.nim:105-115)"""
    return (N * i) // G, (N * (i + 1)) // G


def sparse(n_inf, n):
    """enough (0,0) points for entry lists of their own"""
    return n_inf > 0 and n_inf * 100 >= PCT * n


def n_inf(points, size, lo, hi):
    return sum(points[size * i:size * (i + 1)] == bytes(size) for i in range(lo, hi))


def want_inf_counts(zk, form, i, G):
    """g16_pkey_inf_counts of shard i of G, from the key's bytes"""
    hdr, pts = zk.header, zk.pPoints
    w_lo, w_hi = chunk(hdr.nvars, i, G)
    h_lo, h_hi = chunk(hdr.domainSize, i, G)
    nw = w_hi - w_lo
    a1 = n_inf(pts.pointsA1, 64, w_lo, w_hi)
    b1 = n_inf(pts.pointsB1, 64, w_lo, w_hi)
    b2 = n_inf(pts.pointsB2, 128, w_lo, w_hi)
    # pointsC1[j] belongs to wire npubs + 1 + j; the public wires of the range have no C1 point
    c1 = n_inf(pts.pointsC1, 64, max(w_lo, hdr.npubs + 1) - hdr.npubs - 1, max(w_hi, hdr.npubs + 1) - hdr.npubs - 1)
    h1 = n_inf(pts.pointsH1, 64, h_lo, h_hi)
    # DELTA: B1_i = (0,0) <=> B2_i = (0,0) in a key, and only B2 reads the arrangement: B2's own count.  The other forms:
    # wires where both are (0,0)
    if form == "DELTA":
        dead = b2
    else:
        dead = sum(pts.pointsB1[64 * w:64 * w + 64] == bytes(64) and pts.pointsB2[128 * w:128 * w + 128] == bytes(128)
                   for w in range(w_lo, w_hi))
    return {"A1": a1, "B1": b1, "B2": b2, "C1": c1, "H1": h1, "B1_and_B2": dead,
            "compact_A": nw > 0 and sparse(a1, nw), "compact_B": nw > 0 and sparse(dead, nw)}


@pytest.fixture(scope="module")
def keys(ctx, orc):
    """name -> (zkey, witness bytes, r, s, the C oracle's proof): every setup and every reference once"""
    from nim_groth16_amd import bn128 as F
    from nim_groth16_amd.fake_setup import ToxicWaste, fakeCircuitSetup
    from nim_groth16_amd.synthetic import SplitMix64
    from oracle import bn254_ref as o
    from tests.parity import oracle_proof
    assert "G16_B1_FOLD" not in os.environ and "G16_INF_COMPACT" not in os.environ
    out = {}
    for k, name in enumerate(KEYS):
        r1cs, wit = circuit("squaring" if name == "squaring" else "hand")
        rng = SplitMix64(31 + k)
        zk = fakeCircuitSetup(r1cs, ToxicWaste(*[rng.fr() for _ in range(5)]), 1, ctx)
        if name == "hand_equal_arrays":
            zk = copy.copy(zk)
            zk.pPoints = copy.copy(zk.pPoints)
            zk.pPoints.pointsB1 = zk.pPoints.pointsA1
        wb, r, s = F.frSeqToMontBytes(wit), rng.fr(), rng.fr()
        ref, _oz, _ = oracle_proof(orc, zk, wit, wb, r, s)
        out[name] = (zk, wb, F.frToMontBytes(r), F.frToMontBytes(s),
                     o.g1_to_bytes(ref.pi_a) + o.g2_to_bytes(ref.pi_b) + o.g1_to_bytes(ref.pi_c))
    return out


def test_the_keys_are_the_ones_meant(keys):
    assert keys["hand"][0].header.nvars == 66 and keys["hand_equal_arrays"][0].header.nvars == 66
    forms = {name: rule(*recount(keys[name][0]), keys[name][0].header.nvars, PCT) for name in KEYS}
    assert forms == {"hand": "DELTA", "hand_equal_arrays": "EMPTY", "squaring": "DELTA"}
    # live points and points at infinity in A1, B1 and B2 of the hand-built key (every wire is in some matrix, so C1's
    # only infinities are the library's padding of the public wires), and 7 ranges of unequal length
    pts = keys["hand"][0].pPoints
    assert all(0 < n_inf(p, sz, 0, len(p) // sz) < len(p) // sz
               for p, sz in ((pts.pointsA1, 64), (pts.pointsB1, 64), (pts.pointsB2, 128)))
    assert n_inf(pts.pointsC1, 64, 0, len(pts.pointsC1) // 64) == 0
    assert len({hi - lo for lo, hi in (chunk(66, i, 7) for i in range(7))}) > 1


@pytest.mark.parametrize("shard_count", SHARD_COUNTS)
@pytest.mark.parametrize("name", KEYS)
def test_every_shard_reports_its_range_and_the_shards_prove_the_oracles_proof(ctx, keys, name, shard_count):
    from nim_groth16_amd import loadProvingKey
    zk, wb, rb, sb, want = keys[name]
    live_b1, live_delta = recount(zk)
    fold = {"form": rule(live_b1, live_delta, zk.header.nvars, PCT), "live_b1": live_b1, "live_delta": live_delta}
    shards = []
    try:
        for i in range(shard_count):
            shards.append(loadProvingKey(zk, ctx, shard_index=i, shard_count=shard_count))
        for i, k in enumerate(shards):
            got_fold, got_inf = k.b1_fold(), k.inf_counts()
            print(name, "shard", i, "of", shard_count, got_fold, got_inf)
            assert got_fold == fold, (i, shard_count)
            assert got_inf == want_inf_counts(zk, fold["form"], i, shard_count), (i, shard_count)
        recs = b"".join(k.prove_partials(wb) for k in shards)
        assert len(recs) == 768 * shard_count
        for k in shards:
            assert b"".join(k.prove_combine(recs, shard_count, rb, sb)) == want
    finally:
        for k in shards:
            k.destroy()
