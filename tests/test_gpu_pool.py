"""The prover pool (include/g16hip.h "prover pool"; nim_groth16_amd.ProverPool) on the GPU: every proof that comes out
of it is byte for byte the proof g16_prove gives for the same witness and mask -- out of ticket order, for every witness
flag, both flavours, the frozen Poseidon-shaped circuit and the 2^20 benchmark shape -- and the submit / poll / collect
contract holds (busy code, ticket counter, non-blocking poll, ticket errors, destroy with proofs outstanding)."""
import json
import os
import time

import pytest

from oracle import bn254_ref as o
from tests import inputs as I

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _setup(ctx, log2n, flavour=1, seed=5):
    from nim_groth16_amd import loadProvingKey
    from nim_groth16_amd.fake_setup import ToxicWaste, fakeCircuitSetup
    from nim_groth16_amd.synthetic import SplitMix64, squaringChain
    m = (1 << log2n) - 2
    r1cs, wit = squaringChain(m, seed=4)
    rng = SplitMix64(seed)
    zk = fakeCircuitSetup(r1cs, ToxicWaste(*[rng.fr() for _ in range(5)]), flavour, ctx)
    return zk, loadProvingKey(zk, ctx), wit


@pytest.fixture(scope="module")
def small(ctx):
    """2^14 squaring chain, 7 satisfying witnesses (different free input w_0) and 7 masks"""
    from nim_groth16_amd.synthetic import squaringChain
    zk, pk, wit0 = _setup(ctx, 14)
    m = (1 << 14) - 2
    wits = [wit0] + [squaringChain(m, seed=4, w0=w0)[1] for w0 in (5, 7, 11, 13, 17, 19)]
    rng = o.SplitMix64(77)
    masks = [(rng.fr(), rng.fr()) for _ in wits]
    yield zk, pk, wits, masks
    pk.destroy()


def _mb(x):
    return o.fr_to_mont_bytes(x)


def _submit_until_busy(pool, jobs):
    """submit (witness, r, s) jobs until G16_EBUSY -> tickets of the accepted ones"""
    from nim_groth16_amd._lib import G16_EBUSY, G16Error
    tickets = []
    for w, r, s in jobs:
        try:
            tickets.append(pool.submit(w, r=r, s=s))
        except G16Error as e:
            assert e.code == G16_EBUSY
            break
    return tickets


def test_pool_bit_exact_out_of_order_one_thread(ctx, orc, small):
    from nim_groth16_amd import Proof, ProverPool, extractVKey, verifyProof
    from tests.parity import check_gpu_proof
    zk, pk, wits, masks = small
    wbs = [I.fr_mont_bytes(w) for w in wits]
    jobs = [(wb, _mb(r), _mb(s)) for wb, (r, s) in zip(wbs, masks)]
    pool = ProverPool(pk, depth=3)
    try:
        first = _submit_until_busy(pool, jobs)
        assert first == [1, 2, 3, 4]                        # depth + 1 accepted, tickets from 1
        got = {t: pool.collect(t) for t in (3, 1, 2)}
        rest = [pool.submit(w, r=r, s=s) for w, r, s in jobs[4:]]
        assert rest == [5, 6, 7]
        for t in [4] + rest:
            got[t] = pool.collect(t)
    finally:
        pool.close()
    vk = extractVKey(zk)
    for t in range(1, 8):
        wb, (r, s) = wbs[t - 1], masks[t - 1]
        assert got[t] == pk.prove(wb, r=_mb(r), s=_mb(s)), t
        assert verifyProof(vk, Proof(wb[:32 * (zk.header.npubs + 1)], *got[t]), ctx), t
    r, s = masks[2]
    check_gpu_proof(orc, zk, wits[2], wbs[2], r, s, got[3], ctx)     # the full oracle check on one of them


def test_pool_witness_flags_and_jensgroth(ctx, small):
    import torch
    from nim_groth16_amd import HostBuffer, ProverPool
    zk, pk, wits, masks = small
    wit, (r, s) = wits[1], masks[1]
    std, mont = I.fr_std_bytes(wit), I.fr_mont_bytes(wit)
    pinned = HostBuffer.from_bytes(std)
    dev = torch.frombuffer(bytearray(mont), dtype=torch.uint8).to("cuda")
    torch.cuda.synchronize()
    pool = ProverPool(pk, depth=3)
    try:
        ts = [pool.submit(pinned, mont=False, r=_mb(r), s=_mb(s)),
              pool.submit(std, mont=False, r=_mb(r), s=_mb(s)),
              pool.submit(mont, r=_mb(r), s=_mb(s)),
              pool.submit(dev, device=True, r=_mb(r), s=_mb(s))]
        got = [pool.collect(t) for t in ts]
    finally:
        pool.close()
        pinned.free()
    assert got[0] == got[1] == got[2] == got[3] == pk.prove(mont, r=_mb(r), s=_mb(s))
    # the JensGroth flavour (7 NTTs, prover.nim:118-148) through the pool
    zkj, pkj, witj = _setup(ctx, 10, flavour=0, seed=6)
    try:
        wb = I.fr_mont_bytes(witj)
        pool = ProverPool(pkj, depth=2)
        try:
            t = pool.submit(wb, r=_mb(r), s=_mb(s))
            pj = pool.collect(t)
        finally:
            pool.close()
        assert pj == pkj.prove(wb, r=_mb(r), s=_mb(s))
    finally:
        pkj.destroy()


def test_pool_contract(ctx, small):
    from nim_groth16_amd import G16Error, ProverPool, loadProvingKey
    from nim_groth16_amd._lib import G16_EBUSY, G16_EINVAL
    zk, pk, wits, masks = small
    wbs = [I.fr_mont_bytes(w) for w in wits]
    ref = [pk.prove(wb) for wb in wbs[:5]]
    pool = ProverPool(pk, depth=2)
    try:
        ts = [pool.submit(wbs[i]) for i in range(3)]
        assert ts == [1, 2, 3]
        with pytest.raises(G16Error) as e:                  # the depth + 2-th submit
            pool.submit(wbs[3])
        assert e.value.code == G16_EBUSY
        assert pool.collect(1) == ref[0]
        assert pool.submit(wbs[3]) == 4                     # the refused submit did not take a ticket
        for t, bad in ((1, "collected"), (0, "zero"), (99, "unknown")):
            with pytest.raises(G16Error) as e:
                pool.collect(t)
            assert e.value.code == G16_EINVAL, bad
            with pytest.raises(G16Error) as e:
                pool.poll(t)
            assert e.value.code == G16_EINVAL, bad
        assert [pool.collect(t) for t in (2, 3, 4)] == ref[1:4]
        with pytest.raises(G16Error) as e:
            pool.collect(4)
        assert e.value.code == G16_EINVAL
    finally:
        pool.close()
    # destroy with depth + 1 proofs outstanding returns, and the key still proves
    pool = ProverPool(pk, depth=3)
    for i in range(4):
        pool.submit(wbs[i])
    pool.close()
    assert pk.prove(wbs[4]) == ref[4]
    # creation rules
    for depth in (0, 9):
        with pytest.raises(G16Error) as e:
            ProverPool(pk, depth=depth)
        assert e.value.code == G16_EINVAL
    with pytest.raises(G16Error) as e:
        ProverPool(pk, depth=3, device=1)                   # the key belongs to device 0
    assert e.value.code == G16_EINVAL
    shard = loadProvingKey(zk, ctx, shard_index=0, shard_count=2)
    try:
        with pytest.raises(G16Error) as e:
            ProverPool(shard, depth=3)
        assert e.value.code == G16_EINVAL
    finally:
        shard.destroy()


def test_pool_golden_poseidon_shape(ctx):
    """tests/golden/poseidon_shape.json through the pool, with the mask test_gpu_golden.py uses: the committed
    proof_snarkjs_masked, byte for byte"""
    from nim_groth16_amd import ProverPool, loadProvingKey
    from nim_groth16_amd.fake_setup import ToxicWaste, fakeCircuitSetup
    from nim_groth16_amd.synthetic import poseidonMerkle
    fx = json.load(open(os.path.join(G, "poseidon_shape.json")))
    vec = json.load(open(os.path.join(G, "oracle_vectors.json")))
    r1cs, wit = poseidonMerkle(**fx["args"])
    wb = I.fr_mont_bytes(wit)
    assert wb.hex() == fx["witness_mont"]
    tw = ToxicWaste(*(int(vec["toxic_waste"][k], 16) for k in ("alpha", "beta", "gamma", "delta", "tau")))
    zk = fakeCircuitSetup(r1cs, tw, 1, ctx)
    pk = loadProvingKey(zk, ctx)
    r, s = int(vec["mask"]["r"], 16), int(vec["mask"]["s"], 16)
    pool = ProverPool(pk, depth=3)
    try:
        pa, pb, pc = pool.collect(pool.submit(wb, r=_mb(r), s=_mb(s)))
    finally:
        pool.close()
        pk.destroy()
    g = fx["proof_snarkjs_masked"]
    assert (pa.hex(), pb.hex(), pc.hex()) == (g["pi_a"], g["pi_b"], g["pi_c"])


def test_pool_fullsize_2p20_and_nonblocking_poll(ctx):
    """the bench circuit shape: 4 witnesses through depth 3 (2 of them in pinned memory), each equal to g16_prove with
    the same inputs; and poll answers 0, then 1, each call far under one proof's time"""
    import numpy as np
    from nim_groth16_amd import HostBuffer, ProverPool
    zk, pk, wit = _setup(ctx, 20)
    try:
        nv = zk.header.nvars
        rng = np.random.default_rng(20)
        wbs = [I.fr_mont_bytes(wit)]
        for _ in range(3):                                   # canonical values (< 2^252 < r); any vector proves
            a = rng.integers(0, 256, size=(nv, 32), dtype=np.uint8)
            a[:, 31] &= 0x0F
            wbs.append(a.tobytes())
        srng = o.SplitMix64(21)
        masks = [(_mb(srng.fr()), _mb(srng.fr())) for _ in wbs]
        pins = [HostBuffer.from_bytes(wbs[1]), HostBuffer.from_bytes(wbs[3])]
        inputs = [wbs[0], pins[0], wbs[2], pins[1]]
        t0 = time.perf_counter()
        refs = [pk.prove(wb, r=r, s=s) for wb, (r, s) in zip(wbs, masks)]
        one_proof = (time.perf_counter() - t0) / len(wbs)
        pool = ProverPool(pk, depth=3)
        try:
            ts = [pool.submit(x, r=r, s=s) for x, (r, s) in zip(inputs, masks)]
            got = [pool.collect(t) for t in ts]
            assert got == refs
            # poll: a 2^20 proof runs for milliseconds after submit has returned
            t = pool.submit(wbs[0], r=masks[0][0], s=masks[0][1])
            seen, worst, deadline = [], 0.0, time.perf_counter() + 30
            while not seen or not seen[-1]:
                assert time.perf_counter() < deadline, "proof never finished"
                c0 = time.perf_counter()
                seen.append(pool.poll(t))
                worst = max(worst, time.perf_counter() - c0)
                time.sleep(0.0002)
            assert seen[0] is False and seen[-1] is True
            assert worst < 0.25 * one_proof, (worst, one_proof)
            assert pool.collect(t) == refs[0]
        finally:
            pool.close()
            for p in pins:
                p.free()
    finally:
        pk.destroy()
