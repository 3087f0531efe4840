#!/usr/bin/env python3
"""Times the GPU verifier: toy-circuit proofs replicated into batches of growing size, through g16_verify, g16_verify
with the order-r check of pi_b, and g16_verify_batch (one pairing product per batch; that check is always on).  The three
paths alternate for REPS rounds in one process; each line gives the best and the median of a path's rounds.  Up to 16 384 proofs every kernel of every path is a
single round of waves, so a call costs the latency of one lane's work whatever the count; the two largest sizes are there
to show the paths once the GPU is full."""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


REPS = 5


def main():
    import random
    from nim_groth16_amd import (Context, Mask, Witness, extractVKey, generateProofWithMask, loadVerifyingKey)
    from nim_groth16_amd.fake_setup import R1CS, ToxicWaste, fakeCircuitSetup
    R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
    rng = random.Random(1)
    fr = lambda x: (x * (1 << 256) % R).to_bytes(32, "little")   # noqa: E731
    ctx = Context(0)
    # the reference's toy circuit (tests/groth16/testProver.nim:17-55)
    cons = [([], [], [(1, R - 1), (2, 1), (7, 1)]), ([(3, 1)], [(4, 1)], [(6, 1)]), ([(5, 1)], [(6, 1)], [(7, 1)])]
    tw = ToxicWaste(*(rng.randrange(1, R) for _ in range(5)))
    zk = fakeCircuitSetup(R1CS(8, 1, 1, 3, cons), tw, 1, ctx)
    wt = Witness("bn128", 8, b"".join(fr(x) for x in [1, 2023, 1022, 7, 11, 13, 77, 1001]))
    prf = generateProofWithMask(0, False, zk, wt, Mask(rng.randrange(R), rng.randrange(R)), ctx)
    dev = loadVerifyingKey(extractVKey(zk), ctx)
    trip = (prf.pi_a, prf.pi_b, prf.pi_c)
    assert dev.verify([trip], prf.publicIO) == [1]
    import secrets
    import statistics
    from nim_groth16_amd._lib import device_code_sha16
    print(f"libg16hip.so device code {device_code_sha16()}; rounds per path: {REPS}", flush=True)
    for n in (1, 64, 1024, 4096, 16384, 65536, 262144):
        proofs, pub = [trip] * n, prf.publicIO * n
        zs = [secrets.randbelow((1 << 128) - 1) + 1 for _ in range(n)]
        paths = [("g16_verify", lambda: dev.verify(proofs, pub) == [1] * n),
                 ("g16_verify subgroup", lambda: dev.verify(proofs, pub, subgroup=True) == [1] * n),
                 ("g16_verify_batch", lambda: dev.verify_batch(proofs, pub, multipliers=zs) is True)]
        times = {name: [] for name, _ in paths}
        for rep in range(REPS + 1):                   # round 0 warms every path up at this size
            for name, run in paths:
                t0 = time.perf_counter()              # every path ends in a stream synchronise inside the library
                ok = run()
                dt = time.perf_counter() - t0
                assert ok, name
                if rep:
                    times[name].append(dt)
        for name, _ in paths:
            best, med = min(times[name]), statistics.median(times[name])
            print(f"{name:20s} {n:6d} proofs: best {best * 1e3:9.2f} ms {n / best:10.1f} proofs/s   "
                  f"median {med * 1e3:9.2f} ms {n / med:10.1f} proofs/s", flush=True)
        b, s = statistics.median(times["g16_verify_batch"]), statistics.median(times["g16_verify subgroup"])
        print(f"{'':20s} {n:6d} proofs: g16_verify_batch / g16_verify subgroup = {b / s:.3f} of the time (medians)",
              flush=True)

if __name__ == "__main__":
    main()
