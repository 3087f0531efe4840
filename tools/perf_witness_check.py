#!/usr/bin/env python3
"""The witness check measured at 2^log2n constraints (default 20), one process, one box: the squaring chain and the
Poseidon-shaped Merkle circuit.  Per circuit: wall time of g16_r1cs_create on a prebuilt description, wall time of
g16_witness_check with the witness in HBM and in pinned host memory, the kernels alone (HIP events inside the library,
g16_profile_report), and -- same session, same line -- the kernel time of g16_build_abc over the circuit's key.  A record,
not a gate: nothing compares against it.

  python tools/perf_witness_check.py [--log2n 20] [--repeats 5] [--out profiles/witness_check_2p20.txt]"""
import argparse
import gc
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from nim_groth16_amd import Context, HostBuffer, loadProvingKey  # noqa: E402
from nim_groth16_amd import bn128 as F  # noqa: E402
from nim_groth16_amd._lib import device_code_sha16  # noqa: E402
from nim_groth16_amd.fake_setup import ToxicWaste, fakeCircuitSetup  # noqa: E402
from nim_groth16_amd.files.zkey import r1csDesc  # noqa: E402
from nim_groth16_amd.synthetic import SplitMix64, poseidonMerkle, squaringChain  # noqa: E402

KERNELS = ("witness_canonical", "witness_spmv", "witness_rows", "witness_list")


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = args.out or os.path.join(ROOT, "profiles", f"witness_check_2p{args.log2n}.txt")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"Witness check at 2^{args.log2n} (MI355X, one session, one box, {time.strftime('%Y-%m-%d')}); "
        f"library kernels {device_code_sha16()}")
    gc.disable()
    ctx = Context(0)
    ctx.selftest()
    rng = SplitMix64(5)
    tox = ToxicWaste(*[rng.fr() for _ in range(5)])
    for name, make in (("squaring chain", lambda: squaringChain((1 << args.log2n) - 2, seed=4)),
                       ("poseidon-merkle", lambda: poseidonMerkle(args.log2n, seed=4))):
        r1cs, wit = make()
        rd, keep = r1csDesc(r1cs, 1)
        ws = F.frSeqToStdBytes(wit)
        bad = list(wit)
        bad[len(bad) // 2] = (bad[len(bad) // 2] + 1) % F.primeR
        wbad = F.frSeqToStdBytes(bad)
        tc = []
        system = None
        for _ in range(3):
            if system:
                system.destroy()
            t = time.perf_counter()
            system = ctx.r1cs_load(rd, keep)
            tc.append(time.perf_counter() - t)
        info = system.info()
        say(f"\n== {name}: nvars {info['nvars']}, {info['nconstraints']} constraints, nnz(A)+nnz(B)+nnz(C) {info['nnz']}, "
            f"value dictionary: {info['dict_values'] or 'none'}")
        say(f"   g16_r1cs_create (host range and canonical scans, arranging the matrix, pageable uploads): "
            f"{median(tc) * 1e3:.1f} ms (3 calls: " + ", ".join(f"{t * 1e3:.1f}" for t in tc) + ")")
        say(f"      (the call first gathers the three matrices into one triplet list of its own, 40 bytes per entry = "
            f"{info['nnz'] * 40 / 2**20:.0f} MiB here, which the sparse-matrix builder then copies and reorders once more: "
            f"transient host memory and one extra pass, both inside this figure)")
        d_w = torch.frombuffer(bytearray(ws), dtype=torch.uint8).cuda()
        d_bad = torch.frombuffer(bytearray(wbad), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        pinned, pinned_bad = HostBuffer.from_bytes(ws), HostBuffer.from_bytes(wbad)

        def timed(ptr, device, want_ok):
            system.check(ptr, mont=False, device=device)
            ts = []
            for _ in range(args.repeats):
                t = time.perf_counter()
                rep = system.check(ptr, mont=False, device=device)
                ts.append(time.perf_counter() - t)
                if rep.ok != want_ok:
                    raise SystemExit("unexpected verdict:\n" + str(rep))
            return median(ts) * 1e3
        say(f"   g16_witness_check, standard-form witness, wall ms (median of {args.repeats} after one warm-up):")
        say(f"      witness in HBM:          satisfied {timed(d_w.data_ptr(), True, True):7.3f}   "
            f"one wire changed {timed(d_bad.data_ptr(), True, False):7.3f}")
        say(f"      witness in pinned host:  satisfied {timed(pinned, False, True):7.3f}   "
            f"one wire changed {timed(pinned_bad, False, False):7.3f}")
        ctx.profile(True)
        ctx.profile_reset()
        for _ in range(args.repeats):
            system.check(d_bad.data_ptr(), mont=False, device=True)
        kern = ctx.profile_report()
        ctx.profile(False)
        per = {k: kern[k]["total_ms"] / kern[k]["calls"] for k in KERNELS if k in kern}
        # the same session's buildABC over the circuit's key
        zk = fakeCircuitSetup(r1cs, tox, 1, ctx)
        pk = loadProvingKey(zk, ctx)
        pk.build_abc(ws, mont=False)
        ctx.profile(True)
        ctx.profile_reset()
        for _ in range(args.repeats):
            pk.build_abc(ws, mont=False)
        abc = ctx.profile_report()
        ctx.profile(False)
        pk.destroy()
        abc_ms = {k: abc[k]["total_ms"] / abc[k]["calls"] for k in ("abc_spmv", "abc_cz") if k in abc}
        say("   kernels alone, ms per call (one wire changed): " + ", ".join(f"{k} {v:.3f}" for k, v in per.items()) +
            f"; all {sum(per.values()):.3f}  |  g16_build_abc of the same circuit's key: " +
            ", ".join(f"{k} {v:.3f}" for k, v in abc_ms.items()) + f"; all {sum(abc_ms.values()):.3f}")
        system.destroy()
        pinned.free(), pinned_bad.free()
        del d_w, d_bad, keep, zk
    ctx.close()
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
