#!/usr/bin/env python3
"""The circuit audit measured at 2^log2n constraints (default 20), one process, one box: g16_circuit_audit on the
squaring-chain key, its r1cs and a ptau made from the same toxic waste -- wall time of the C call on prebuilt
descriptors, then one call with every launch bracketed by HIP events to say which pass takes the time.  A record, not a
gate: nothing compares against it.

  python tools/perf_circuit_audit.py [--log2n 20] [--repeats 3] [--out profiles/circuit_audit_2p20.txt]"""
import argparse
import ctypes
import gc
import os
import secrets
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nim_groth16_amd import Context  # noqa: E402
from nim_groth16_amd import fake_setup as FS  # noqa: E402
from nim_groth16_amd._lib import VkeyDesc, device_code_sha16  # noqa: E402
from nim_groth16_amd.files.zkey import ptauDesc, r1csDesc  # noqa: E402
from nim_groth16_amd.prover import pkeyDesc  # noqa: E402
from nim_groth16_amd.synthetic import SplitMix64, squaringChain  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = args.out or os.path.join(ROOT, "profiles", f"circuit_audit_2p{args.log2n}.txt")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"Circuit audit at 2^{args.log2n} (MI355X, one session, one box, {time.strftime('%Y-%m-%d')}); "
        f"library kernels {device_code_sha16()}")
    gc.disable()
    ctx = Context(0)
    ctx.selftest()
    rng = SplitMix64(5)
    tox = FS.ToxicWaste(*[rng.fr() for _ in range(5)])
    r1cs, _ = squaringChain((1 << args.log2n) - 2, seed=4)
    t0 = time.perf_counter()
    zk = FS.fakeCircuitSetup(r1cs, tox, 1, ctx)
    t1 = time.perf_counter()
    hdr = zk.header
    pt = FS.fakePtau(tox.tau, tox.alpha, tox.beta, hdr.logDomainSize + 1, ctx)
    t2 = time.perf_counter()
    say(f"squaring chain: nvars {hdr.nvars}, domain 2^{hdr.logDomainSize}, {len(zk.coeffs)} coefficients; ptau of power "
        f"{pt.power} ({(len(pt.tauG1) + len(pt.tauG2) + len(pt.alphaTauG1) + len(pt.betaTauG1)) / 2**20:.0f} MiB)"
        f"\n(made here: fake setup {t1 - t0:.2f} s, fake ptau {t2 - t1:.2f} s -- not part of the audit)")
    desc, bufs, raw4 = pkeyDesc(zk)
    sp = zk.specPoints
    vbufs = [ctypes.create_string_buffer(x, len(x)) for x in (sp.alpha1, sp.beta2, sp.gamma2, sp.delta2, zk.pointsIC)]
    va = [ctypes.cast(b, ctypes.c_void_p) for b in vbufs]
    vk = VkeyDesc(hdr.npubs, va[0], va[1], va[2], va[3], va[4])
    rd, rkeep = r1csDesc(r1cs, hdr.flavour)
    pd, pkeep = ptauDesc(pt)
    draw = lambda k: b"".join((secrets.randbelow((1 << 128) - 1) + 1).to_bytes(16, "little") for _ in range(k))   # noqa: E731
    zw, zh = draw(hdr.nvars), draw(hdr.domainSize)

    def audit():
        t = time.perf_counter()
        rep = ctx.circuit_audit(desc, vk, raw4, rd, pd, zw, zh)
        t = time.perf_counter() - t
        if not rep.ok:
            raise SystemExit("the audit rejects an honest key:\n" + str(rep))
        return t

    def key_audit():
        t = time.perf_counter()
        ctx.key_audit(desc, vk, section4=raw4, multipliers=zw)
        return time.perf_counter() - t
    audit(), key_audit()
    say(f"\nwall time of the C call on prebuilt descriptors (host checks, matrix arrangement, pageable uploads, kernels),\n"
        f"g16_key_audit on the same key beside it (it is the first part of the circuit audit); {args.repeats} repeats after "
        f"one warm-up of each")
    ta, tk = [], []
    for rep in range(args.repeats):
        ta.append(audit())
        tk.append(key_audit())
        say(f"   #{rep}: g16_circuit_audit {ta[-1]:7.3f} s   g16_key_audit {tk[-1]:7.3f} s")
    ta.sort(), tk.sort()
    say(f"   median: g16_circuit_audit {ta[len(ta) // 2]:.3f} s, of which g16_key_audit {tk[len(tk) // 2]:.3f} s")
    ctx.profile(True)
    ctx.profile_reset()
    t = time.perf_counter()
    ctx.circuit_audit(desc, vk, raw4, rd, pd, zw, zh)
    wall = time.perf_counter() - t
    kern = ctx.profile_report()
    ctx.profile(False)
    say(f"\none audit with every launch bracketed by events ({wall:.3f} s wall); kernel time by pass, ms:")
    total = 0.0
    for k, v in sorted(kern.items(), key=lambda kv: -kv[1]["total_ms"]):
        say(f"     {k:28s} {v['total_ms']:9.2f}  ({v['calls']} launches)")
        total += v["total_ms"]
    say(f"     {'all kernels':28s} {total:9.2f}   -> host side (range and canonical scans, arranging three sparse "
        f"matrices, multipliers, pageable uploads, waits): {wall * 1e3 - total:.0f} ms")
    ctx.close()
    del bufs, vbufs, rkeep, pkeep
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
