#!/usr/bin/env python3
"""The key audit measured at 2^log2n constraints (default 20), one process, one box:

 1. the order-r kernel: tools/ubench_subgroup (the library's fixed-schedule kernel beside the same pass built with the
    generic double-and-add ladder of pairing.hip), 2^log2n G2 points, alternating launches;
 2. the whole audit: g16_key_audit on the squaring-chain key beside g16_pkey_create on the same key, alternating, with
    the audit's kernel times (HIP events, a run of their own) to say which pass takes the time.  g16_pkey_create is the
    parent commit's: this change does not touch it.

  python tools/perf_audit.py [--log2n 20] [--repeats 3] [--out profiles/key_audit_2p20.txt]"""
import argparse
import gc
import os
import secrets
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nim_groth16_amd import Context  # noqa: E402
from nim_groth16_amd import fake_setup as FS  # noqa: E402
from nim_groth16_amd._lib import ProvingKey, VkeyDesc, device_code_sha16  # noqa: E402
from nim_groth16_amd.prover import pkeyDesc  # noqa: E402
from nim_groth16_amd.synthetic import SplitMix64, squaringChain  # noqa: E402


def ubench(log2n):
    exe = os.path.join(ROOT, "tools", "ubench_subgroup")
    if not os.path.exists(exe):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950",
                               "-I" + os.path.join(ROOT, "include"), exe + ".hip",
                               "-L" + os.path.join(ROOT, "nim_groth16_amd", "csrc"), "-lg16hip",
                               "-Wl,-rpath,$ORIGIN/../nim_groth16_amd/csrc", "-o", exe])
    return subprocess.run([exe, str(log2n), "5"], check=True, capture_output=True, text=True).stdout.rstrip().split("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = args.out or os.path.join(ROOT, "profiles", f"key_audit_2p{args.log2n}.txt")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"Key audit at 2^{args.log2n} (MI355X, one session, one box, {time.strftime('%Y-%m-%d')}); "
        f"library kernels {device_code_sha16()}")
    say("\n1. the order-r pass over an array of G2 points (tools/ubench_subgroup: HIP events around single launches, one "
        "warm-up each,\n   the kernels alternating; points = random multiples of gen2)")
    for ln in ubench(args.log2n):
        say("   " + ln)

    gc.disable()
    ctx = Context(0)
    ctx.selftest()
    rng = SplitMix64(5)
    tox = FS.ToxicWaste(*[rng.fr() for _ in range(5)])
    r1cs, _ = squaringChain((1 << args.log2n) - 2, seed=4)
    zk = FS.fakeCircuitSetup(r1cs, tox, 1, ctx)
    hdr = zk.header
    say(f"\n2. g16_key_audit beside g16_pkey_create, squaring chain: nvars {hdr.nvars}, domain 2^{hdr.logDomainSize}, "
        f"{len(zk.coeffs)} coefficients\n   (wall time of the C call on one prebuilt descriptor: checks, uploads, kernels; alternating, "
        f"{args.repeats} repeats after one warm-up of each)")
    import ctypes
    desc, bufs, _ = pkeyDesc(zk)                                   # one descriptor for both: the calls alone are timed
    sp = zk.specPoints
    vbufs = [ctypes.create_string_buffer(x, len(x)) for x in (sp.alpha1, sp.beta2, sp.gamma2, sp.delta2, zk.pointsIC)]
    va = [ctypes.cast(b, ctypes.c_void_p) for b in vbufs]
    vk = VkeyDesc(hdr.npubs, va[0], va[1], va[2], va[3], va[4])
    zs = b"".join((secrets.randbelow((1 << 128) - 1) + 1).to_bytes(16, "little") for _ in range(hdr.nvars))

    def create():
        t0 = time.perf_counter()
        pk = ProvingKey(ctx, desc, bufs)
        t = time.perf_counter() - t0
        pk.destroy()
        return t

    def audit():
        t0 = time.perf_counter()
        rep = ctx.key_audit(desc, vk, multipliers=zs)
        t = time.perf_counter() - t0
        if not rep.ok:
            raise SystemExit("the audit rejects an honest key:\n" + str(rep))
        return t
    create(), audit()
    tc, ta = [], []
    for rep in range(args.repeats):
        tc.append(create())
        ta.append(audit())
        say(f"   #{rep}: g16_pkey_create {tc[-1]:7.3f} s   g16_key_audit {ta[-1]:7.3f} s")
    tc.sort(), ta.sort()
    mc, ma = tc[len(tc) // 2], ta[len(ta) // 2]
    say(f"   median: g16_pkey_create {mc:.3f} s, g16_key_audit {ma:.3f} s  (audit / create = {ma / mc:.2f}; aim: the audit "
        f"takes no longer than key creation: {'met' if ma <= mc else 'NOT met'})")
    ctx.profile(True)
    ctx.profile_reset()
    t0 = time.perf_counter()
    ctx.key_audit(desc, vk, multipliers=zs)
    wall = time.perf_counter() - t0
    kern = ctx.profile_report()
    ctx.profile(False)
    say(f"   one audit with every launch bracketed by events ({wall:.3f} s wall); kernel time by pass, ms:")
    total = 0.0
    for k, v in sorted(kern.items(), key=lambda kv: -kv[1]["total_ms"]):
        say(f"     {k:28s} {v['total_ms']:9.2f}  ({v['calls']} launches)")
        total += v["total_ms"]
    say(f"     {'all kernels':28s} {total:9.2f}   -> host side (coefficient scan, multipliers, pageable uploads of "
        f"{(5 * 64 + 128) * hdr.nvars / 2**20:.0f} MiB, waits): {wall * 1e3 - total:.0f} ms")
    ctx.close()
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
