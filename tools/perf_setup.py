#!/usr/bin/env python3
"""fakeCircuitSetup end to end, scalar side on the host (Python integers: the path before g16_fake_setup) against scalar
side on the device (one g16_fake_setup call), on bench.py's two circuits: the squaring chain and the Poseidon-shaped
Merkle path at 2^log2n constraints.  Same process, same box, alternating host / device, three repeats each; the keys of
the two paths are compared byte for byte.  Per-stage split: for the host path the wall time inside lagrangeTaus,
columnDots and Context.fixed_base (the rest is the Python loops over the wires and the domain); for the device path the
library's kernel times (HIP events) next to the wall time of the call.

The host path's Lagrange cache is emptied before every repeat: each figure is one setup from nothing.  (bench.py builds
its two keys from one toxic waste, so its second setup finds the values of the first: see the `warm` line.)

  python tools/perf_setup.py [--log2n 20] [--repeats 3] [--out profiles/fake_setup_ab.txt]

--circuit-setup: the real setup instead -- circuitSetup (one g16_circuit_setup call: group inverse NTTs and sparse matrix x
point vector products) from the circuit and a fakePtau of power log2n + 1, on the same two circuits, with the library's
per-kernel times; beside it fakeCircuitSetup (g16_fake_setup) for the same (alpha, beta, gamma = 1, delta = 1, tau) as the
only available yardstick -- it does one fixed-base multiplication where the real setup does a transform -- and the two
keys compared byte for byte.

  python tools/perf_setup.py --circuit-setup [--log2n 20] [--repeats 2] [--out profiles/circuit_setup_2p20.txt]

--contribute: the phase-2 contribution instead -- the whole g16_key_contribute and g16_contributions_verify (a chain of 3
records) on the part of a key a contribution touches at 2^log2n: pointsC1 and pointsH1 of 2^log2n points each (random
multiples of gen1; no circuit is needed: the two calls read nothing else of a key), wall time of the Python call and the
library's per-kernel times.  The chain is checked to verify, and to fail once a point of the final key is moved.

  python tools/perf_setup.py --contribute [--log2n 20] [--repeats 3] [--out FILE]

--ptau-contribute: the phase-1 contribution instead -- the whole g16_ptau_contribute on a fakePtau of power log2n (tauG1 of
2^(log2n+1) - 1 points, the three shorter arrays of 2^log2n), wall time of the Python call and the library's per-kernel
times; the result of every call is compared with the fakePtau of the product of the secrets, byte for byte.

  python tools/perf_setup.py --ptau-contribute [--log2n 21] [--repeats 3] [--out FILE]

--ptau-verify: g16_ptau_verify on the same fakePtau with a chain of no records (the sums and the five fixed products are
what grows with the power), wall time and per-kernel times; then the file with one element of tauG1 doubled must fail.

  python tools/perf_setup.py --ptau-verify [--log2n 21] [--repeats 3] [--out FILE]"""
import argparse
import gc
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nim_groth16_amd import Context  # noqa: E402
from nim_groth16_amd import fake_setup as FS  # noqa: E402
from nim_groth16_amd.synthetic import SplitMix64, poseidonMerkle, squaringChain  # noqa: E402
from nim_groth16_amd.zkey_types import packCoeffs  # noqa: E402


class Stages:
    """wall time spent inside the named functions of the host path"""

    def __init__(self, ctx):
        self.t = {}
        self.ctx = ctx
        self.saved = (FS.lagrangeTaus, FS.columnDots, ctx.fixed_base)

    def wrap(self, name, fn):
        def timed(*a, **k):
            t0 = time.perf_counter()
            try:
                return fn(*a, **k)
            finally:
                self.t[name] = self.t.get(name, 0.0) + time.perf_counter() - t0
        return timed

    def __enter__(self):
        FS.lagrangeTaus = self.wrap("lagrange", self.saved[0])
        FS.columnDots = self.wrap("column_sums", self.saved[1])
        self.ctx.fixed_base = self.wrap("fixed_base", self.saved[2])
        return self

    def __exit__(self, *exc):
        FS.lagrangeTaus, FS.columnDots = self.saved[:2]
        del self.ctx.fixed_base


def same_key(a, b):
    return (a.header == b.header and a.specPoints == b.specPoints and a.pointsIC == b.pointsIC and
            a.pPoints == b.pPoints and packCoeffs(a.coeffs) == packCoeffs(b.coeffs))


def circuit_setup_main(args):
    from nim_groth16_amd.setup import circuitSetup
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    gc.disable()
    ctx = Context(0)
    ctx.selftest()
    rng = SplitMix64(5)
    alpha, beta, _, _, tau = (rng.fr() for _ in range(5))
    tox = FS.ToxicWaste(alpha, beta, 1, 1, tau)
    say(f"circuitSetup (g16_circuit_setup) beside fakeCircuitSetup (g16_fake_setup), 2^{args.log2n} constraints, snarkjs "
        f"flavour, delta = 1, {args.repeats} repeats, one process ({time.strftime('%Y-%m-%d')})")
    t0 = time.perf_counter()
    pt = FS.fakePtau(tau, alpha, beta, args.log2n + 1, ctx)
    say(f"fakePtau, power {args.log2n + 1}: {time.perf_counter() - t0:.1f} s")
    small, _ = squaringChain((1 << 8) - 2, seed=4)
    circuitSetup(small, pt, 1, None, ctx)                                  # warm-up: code objects
    for name, make in (("squaring chain", lambda: squaringChain((1 << args.log2n) - 2, seed=4)),
                       ("Poseidon shape", lambda: poseidonMerkle(args.log2n, seed=4))):
        t0 = time.perf_counter()
        r1cs, _ = make()
        nnz = [len(m[0]) for m in FS._triplets(r1cs)[1:]]
        say(f"\n{name}: nvars {r1cs.nWires}, entries A {nnz[0]} B {nnz[1]} C {nnz[2]}, circuit built in "
            f"{time.perf_counter() - t0:.1f} s")
        zf = FS.fakeCircuitSetup(r1cs, tox, 1, ctx, scalarSide="device")   # warm-up of the yardstick: fixed-base tables
        for rep_i in range(args.repeats):
            t0 = time.perf_counter()
            zf = FS.fakeCircuitSetup(r1cs, tox, 1, ctx, scalarSide="device")
            tf = time.perf_counter() - t0
            ctx.profile(True)
            ctx.profile_reset()
            t0 = time.perf_counter()
            zc = circuitSetup(r1cs, pt, 1, None, ctx)
            tc = time.perf_counter() - t0
            rep_k = ctx.profile_report()
            ctx.profile(False)
            say(f"  #{rep_i}: circuitSetup {tc:7.2f} s (call, with the host's entry sort and the copies)   fakeCircuitSetup {tf:7.2f} s")
            for k, v in sorted(rep_k.items()):
                say(f"        {k:<22} {v['calls']:>4} launches {v['total_ms']:>10.1f} ms")
            say(f"        {'all kernels':<22} {sum(v['calls'] for v in rep_k.values()):>4} launches "
                f"{sum(v['total_ms'] for v in rep_k.values()):>10.1f} ms")
            if not same_key(zf, zc):
                raise SystemExit("circuitSetup and fakeCircuitSetup built different keys")
            del zc
        say("  keys equal byte for byte")
        del r1cs, zf
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


def contribute_main(args):
    import numpy as np
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    from nim_groth16_amd._lib import device_code_sha16
    ctx = Context(0)
    ctx.selftest()
    n = 1 << args.log2n
    rs = np.random.default_rng(20)

    def scalars(count):                                   # standard form, below 2^253, never zero
        a = rs.integers(0, 1 << 63, size=(count, 4), dtype=np.uint64)
        a[:, 3] &= np.uint64((1 << 61) - 1)
        a[:, 0] |= np.uint64(1)
        return a.tobytes()

    def multipliers(count):
        a = rs.integers(0, 1 << 63, size=(count, 2), dtype=np.uint64)
        a[:, 0] |= np.uint64(1)
        return a.tobytes()

    say(f"phase-2 contribution at 2^{args.log2n}: pointsC1 and pointsH1 of {n} points each, {args.repeats} repeats "
        f"({time.strftime('%Y-%m-%d')}; library kernels {device_code_sha16()})")
    delta = scalars(1)                                    # delta1 and delta2: the same multiple of the two generators
    key0 = {"delta1": ctx.fixed_base(1, delta, mont=False), "delta2": ctx.fixed_base(2, delta, mont=False),
            "pointsC1": ctx.fixed_base(1, scalars(n), mont=False), "pointsH1": ctx.fixed_base(1, scalars(n), mont=False)}
    chal = [ctx.fixed_base(2, scalars(1), mont=False) for _ in range(3)]
    zc, zh = multipliers(n), multipliers(n)

    def timed(what, fn):
        ctx.profile(True)
        ctx.profile_reset()
        t0 = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t0
        rep = ctx.profile_report()
        ctx.profile(False)
        kern = "  ".join(f"{k} {v['total_ms']:.2f} ({v['calls']})" for k, v in sorted(rep.items()))
        say(f"  {what}: {dt * 1e3:8.1f} ms wall   kernels, ms (launches): {kern}")
        return out, dt

    ctx.key_contribute(key0, scalars(1), scalars(1), chal[0], mont=False)          # warm-up: allocations, code objects
    walls = {"contribute": [], "verify": []}
    for rep in range(args.repeats):
        key, recs = key0, []
        for j in range(3):
            d, s = scalars(1), scalars(1)
            (key, rec), dt = timed(f"g16_key_contribute #{rep}.{j}", lambda: ctx.key_contribute(key, d, s, chal[j], mont=False))
            recs.append(rec)
            walls["contribute"].append(dt)
        report, dt = timed(f"g16_contributions_verify #{rep} (3 records)",
                           lambda: ctx.contributions_verify(key0, key, recs, chal, zc, zh))
        walls["verify"].append(dt)
        if not report.ok:
            raise SystemExit(f"an honest chain does not verify: {report}")
    moved = dict(key)
    moved["pointsH1"] = key["pointsH1"][64:128] + key["pointsH1"][:64] + key["pointsH1"][128:]
    report = ctx.contributions_verify(key0, moved, recs, chal, zc, zh)
    if report.relation != [1, 1, 1, 1, 1, 1, 0]:
        raise SystemExit(f"two swapped points of pointsH1 are not found: {report}")
    for k, v in walls.items():
        v.sort()
        say(f"  median {k}: {v[len(v) // 2] * 1e3:.1f} ms wall (min {v[0] * 1e3:.1f}, max {v[-1] * 1e3:.1f}, {len(v)} calls)")
    say("  every chain verified; two swapped points of the final pointsH1 give H1 = 0 and nothing else")
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


def ptau_contribute_main(args):
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    from nim_groth16_amd import bn128 as F
    from nim_groth16_amd._lib import PTAU_SECTIONS, device_code_sha16
    ctx = Context(0)
    ctx.selftest()
    power = args.log2n
    rng = SplitMix64(21)
    waste = [rng.fr() or 1 for _ in range(3)]
    say(f"phase-1 contribution at power {power}: tauG1 of {(2 << power) - 1} points, tauG2 / alphaTauG1 / betaTauG1 of "
        f"{1 << power}, {args.repeats} repeats ({time.strftime('%Y-%m-%d')}; library kernels {device_code_sha16()})")
    t0 = time.perf_counter()
    pt = FS.fakePtau(waste[0], waste[1], waste[2], power, ctx)
    say(f"fakePtau, power {power}: {time.perf_counter() - t0:.1f} s")
    arrays = {k: getattr(pt, k) for k in PTAU_SECTIONS}
    chal = ctx.fixed_base(2, F.frSeqToMontBytes([7, 8, 9]))
    small = {k: getattr(FS.fakePtau(1, 1, 1, 3, ctx), k) for k in PTAU_SECTIONS}
    enc = F.frToMontBytes
    ctx.ptau_contribute(small, enc(2), enc(3), enc(4), F.frSeqToMontBytes([5, 6, 7]), chal)   # warm-up: code objects
    walls = []
    for rep in range(args.repeats):
        x = [rng.fr() or 1 for _ in range(6)]
        ctx.profile(True)
        ctx.profile_reset()
        t0 = time.perf_counter()
        new, _ = ctx.ptau_contribute(arrays, enc(x[0]), enc(x[1]), enc(x[2]), F.frSeqToMontBytes(x[3:]), chal, power=power)
        dt = time.perf_counter() - t0
        rep_k = ctx.profile_report()
        ctx.profile(False)
        kern = "  ".join(f"{k} {v['total_ms']:.2f} ({v['calls']})" for k, v in sorted(rep_k.items()))
        say(f"  g16_ptau_contribute #{rep}: {dt * 1e3:8.1f} ms wall   kernels, ms (launches): {kern}")
        walls.append(dt)
        waste = [a * b % F.primeR for a, b in zip(waste, x[:3])]
        want = FS.fakePtau(waste[0], waste[1], waste[2], power, ctx)
        if any(new[k] != getattr(want, k) for k in PTAU_SECTIONS):
            raise SystemExit("the contributed powers are not those of the product of the secrets")
        arrays = new
        del want
    walls.sort()
    say(f"  median: {walls[len(walls) // 2] * 1e3:.1f} ms wall (min {walls[0] * 1e3:.1f}, max {walls[-1] * 1e3:.1f}, "
        f"{len(walls)} calls); every result equals fakePtau of the product of the secrets byte for byte")
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


def ptau_verify_main(args):
    import numpy as np
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    from nim_groth16_amd._lib import PTAU_SECTIONS, device_code_sha16
    ctx = Context(0)
    ctx.selftest()
    power = args.log2n
    rng = SplitMix64(22)
    pt = FS.fakePtau(rng.fr(), rng.fr(), rng.fr(), power, ctx)
    arrays = {k: getattr(pt, k) for k in PTAU_SECTIONS}
    z = np.random.default_rng(23).integers(0, 1 << 63, size=((2 << power) - 2, 2), dtype=np.uint64)
    z[:, 0] |= np.uint64(1)
    z = z.tobytes()
    say(f"g16_ptau_verify at power {power}, no records, {args.repeats} repeats ({time.strftime('%Y-%m-%d')}; library kernels "
        f"{device_code_sha16()})")
    small = {k: getattr(FS.fakePtau(2, 3, 5, 3, ctx), k) for k in PTAU_SECTIONS}
    ctx.ptau_verify(small, None, None, [3] * 14)                                   # warm-up: code objects
    walls = []
    for rep in range(args.repeats):
        ctx.profile(True)
        ctx.profile_reset()
        t0 = time.perf_counter()
        report = ctx.ptau_verify(arrays, None, None, z, power=power)
        dt = time.perf_counter() - t0
        rep_k = ctx.profile_report()
        ctx.profile(False)
        kern = "  ".join(f"{k} {v['total_ms']:.2f} ({v['calls']})" for k, v in sorted(rep_k.items()))
        say(f"  g16_ptau_verify #{rep}: {dt * 1e3:8.1f} ms wall   kernels, ms (launches): {kern}")
        walls.append(dt)
        if report.relation != [1] * 7 + [-1] * 3:
            raise SystemExit(f"honest powers do not verify: {report}")
    bad = dict(arrays)
    k = 12345 % ((2 << power) - 1)
    dbl = ctx.points_scale(1, arrays["tauG1"][64 * k:64 * k + 64], (2).to_bytes(32, "little"), mont=False)
    bad["tauG1"] = arrays["tauG1"][:64 * k] + dbl + arrays["tauG1"][64 * k + 64:]
    report = ctx.ptau_verify(bad, None, None, z, power=power)
    if report.relation[2] != 0:
        raise SystemExit(f"a doubled element of tauG1 is not found: {report}")
    walls.sort()
    say(f"  median: {walls[len(walls) // 2] * 1e3:.1f} ms wall (min {walls[0] * 1e3:.1f}, max {walls[-1] * 1e3:.1f}); honest "
        f"powers verify, tauG1[{k}] doubled gives TAU_G1 = 0")
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--circuit-setup", action="store_true", help="measure g16_circuit_setup (see the module text)")
    ap.add_argument("--contribute", action="store_true",
                    help="measure g16_key_contribute and g16_contributions_verify (see the module text)")
    ap.add_argument("--ptau-contribute", action="store_true", help="measure g16_ptau_contribute (see the module text)")
    ap.add_argument("--ptau-verify", action="store_true", help="measure g16_ptau_verify (see the module text)")
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fake_setup_ab.txt"))
    args = ap.parse_args()
    if args.circuit_setup:
        return circuit_setup_main(args)
    if args.contribute:
        return contribute_main(args)
    if args.ptau_contribute:
        return ptau_contribute_main(args)
    if args.ptau_verify:
        return ptau_verify_main(args)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    gc.disable()                       # as bench.py does around its setup: millions of tuples, no cycles
    ctx = Context(0)
    ctx.selftest()
    rng = SplitMix64(5)
    tox = FS.ToxicWaste(*[rng.fr() for _ in range(5)])
    say(f"fakeCircuitSetup, scalar side host vs device, 2^{args.log2n} constraints, snarkjs flavour, {args.repeats} repeats, "
        f"alternating, one process ({time.strftime('%Y-%m-%d')})")
    totals = {}
    for name, make in (("squaring chain", lambda: squaringChain((1 << args.log2n) - 2, seed=4)),
                       ("Poseidon shape", lambda: poseidonMerkle(args.log2n, seed=4))):
        t0 = time.perf_counter()
        r1cs, _ = make()
        say(f"\n{name}: nvars {r1cs.nWires}, circuit built in {time.perf_counter() - t0:.1f} s")
        FS.fakeCircuitSetup(r1cs, tox, 1, ctx, scalarSide="device")        # warm-up: fixed-base tables, allocations
        host, dev = [], []
        for rep in range(args.repeats):
            FS._lag_cache.clear()
            with Stages(ctx) as st:
                t0 = time.perf_counter()
                zh = FS.fakeCircuitSetup(r1cs, tox, 1, ctx, scalarSide="host")
                th = time.perf_counter() - t0
            rest = th - sum(st.t.values())
            say(f"  host   #{rep}: {th:7.2f} s   lagrange {st.t.get('lagrange', 0):.2f}  column sums {st.t.get('column_sums', 0):.2f}  "
                f"fixed-base calls {st.t.get('fixed_base', 0):.2f}  Python loops and encoding {rest:.2f}")
            ctx.profile(True)
            ctx.profile_reset()
            t0 = time.perf_counter()
            zd = FS.fakeCircuitSetup(r1cs, tox, 1, ctx, scalarSide="device")
            td = time.perf_counter() - t0
            rep_k = ctx.profile_report()
            ctx.profile(False)
            kern = "  ".join(f"{k} {v['total_ms']:.1f}" for k, v in sorted(rep_k.items()))
            say(f"  device #{rep}: {td:7.2f} s   kernels, ms: {kern}")
            if not same_key(zh, zd):
                raise SystemExit("the two paths built different keys")
            host.append(th), dev.append(td)
            del zh, zd
        if name == "squaring chain":                                       # what bench.py's second setup sees
            t0 = time.perf_counter()
            FS.fakeCircuitSetup(r1cs, tox, 1, ctx, scalarSide="host")
            say(f"  host, warm Lagrange cache (a second key from the same toxic waste): {time.perf_counter() - t0:.2f} s")
        host.sort(), dev.sort()
        say(f"  median: host {host[len(host) // 2]:.2f} s, device {dev[len(dev) // 2]:.2f} s "
            f"(min {host[0]:.2f} / {dev[0]:.2f}, max {host[-1]:.2f} / {dev[-1]:.2f}); keys equal byte for byte")
        totals[name] = (host[len(host) // 2], dev[len(dev) // 2])
        del r1cs
    say("\ncondition for the device default: the device total below the host total on both circuits: " +
        ("met" if all(d < h for h, d in totals.values()) else "NOT met"))
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
