#!/usr/bin/env python3
"""fakeCircuitSetup end to end, scalar side on the host (Python integers: the path before g16_fake_setup) against scalar
side on the device (one g16_fake_setup call), on bench.py's two circuits: the squaring chain and the Poseidon-shaped
Merkle path at 2^log2n constraints.  Same process, same box, alternating host / device, three repeats each; the keys of
the two paths are compared byte for byte.  Per-stage split: for the host path the wall time inside lagrangeTaus,
columnDots and Context.fixed_base (the rest is the Python loops over the wires and the domain); for the device path the
library's kernel times (HIP events) next to the wall time of the call.

The host path's Lagrange cache is emptied before every repeat: each figure is one setup from nothing.  (bench.py builds
its two keys from one toxic waste, so its second setup finds the values of the first: see the `warm` line.)

  python tools/perf_setup.py [--log2n 20] [--repeats 3] [--out profiles/fake_setup_ab.txt]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fake_setup_ab.txt"))
    args = ap.parse_args()
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
