"""The MSM tail kernels (msm_heavy, msm_reduce1, every msm_reduce2 variant, the four folds) at exceptional bucket
pictures: equal, opposite and infinite operands in every chain of the tail, dictated through the C ABI by scalars that
are single digits over points k * G with chosen logs (tests/msm_pictures.py).  One child process per knob set (G16_*
knobs are read once per process); every picture runs for G1 and G2, one-shot and registered, and is compared byte for
byte with (sum s_i k_i mod r) * G -- and with the oracle's naive MSM where n <= 64.  What each picture reaches, and
that the knob sets launch every kernel form, is asserted on the CPU in tests/test_msm_pictures_cpu.py."""
import os
import subprocess
import sys
import time

import pytest

from tests import msm_pictures as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(index):
    from oracle import bn254_ref as o
    from tests import inputs as I
    from tests.oracle_c import load_oracle
    from nim_groth16_amd import Context
    knobs, families = mp.KNOB_SETS[index]
    assert {k: v for k, v in os.environ.items() if k.startswith("G16_")} == knobs
    orc = load_oracle()
    ctx = Context(0)
    ctx.selftest()
    mont, std = {}, {}

    def enc(vals, table, fn):
        for v in set(vals) - table.keys():
            table[v] = fn(v)
        return b"".join(table[v] for v in vals)
    differ, ran, t0 = [], 0, time.time()
    for group in (1, 2):
        psz = 64 * group
        for registered in (False, True):
            plans = {}
            for pic, g, (scalars, logs, infs) in mp.cases(knobs, families, registered, group == 1):
                n = len(scalars)
                pts = bytearray(orc.fixed_base(group, enc(logs, mont, o.fr_to_mont_bytes)))
                for j in infs:
                    pts[psz * j: psz * (j + 1)] = bytes(psz)
                pts = bytes(pts)
                forms = [(enc(scalars, mont, o.fr_to_mont_bytes), True)]
                if pic.std:
                    forms.append((enc(scalars, std, o.fr_to_std_bytes), False))
                want = I.expected_from_logs(group, scalars, logs)
                if n <= 64:
                    assert want == orc.msm_naive(group, forms[0][0], pts), pic.name
                if registered:
                    h = ctx.register_points(group, pts, n)
                    try:
                        c, ntab = h.info()        # the geometry the CPU test assumed is the one that runs
                        assert (c, ntab) == (g.c, g.mtab * g.nwin), (pic.name, c, ntab, g.describe())
                        got = [ctx.msm_points(h, sb, mont=m) for sb, m in forms]
                    finally:
                        h.release()
                else:
                    got = [ctx.msm(group, sb, pts, n, mont=m) for sb, m in forms]
                for (sb, m), res in zip(forms, got):
                    ran += 1
                    if res != want:
                        differ.append((pic.name, group, registered, "mont" if m else "std", g.describe()))
                plans.setdefault(tuple(g.describe().items()), []).append(n)
            for plan, ns in plans.items():
                print(f"plan G{group} {'registered' if registered else 'one-shot'} {dict(plan)} pictures={len(ns)} "
                      f"max_n={max(ns)}")
    ctx.close()
    print(f"{ran} MSMs in {time.time() - t0:.1f} s")
    if differ:
        print("FIRST DIFFERING PICTURE:", differ[0])
        for d in differ[1:]:
            print("also differs:", d)
        sys.exit(1)
    print("tail edges ok")


@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize("index", range(len(mp.KNOB_SETS)), ids=[mp.knob_id(k) for k, _ in mp.KNOB_SETS])
def test_tail_kernels_at_exceptional_bucket_pictures(index):
    env = {k: v for k, v in os.environ.items() if not k.startswith("G16_")}
    env.update(mp.KNOB_SETS[index][0])
    t0 = time.time()
    r = subprocess.run([sys.executable, "-m", "tests.test_gpu_msm_tail_edges", str(index)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=800)
    print(r.stdout[-4000:], f"case took {time.time() - t0:.1f} s")
    assert r.returncode == 0 and "tail edges ok" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


if __name__ == "__main__":
    child(int(sys.argv[1]))
