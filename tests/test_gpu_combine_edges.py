"""A proof's last step on the GPU at exceptional pictures (tests/combine_pictures.py): prove_combine_kernel behind
g16_prove_combine and sum_partials_kernel behind g16_g1_sum_partials / g16_g2_sum_partials on crafted XYZZ records --
infinities anywhere in the list, equal and opposite records, a running sum that returns to infinity and goes on, the ABI's
maximum counts, records scaled by (l^2, l^3) -- and the host mask algebra behind them at masks and sums that make its
additions meet equal, opposite and infinite operands.  Every expected proof is the closed form on integers mod r times
the generator (the C oracle's fixed-base multiplier); what each picture reaches is asserted on the CPU in
tests/test_host_algebra_cpu.py.  H and C enter pi_c symmetrically: an exchange of those two slots is not claimed."""
import time

import pytest

from oracle import bn254_ref as o
from tests import combine_pictures as cp
from tests.test_host_algebra_cpu import Points

pytestmark = pytest.mark.gpu
R = o.R


def _mb(x):
    return o.fr_to_mont_bytes(x) if x % R else None      # None: the trivial mask's NULL pointer


@pytest.fixture(scope="module")
def pts(orc):
    return Points(orc)


@pytest.fixture(scope="module")
def toy(ctx, pts):
    """the toy key under the known toxic waste (fakeCircuitSetup), resident"""
    from nim_groth16_amd import loadProvingKey
    from nim_groth16_amd.fake_setup import R1CS, ToxicWaste, fakeCircuitSetup
    zk = fakeCircuitSetup(R1CS(8, 1, 1, 3, o.toy_r1cs().constraints), ToxicWaste(*cp.TOXIC), 1, ctx)
    sp = zk.specPoints
    assert (sp.alpha1, sp.beta1, sp.delta1) == tuple(pts.b(1, k) for k in (cp.ALPHA, cp.BETA, cp.DELTA))
    assert (sp.beta2, sp.delta2) == (pts.b(2, cp.BETA), pts.b(2, cp.DELTA))
    pk = loadProvingKey(zk, ctx)
    yield zk, pk
    pk.destroy()


def _proof(pts, logs):
    return pts.b(1, logs[0]), pts.b(2, logs[1]), pts.b(1, logs[2])


def _need(pts, slot_logs, expected):
    """every point of a test from two calls of the oracle's multiplier: [{slot: logs}], [(log pi_a, pi_b, pi_c)]"""
    by_group = {1: [e[0] for e in expected] + [e[2] for e in expected], 2: [e[1] for e in expected]}
    for logs in slot_logs:
        for slot, ks in logs.items():
            by_group[cp.SLOT_GROUP[slot]] += ks
    pts.need(1, by_group[1])
    pts.need(2, by_group[2])


@pytest.mark.parametrize("count", cp.COMBINE_COUNTS)
def test_combine_list_pictures(toy, pts, count):
    """every list picture in all five slots at once (each slot its own logs), and one picture per slot rotated; records
    with ZZ = ZZZ = 1, with random and with edge scalings; a generic and the trivial mask"""
    _, pk = toy
    names = [name for name, _ in cp.list_pictures(count)]
    cases = [(name, cp.record_logs(count, name)) for name in names]
    cases += [("mixed%d" % i, cp.record_logs(count, cp.mixed_names(count, i))) for i in range(len(names))]
    modes = cp.LAMBDA_MODES if count <= 8 else None          # large counts: one scaling per picture, rotated
    jobs = []
    for i, (name, logs) in enumerate(cases):
        sums = tuple(sum(logs[slot]) % R for slot in cp.SLOTS)
        for j, mode in enumerate(modes or (cp.LAMBDA_MODES[i % 3],)):
            r, s = (cp.R0, cp.S0) if (i + j) % 2 == 0 else (0, 0)
            jobs.append((name, mode, logs, r, s, cp.expected_logs(r, s, *sums)))
    _need(pts, [logs for _, logs in cases], [j[5] for j in jobs])
    t_gpu, slowest = 0.0, (0.0, None)
    for name, mode, logs, r, s, want in jobs:
        rec = cp.build_records(logs, mode, pts.aff)
        assert len(rec) == cp.RECORD_BYTES * count
        t0 = time.perf_counter()
        got = pk.prove_combine(rec, count, _mb(r), _mb(s))
        dt = time.perf_counter() - t0
        t_gpu, slowest = t_gpu + dt, max(slowest, (dt, name))
        assert got == _proof(pts, want), (count, name, mode, "trivial mask" if r == 0 else "generic mask")
    print(f"count {count}: {len(jobs)} combines, {t_gpu:.3f} s in g16_prove_combine, slowest {slowest[0] * 1e3:.1f} ms ({slowest[1]})")


def test_combine_mask_pictures(toy, pts):
    """every mask and point picture: the sums in one record (ZZ = 1), and split over two scaled records"""
    _, pk = toy
    pics = cp.mask_pictures()
    g = o.SplitMix64(0x5b117)
    jobs = []
    for p in pics:
        part = tuple(g.fr() for _ in range(5))
        one = {slot: [x] for slot, x in zip(cp.SLOTS, p.sums)}
        two = {slot: [(x - m) % R, m] for slot, x, m in zip(cp.SLOTS, p.sums, part)}
        jobs += [(p, one, "unit"), (p, two, "random")]
    _need(pts, [logs for _, logs, _ in jobs], [p.expected() for p in pics])
    for p, logs, mode in jobs:
        n = len(logs["a"])
        got = pk.prove_combine(cp.build_records(logs, mode, pts.aff), n, _mb(p.r), _mb(p.s))
        assert got == _proof(pts, p.expected()), (p.name, n)


def test_combine_count_limits_and_device_records(toy, pts):
    import torch
    from nim_groth16_amd._lib import G16_EINVAL, G16Error
    _, pk = toy
    logs = cp.record_logs(3, cp.mixed_names(3, 1))
    sums = tuple(sum(logs[slot]) % R for slot in cp.SLOTS)
    want = cp.expected_logs(cp.R0, cp.S0, *sums)
    _need(pts, [logs], [want])
    rec = cp.build_records(logs, "random", pts.aff)
    for bad in (0, 1025):
        with pytest.raises(G16Error) as e:
            pk.prove_combine(rec * 342, bad, _mb(cp.R0), _mb(cp.S0))       # (1026 records are there to be read)
        assert e.value.code == G16_EINVAL, bad
    dev = torch.frombuffer(bytearray(rec), dtype=torch.uint8).to("cuda")
    torch.cuda.synchronize()
    assert pk.prove_combine(dev.data_ptr(), 3, _mb(cp.R0), _mb(cp.S0), device=True) == _proof(pts, want)
    assert pk.prove_combine(rec, 3, _mb(cp.R0), _mb(cp.S0)) == _proof(pts, want)


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("count", cp.SUM_COUNTS)
def test_sum_partials_list_pictures(ctx, pts, group, count):
    from nim_groth16_amd._lib import G16_EINVAL, G16Error
    psz = 64 * group
    if count == 0:
        assert ctx.sum_partials(group, b"", 0) == bytes(psz)
        with pytest.raises(G16Error) as e:
            ctx.sum_partials(group, bytes(2 * psz * 4097), 4097)
        assert e.value.code == G16_EINVAL
        return
    k, m = cp.slot_seeds("b2" if group == 2 else "b1")
    cases = [(name, build(count, k, m)) for name, build in cp.list_pictures(count)]
    pts.need(group, [x for _, logs in cases for x in logs + [sum(logs)]])
    t_gpu, slowest = 0.0, (0.0, None)
    for i, (name, logs) in enumerate(cases):
        for mode in (cp.LAMBDA_MODES if count <= 3 else (cp.LAMBDA_MODES[i % 3],)):
            rec = b"".join(cp.xyzz_bytes(group, pts.aff(group, x), cp.lam_of(mode, group, j)) for j, x in enumerate(logs))
            t0 = time.perf_counter()
            got = ctx.sum_partials(group, rec, count)
            dt = time.perf_counter() - t0
            t_gpu, slowest = t_gpu + dt, max(slowest, (dt, name))
            assert got == pts.b(group, sum(logs)), (group, count, name, mode)
    print(f"G{group} count {count}: {t_gpu:.3f} s in sum_partials, slowest {slowest[0] * 1e3:.1f} ms ({slowest[1]})")


def test_mask_pictures_through_prove_and_the_pool(toy, pts):
    """the mask pictures through the paths users call: g16_prove and a depth-1 prover pool on the toy witness.  The five
    MSM sums are the oracle prover's (combine_pictures.toy_sum_logs); the pictures that need a relation between a sum
    and the mask solve for the mask."""
    from nim_groth16_amd import ProverPool
    _, pk = toy
    wb = b"".join(o.fr_to_mont_bytes(w) for w in o.TOY_WITNESS)
    pics = cp.mask_pictures(cp.toy_sum_logs())
    _need(pts, [], [p.expected() for p in pics])
    for p in pics:
        assert pk.prove(wb, r=_mb(p.r), s=_mb(p.s)) == _proof(pts, p.expected()), p.name
    pool = ProverPool(pk, depth=1)
    try:
        for p in pics:
            t = pool.submit(wb, r=_mb(p.r), s=_mb(p.s))
            assert pool.collect(t) == _proof(pts, p.expected()), p.name
    finally:
        pool.close()
