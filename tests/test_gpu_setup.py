"""The fake trusted setup with its scalar side on the device (g16_fake_setup, g16_lagrange_fr, g16_powers_fr;
reference groth16/fake_setup.nim:201-326, math/poly.nim:242-250).  Field arithmetic is exact: every value is compared
for equality -- with the oracle's eval_lagrange_poly_at / fake_circuit_setup or a closed form, never with the code under
test -- and a key built on the device must be the bytes of the key built with the scalar side in Python integers."""
import ctypes

import numpy as np
import pytest

from oracle import bn254_ref as o
from tests import inputs as I

pytestmark = pytest.mark.gpu
R = o.R
M, B = 8, 256                 # elements per thread and threads per workgroup of the kernel (held by tests/test_setup_cpu.py)
COUNTS = (1, M - 1, M, M + 1, B * M - 1, B * M, B * M + 1)
POINTS = ("alpha1", "beta1", "delta1", "beta2", "gamma2", "delta2", "pointsIC", "pointsA1", "pointsB1", "pointsB2",
          "pointsC1", "pointsH1")


def mont(x):
    return o.fr_to_mont_bytes(x % R)


def ints(b):
    return [o.fr_from_mont_bytes(b[i:i + 32]) for i in range(0, len(b), 32)]


def omega(log2n):
    return pow(o.GEN28, 1 << (28 - log2n), R)


def still_usable(ctx):
    assert ints(ctx.powers(mont(3), 5)) == [1, 3, 9, 27, 81]


def einval(ctx, fn, *needles):
    from nim_groth16_amd._lib import G16Error
    with pytest.raises(G16Error) as e:
        fn()
    assert e.value.code == -1, e.value
    for needle in needles:
        assert needle in str(e.value), e.value
    still_usable(ctx)


TAU = o.SplitMix64(2024).fr()


@pytest.fixture(scope="module")
def lag13():
    """L_j(TAU) for every j of the 2^13 domain, from the oracle, computed once"""
    D = o.Domain(1 << 13)
    return [o.eval_lagrange_poly_at(D, j, TAU) for j in range(1 << 13)]


# ---- g16_lagrange_fr -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log2n", range(6))
def test_lagrange_every_index_of_the_small_domains(ctx, log2n):
    D = o.Domain(1 << log2n)
    got = ints(ctx.lagrange(log2n, mont(TAU)))
    assert got == [o.eval_lagrange_poly_at(D, j, TAU) for j in range(1 << log2n)]


@pytest.mark.parametrize("first,step", [(1, 2), (0, 1)])
def test_lagrange_counts_around_a_run_and_a_workgroup(ctx, lag13, first, step):
    for count in COUNTS:
        got = ints(ctx.lagrange(13, mont(TAU), first=first, step=step, count=count))
        assert got == [lag13[first + step * i] for i in range(count)], count


def test_lagrange_identities_at_2p16(ctx):
    """sum_j L_j(tau) = 1 and sum_j omega^j L_j(tau) = tau (the interpolation of 1 and of x)"""
    got = ints(ctx.lagrange(16, mont(TAU)))
    assert len(got) == 1 << 16
    assert sum(got) % R == 1
    w, acc, wj = omega(16), 0, 1
    for v in got:
        acc += wj * v
        wj = wj * w % R
    assert acc % R == TAU


def test_lagrange_tau_zero(ctx):
    for log2n in (0, 3, 9):
        assert ints(ctx.lagrange(log2n, mont(0))) == [pow(1 << log2n, -1, R)] * (1 << log2n)


def test_lagrange_tau_elsewhere_in_the_domain(ctx):
    """tau on the doubled domain at an even index while only odd indices are requested: every value is zero, no error"""
    tau = pow(omega(10), 2 * 77, R)
    assert ints(ctx.lagrange(10, mont(tau), first=1, step=2)) == [0] * 512


def test_lagrange_tau_inside_the_request(ctx):
    for log2n, first, step, count, j in [(10, 0, 1, 1024, 777), (10, 1, 2, 512, 2 * 300 + 1), (4, 3, 1, 5, 3), (4, 0, 1, 16, 15)]:
        tau = pow(omega(log2n), j, R)
        einval(ctx, lambda: ctx.lagrange(log2n, mont(tau), first=first, step=step, count=count),
               "tau lies in the domain", f"omega^{j} ")


def test_lagrange_scale(ctx, lag13):
    s = o.SplitMix64(9).fr()
    plain = ctx.lagrange(13, mont(TAU), first=5, step=3, count=100)
    assert plain == ctx.lagrange(13, mont(TAU), first=5, step=3, count=100, scale=mont(1))
    assert ints(plain) == [lag13[5 + 3 * i] for i in range(100)]
    assert ints(ctx.lagrange(13, mont(TAU), first=5, step=3, count=100, scale=mont(s))) == \
        [s * lag13[5 + 3 * i] % R for i in range(100)]


# ---- g16_powers_fr -------------------------------------------------------------------------------------------------------
def test_powers_against_pow(ctx):
    base, scale = o.SplitMix64(12).fr(), o.SplitMix64(13).fr()
    want = [1]
    for _ in range(B * M):
        want.append(want[-1] * base % R)
    for count in COUNTS:
        assert ints(ctx.powers(mont(base), count)) == want[:count], count
        assert ints(ctx.powers(mont(base), count, scale=mont(scale))) == [scale * v % R for v in want[:count]], count
    assert ctx.powers(mont(base), 0) == b""


def test_powers_base_zero_and_one(ctx):
    s = o.SplitMix64(14).fr()
    assert ints(ctx.powers(mont(0), 20, scale=mont(s))) == [s] + [0] * 19
    assert ints(ctx.powers(mont(1), 20, scale=mont(s))) == [s] * 20


# ---- g16_fake_setup against the oracle -------------------------------------------------------------------------------
def _matrices(constraints, std=False):
    """the list form (files/r1cs.nim:62-80) -> three (constraint, wire, values) triplet sets"""
    out = []
    for k in range(3):
        rows, wires, vals = [], [], []
        for i, con in enumerate(constraints):
            for (w, v) in con[k]:
                rows.append(i), wires.append(w), vals.append(v % R)
        enc = (lambda v: v.to_bytes(32, "little")) if std else mont
        out.append((np.array(rows, dtype=np.uint32), np.array(wires, dtype=np.uint32), b"".join(enc(v) for v in vals)))
    return out


def _device_setup(ctx, nwires, npubs, constraints, tox, flavour, std=False):
    enc = (lambda v: (v % R).to_bytes(32, "little")) if std else mont
    return ctx.fake_setup(nwires, npubs, len(constraints), flavour, _matrices(constraints, std), [enc(t) for t in tox],
                          mont=not std)


def _oracle_setup(orc, nwires, npubout, npubin, constraints, tox, flavour):
    """-> {name: bytes} from the oracle's transliteration of fake_setup.nim:201-326 (fixed-base by the C oracle)"""
    chunks = lambda b, k: [b[i:i + k] for i in range(0, len(b), k)]                                        # noqa: E731
    bg1 = lambda ks: [o.g1_from_bytes(x) for x in chunks(orc.fixed_base(1, I.fr_mont_bytes(ks)), 64)]      # noqa: E731
    bg2 = lambda ks: [o.g2_from_bytes(x) for x in chunks(orc.fixed_base(2, I.fr_mont_bytes(ks)), 128)]     # noqa: E731
    oz = o.fake_circuit_setup(o.R1CS(nwires, npubout, npubin, nwires - 1 - npubout - npubin, constraints),
                              o.ToxicWaste(*tox), o.SNARKJS if flavour else o.JENS_GROTH, bg1, bg2)
    out = {}
    for name in POINTS:
        v = getattr(oz, name)
        pts = v if name.startswith("points") else [v]
        out[name] = b"".join((o.g2_to_bytes if name.endswith("2") else o.g1_to_bytes)(p) for p in pts)
    return oz.logDomainSize, out


def _toxic(seed):
    rng = o.SplitMix64(seed)
    return [rng.fr() for _ in range(5)]


@pytest.mark.parametrize("flavour", [1, 0])
def test_fake_setup_toy_circuit(ctx, orc, flavour):
    cons, tox = o.toy_r1cs().constraints, _toxic(5)
    want_log, want = _oracle_setup(orc, 8, 1, 1, cons, tox, flavour)
    got_log, got = _device_setup(ctx, 8, 2, cons, tox, flavour)
    assert got_log == want_log == 3
    for name in POINTS:
        assert got[name] == want[name], name
    # standard-form values and toxic waste (G16_SCALARS_STD): the same key
    assert _device_setup(ctx, 8, 2, cons, tox, flavour, std=True) == (got_log, got)


@pytest.mark.parametrize("flavour", [1, 0])
def test_fake_setup_poseidon_2p10(ctx, orc, flavour):
    from nim_groth16_amd.synthetic import poseidonMerkle
    r1cs, _ = poseidonMerkle(10, seed=4)
    tox = _toxic(6)
    want_log, want = _oracle_setup(orc, r1cs.nWires, 1, 0, r1cs.constraints, tox, flavour)
    got_log, got = _device_setup(ctx, r1cs.nWires, 1, r1cs.constraints, tox, flavour)
    assert got_log == want_log == 10
    for name in POINTS:
        assert got[name] == want[name], name
    if flavour:
        assert _device_setup(ctx, r1cs.nWires, 1, r1cs.constraints, tox, flavour, std=True) == (got_log, got)


@pytest.mark.parametrize("ncons", [7, 8])
@pytest.mark.parametrize("flavour", [1, 0])
def test_fake_setup_hand_built_circuit(ctx, orc, flavour, ncons):
    """a repeated (constraint, wire) entry, a wire in no matrix (its points are (0,0)), an empty C matrix, npubs = 0, and
    n + p + 1 an exact power of two (7 constraints: domain 8) and one more than that (8 constraints: domain 16)"""
    rng = o.SplitMix64(40 + ncons)
    nwires = 9                                                # wire 8 appears nowhere
    cons = []
    for i in range(ncons):
        a = [(1 + i % 7, rng.fr()), (1 + (i + 3) % 7, rng.fr())]
        b = [(1 + (2 * i) % 7, rng.fr())]
        if i == 2:
            a = [(5, rng.fr()), (5, rng.fr()), (0, 1)]        # entries of one (constraint, wire) add up
            b = [(3, 2), (3, R - 5)]
        cons.append((a, b, []))
    tox = _toxic(50)
    want_log, want = _oracle_setup(orc, nwires, 0, 0, cons, tox, flavour)
    got_log, got = _device_setup(ctx, nwires, 0, cons, tox, flavour)
    assert got_log == want_log == (3 if ncons == 7 else 4)
    for name in POINTS:
        assert got[name] == want[name], name
    assert got["pointsA1"][64 * 8:] == bytes(64) and got["pointsB2"][128 * 8:] == bytes(128)
    assert got["pointsC1"][64 * 7:] == bytes(64) and len(got["pointsIC"]) == 64
    assert _device_setup(ctx, nwires, 0, cons, tox, flavour, std=True) == (got_log, got)


# ---- the device path of fakeCircuitSetup against the host path ---------------------------------------------------------
@pytest.mark.parametrize("flavour", [1, 0])
def test_device_path_equals_host_path_on_the_2p12_chain(ctx, flavour):
    from nim_groth16_amd import Mask, Witness, extractVKey, generateProofWithMask, loadProvingKey, verifyProof
    from nim_groth16_amd.fake_setup import ToxicWaste, fakeCircuitSetup
    from nim_groth16_amd.synthetic import squaringChain
    from nim_groth16_amd.zkey_types import packCoeffs
    r1cs, wit = squaringChain((1 << 12) - 2, seed=4)
    tox = ToxicWaste(*_toxic(7))
    host = fakeCircuitSetup(r1cs, tox, flavour, ctx, scalarSide="host")
    dev = fakeCircuitSetup(r1cs, tox, flavour, ctx, scalarSide="device")
    assert dev.header == host.header and dev.specPoints == host.specPoints and dev.pointsIC == host.pointsIC
    for name in ("pointsA1", "pointsB1", "pointsB2", "pointsC1", "pointsH1"):
        assert getattr(dev.pPoints, name) == getattr(host.pPoints, name), name
    assert packCoeffs(dev.coeffs) == packCoeffs(host.coeffs)
    with pytest.raises(ValueError):
        fakeCircuitSetup(r1cs, tox, flavour, ctx, scalarSide="gpu")
    pk = loadProvingKey(dev, ctx)
    try:
        rng = o.SplitMix64(8)
        pr = generateProofWithMask(0, False, dev, Witness("bn128", len(wit), I.fr_mont_bytes(wit)),
                                   Mask(rng.fr(), rng.fr()), ctx, pkey=pk)
        assert verifyProof(extractVKey(dev), pr, ctx)                      # g16_verify
    finally:
        pk.destroy()


def test_default_is_the_device_path(ctx):
    """with a Context and no scalarSide the setup is one g16_fake_setup call: its kernels show up in the profile"""
    from nim_groth16_amd.fake_setup import R1CS, ToxicWaste, fakeCircuitSetup
    r1cs, tox = R1CS(8, 1, 1, 3, o.toy_r1cs().constraints), ToxicWaste(*_toxic(5))
    ctx.profile(True)
    try:
        ctx.profile_reset()
        zk = fakeCircuitSetup(r1cs, tox, 1, ctx)
        kernels = ctx.profile_report()
    finally:
        ctx.profile(False)
    assert {"setup_lagrange", "setup_combine", "spmv", "fixed_base_mul"} <= set(kernels)
    assert kernels["setup_lagrange"]["calls"] == 2          # the domain, and the odd half of the doubled domain
    assert zk.pPoints == fakeCircuitSetup(r1cs, tox, 1, ctx, scalarSide="host").pPoints


def test_device_path_raises_the_reference_assert_for_tau_in_the_domain(ctx):
    from nim_groth16_amd.fake_setup import R1CS, ToxicWaste, fakeCircuitSetup
    a, b, g, d, _ = _toxic(9)
    r1cs = R1CS(8, 1, 1, 3, o.toy_r1cs().constraints)
    with pytest.raises(AssertionError, match="point should be outside the domain"):
        fakeCircuitSetup(r1cs, ToxicWaste(a, b, g, d, pow(omega(3), 5, R)), 1, ctx, scalarSide="device")
    still_usable(ctx)


# ---- every G16_EINVAL case, each leaving the context usable ----------------------------------------------------------------
def test_lagrange_and_powers_reject_bad_arguments(ctx):
    lib, h = ctx._lib, ctx._h
    out = ctypes.create_string_buffer(32 * 64)
    t = mont(TAU)
    einval(ctx, lambda: ctx._check(lib.g16_lagrange_fr(h, 4, 0, 1, 16, None, None, out)), "null pointer")
    einval(ctx, lambda: ctx._check(lib.g16_lagrange_fr(h, 4, 0, 1, 16, t, None, None)), "null pointer")
    einval(ctx, lambda: ctx._check(lib.g16_powers_fr(h, None, None, 4, out)), "null pointer")
    einval(ctx, lambda: ctx._check(lib.g16_powers_fr(h, t, None, 4, None)), "null pointer")
    einval(ctx, lambda: ctx.lagrange(29, t, count=1), "log2n")
    einval(ctx, lambda: ctx.lagrange(4, t, first=0, step=1, count=17), "outside the domain")
    einval(ctx, lambda: ctx.lagrange(4, t, first=1, step=2, count=9), "outside the domain")
    einval(ctx, lambda: ctx.lagrange(4, t, first=16, step=0, count=1), "outside the domain")
    einval(ctx, lambda: ctx.lagrange(28, t, first=0xffffffff, step=0xffffffff, count=3), "outside the domain")
    big = R.to_bytes(32, "little")                            # r itself: the smallest value that is not canonical
    einval(ctx, lambda: ctx.lagrange(4, big), "not canonical")
    einval(ctx, lambda: ctx.lagrange(4, t, scale=big), "not canonical")
    einval(ctx, lambda: ctx.powers(big, 4), "not canonical")
    einval(ctx, lambda: ctx.powers(t, 4, scale=bytes([255]) * 32), "not canonical")
    einval(ctx, lambda: ctx._check(lib.g16_powers_fr(h, t, None, (1 << 29) + 1, out)), "count too large")
    assert ctx.lagrange(4, t, count=0) == b""


def test_fake_setup_rejects_bad_arguments(ctx):
    from nim_groth16_amd._lib import SetupDesc, SetupPoints
    lib, h = ctx._lib, ctx._h
    cons, tox = o.toy_r1cs().constraints, _toxic(5)
    big = R.to_bytes(32, "little")

    def setup(nwires=8, npubs=2, constraints=cons, toxic=tox, flavour=1, mats=None, ncons=None):
        mats = mats or _matrices(constraints)
        return ctx.fake_setup(nwires, npubs, len(constraints) if ncons is None else ncons, flavour, mats,
                              [t if isinstance(t, bytes) else mont(t) for t in toxic])

    setup()                                                   # (the arguments every case below damages are fine)
    # null pointers
    einval(ctx, lambda: ctx._check(lib.g16_fake_setup(h, None, ctypes.byref(SetupPoints()))), "null pointer")
    einval(ctx, lambda: ctx._check(lib.g16_fake_setup(h, ctypes.byref(SetupDesc()), None)), "null pointer")
    d = SetupDesc()
    d.nvars, d.npubs, d.nconstraints, d.flavour, d.flags = 8, 2, 3, 1, 1
    einval(ctx, lambda: ctx._check(lib.g16_fake_setup(h, ctypes.byref(d), ctypes.byref(SetupPoints()))),
           "null toxic-waste pointer")
    keep = [ctypes.create_string_buffer(mont(t), 32) for t in tox]
    d.alpha, d.beta, d.gamma, d.delta, d.tau = (ctypes.addressof(k) for k in keep)
    einval(ctx, lambda: ctx._check(lib.g16_fake_setup(h, ctypes.byref(d), ctypes.byref(SetupPoints()))),
           "null output pointer")
    d.nnz[1] = 1
    einval(ctx, lambda: ctx._check(lib.g16_fake_setup(h, ctypes.byref(d), ctypes.byref(SetupPoints()))),
           "null matrix pointer")
    # entries out of range: a constraint index, a wire index
    for k, (what, where) in enumerate([("row", 3), ("col", 8), ("row", 0xffffffff)]):
        mats = _matrices(cons)
        rows, wires, vals = mats[2]
        (rows if what == "row" else wires)[1] = where
        einval(ctx, lambda: setup(mats=mats), "matrix 2 entry 1 out of range")
    # a value, and each toxic scalar, that is not canonical
    mats = _matrices(cons)
    mats[1] = (mats[1][0], mats[1][1], mats[1][2][:32] + big + mats[1][2][64:])
    einval(ctx, lambda: setup(mats=mats), "matrix 1 entry 1", "not canonical")
    for i in range(5):
        einval(ctx, lambda: setup(toxic=tox[:i] + [big] + tox[i + 1:]), "not canonical")
    # gamma or delta zero
    einval(ctx, lambda: setup(toxic=tox[:2] + [0] + tox[3:]), "gamma and delta")
    einval(ctx, lambda: setup(toxic=tox[:3] + [0] + tox[4:]), "gamma and delta")
    # shapes: no wire beyond the public ones, an unknown flavour, a domain above 2^28 (doubled for the snarkjs flavour)
    einval(ctx, lambda: setup(nwires=2, npubs=2, constraints=[]), "nvars must exceed npubs")
    einval(ctx, lambda: setup(flavour=2), "flavour")
    einval(ctx, lambda: setup(nwires=3, npubs=1, constraints=[], ncons=1 << 27, flavour=1), "domain too large")
    einval(ctx, lambda: setup(nwires=3, npubs=1, constraints=[], ncons=1 << 28, flavour=0), "domain too large")
    # tau in the domain that is evaluated: found by the kernel, reported after the run with the index
    einval(ctx, lambda: setup(toxic=tox[:4] + [pow(omega(3), 6, R)]), "tau lies in the domain", "omega^6 of the 2^3 domain")
    einval(ctx, lambda: setup(toxic=tox[:4] + [pow(omega(4), 11, R)]), "tau lies in the domain",
           "omega^11 of the 2^4 domain")
    setup(toxic=tox[:4] + [pow(omega(4), 11, R)], flavour=0)  # JensGroth never evaluates the doubled domain
    setup(toxic=tox[:4] + [0])                                # tau = 0 is outside every domain
