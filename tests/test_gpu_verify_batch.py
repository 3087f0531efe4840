"""g16_verify_batch on the GPU against the integer model of tests/verify_batch_pictures.py (held to the oracle's pairing
product in tests/test_verify_batch_model_cpu.py): batch sizes 1, 2, 64, 65, 131 cross every workgroup boundary of the
kernels (64 lanes; the Miller launch carries count + 3 lanes); errors that cancel under the multipliers show that the
kernels compute the equation with all 128 bits; exceptional points go through the complete additions of the trees."""
import dataclasses

import pytest

from oracle import bn254_ref as o
from tests import verify_batch_pictures as VB

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 64, 65, 131)


@pytest.fixture(scope="module")
def keys(ctx):
    """one device key per model (a model is a seed and a number of public inputs)"""
    cache = {}

    def get(pic):
        m = pic.model
        k = (m.alpha, m.npubs)
        if k not in cache:
            cache[k] = m.load(ctx)
        return cache[k]
    yield get
    for dev in cache.values():
        dev.destroy()


def _run(dev, pic, mont=True, compare_per_proof=True):
    pub = pic.public_io(mont)
    res, st = dev.verify_batch(pic.proofs, pub, mont=mont, multipliers=pic.multipliers, want_status=True)
    assert res == bool(pic.result), (res, pic.result)
    assert st == pic.statuses, [(j, s, e) for j, (s, e) in enumerate(zip(st, pic.statuses)) if s != e]
    assert dev.verify_batch(pic.proofs, pub, mont=mont, multipliers=pic.multipliers) == bool(pic.result)   # status NULL
    if compare_per_proof and not pic.result:
        assert st == dev.verify(pic.proofs, pub, mont=mont, subgroup=True)


@pytest.mark.parametrize("count", SIZES)
def test_all_valid(ctx, keys, count):
    pic = VB.picture("valid", count)
    assert {1, VB.Z_MAX, 1 << 127, 3} <= set(pic.multipliers) or count < 4
    dev = keys(pic)
    _run(dev, pic, mont=True)
    _run(dev, pic, mont=False)


@pytest.mark.parametrize("at", [0, 63, 64, 130])
def test_one_bad_proof(ctx, keys, at):
    pic = VB.picture("one_bad", 131, at=at)
    assert pic.statuses == [0 if j == at else 1 for j in range(131)]
    _run(keys(pic), pic)


@pytest.mark.parametrize("count,at", [(2, (0, 1)), (131, (63, 64))])
@pytest.mark.parametrize("kind", ["cancel_equal", "cancel_unequal", "cancel_wide", "cancel_wide_broken", "cancel_pub",
                                  "cancel_a_c"])
def test_errors_that_cancel(ctx, keys, kind, count, at):
    pic = VB.picture(kind, count, at=at)
    dev = keys(pic)
    _run(dev, pic, mont=True)
    if kind == "cancel_pub":
        _run(dev, pic, mont=False)
    if pic.result:      # accepted, although g16_verify rejects both proofs of the pair
        st = dev.verify([pic.proofs[j] for j in at], b"".join(pic.public_io(True)[96 * j:96 * j + 96] for j in at),
                        subgroup=True)
        assert st == [0, 0]


@pytest.mark.parametrize("kind,count,at", [
    ("A_inf", 3, 1), ("B_inf", 3, 1), ("C_inf", 3, 1), ("vk_x_inf", 3, 1), ("A_inf", 65, 64), ("B_inf", 65, 63),
    ("sum_zC_inf", 2, None), ("sum_zC_inf", 131, None), ("sum_sIC_inf", 2, None), ("sum_sIC_inf", 65, None),
    ("same_twice", 2, (0, 1)), ("same_twice", 131, (63, 64)), ("opposite_C", 2, (0, 1)), ("opposite_C", 131, (63, 64)),
    ("npubs_0", 1, None), ("npubs_0", 65, None)])
def test_exceptional_points(ctx, keys, kind, count, at):
    pic = VB.picture(kind, count, at=at)
    assert pic.result == 1
    dev = keys(pic)
    _run(dev, pic, mont=True)
    _run(dev, pic, mont=False)
    # ... and its neighbour, off by one in c of the last proof, is rejected
    a, b, c, pubs = pic.scalars[-1]
    bad = dataclasses.replace(pic, scalars=pic.scalars[:-1] + [(a, b, (c + 1) % o.R, pubs)], proofs=None, result=0,
                              statuses=[1] * (count - 1) + [0])
    assert not pic.model.accepts(bad.scalars, bad.multipliers)
    _run(dev, bad)


@pytest.mark.parametrize("kind", list(VB.STRUCTURAL))
def test_structural_defects(ctx, keys, kind):
    pic = VB.structural(kind, count=5, at=2)
    dev = keys(pic)
    _run(dev, pic)                       # no flag passed: a B of small order is refused all the same
    if kind == "small_order_b":
        pub = pic.public_io(True)
        assert dev.verify(pic.proofs, pub) == [1, 1, 0, 1, 1]          # g16_verify without the flag lets it in
    if kind != "noncanonical_pub":
        _run(dev, pic, mont=False)
    # the defect at the last lane of a workgroup and at the first of the next
    for at in (63, 64):
        big = VB.structural(kind, count=66, at=at)
        _run(keys(big), big, compare_per_proof=False)


def test_arguments(ctx, keys):
    import ctypes
    from nim_groth16_amd import Context, G16Error
    from nim_groth16_amd._lib import G16_EINVAL, _buf
    pic = VB.picture("valid", 8)
    dev = keys(pic)
    pub = pic.public_io(True)
    zs = list(pic.multipliers)
    zs[5] = 0
    with pytest.raises(G16Error, match=r"multiplier 5 is zero") as e:
        dev.verify_batch(pic.proofs, pub, multipliers=zs)
    assert e.value.code == G16_EINVAL
    lib, raw, res = ctx._lib, b"".join(a + b + c for a, b, c in pic.proofs), ctypes.c_int32(-7)
    assert lib.g16_verify_batch(ctx._h, dev._h, _buf(raw), _buf(pub), 1, 8, None, ctypes.byref(res), None) == G16_EINVAL
    zb = b"".join(z.to_bytes(16, "little") for z in pic.multipliers)
    assert lib.g16_verify_batch(ctx._h, dev._h, _buf(raw), _buf(pub), 1, 8, _buf(zb), None, None) == G16_EINVAL
    assert res.value == -7
    assert lib.g16_verify_batch(ctx._h, dev._h, None, None, 1, 0, None, ctypes.byref(res), None) == 0
    assert res.value == 1
    assert dev.verify_batch([], b"") is True
    assert dev.verify_batch([], b"", want_status=True) == (True, [])
    # a key of another context of the same device
    other = Context(0)
    try:
        key2 = pic.model.load(other)
        res = ctypes.c_int32(-7)
        assert lib.g16_verify_batch(ctx._h, key2._h, _buf(raw), _buf(pub), 1, 8, _buf(zb), ctypes.byref(res), None) == 0
        assert res.value == 1
        key2.destroy()
    finally:
        other.close()


@pytest.mark.parametrize("flavour", [0, 1])
def test_real_proofs(ctx, flavour):
    from nim_groth16_amd import extractVKey, loadVerifyingKey, verifyProofsBatch
    from tests.test_gpu_verifier import _toy
    zk, (good, other) = _toy(ctx, flavour)
    dev = loadVerifyingKey(extractVKey(zk), ctx)
    bad_c = dataclasses.replace(good, pi_c=other.pi_c)
    assert verifyProofsBatch(dev, [good, other], ctx, multipliers=[VB.Z_MAX, (1 << 127) + 5]) is True
    assert verifyProofsBatch(dev, [good, other, bad_c], ctx, multipliers=[VB.Z_MAX, (1 << 127) + 5, 7]) is False
    for _ in range(2):          # multipliers drawn afresh each time: the same verdicts
        assert verifyProofsBatch(dev, [good, other], ctx) is True
        assert verifyProofsBatch(dev, [good, other, bad_c], ctx) is False
    assert verifyProofsBatch(extractVKey(zk), [good, other], ctx) is True        # an unloaded key
    res, st = dev.verify_batch([(p.pi_a, p.pi_b, p.pi_c) for p in (good, bad_c, other)],
                               b"".join(p.publicIO for p in (good, bad_c, other)), want_status=True)
    assert (res, st) == (False, [1, 0, 1])
    dev.destroy()
