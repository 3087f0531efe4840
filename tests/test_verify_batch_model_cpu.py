"""The expected verdicts of the batch-verifier tests need no GPU: for the two-to-three-proof form of every picture kind
of tests/verify_batch_pictures.py, the integer model's verdict equals the oracle's pairing product (its Miller loop and
final exponentiation) of the batch equation on the very points; and the C header, the ctypes mirror and the package
declare the entry point."""
import os
import re

import pytest

from tests import verify_batch_pictures as VB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("kind", VB.SCALAR_KINDS)
def test_model_verdict_is_the_oracle_pairing_product(kind):
    pic = VB.picture(kind, 2 if kind in ("same_twice", "opposite_C", "sum_zC_inf") else 3)
    assert pic.result == VB.EXPECTED.get(kind, 1)
    assert VB.oracle_result(pic) == pic.result
    if pic.result == 0:
        assert 0 in pic.statuses and set(pic.statuses) <= {0, 1}
    # the kinds are what their names say
    pts = pic.points()
    from oracle import bn254_ref as o
    if kind == "A_inf":
        assert pts[0][0] == o.INF_G1
    elif kind == "B_inf":
        assert pts[0][1] == o.INF_G2
    elif kind == "C_inf":
        assert pts[0][2] == o.INF_G1
    elif kind == "vk_x_inf":
        assert o.G1.msm_naive(pic.pubs[0], pic.model.ic) == o.INF_G1
    elif kind == "same_twice":
        assert pts[0] == pts[1] and pts[0][2] != o.INF_G1 and pic.multipliers[0] == pic.multipliers[1]
    elif kind == "opposite_C":
        assert pts[0][2] == o.G1.neg(pts[1][2]) != o.INF_G1 and pic.multipliers[0] == pic.multipliers[1]
    elif kind in ("cancel_equal", "cancel_wide", "cancel_pub", "cancel_a_c"):
        m = pic.model                                   # accepted although neither proof of the pair verifies alone
        assert m.defect(*pic.scalars[0]) and m.defect(*pic.scalars[1])


def test_cancelling_errors_need_all_128_bits_of_the_multiplier():
    """cancel_wide and cancel_wide_broken are the same proofs; the multipliers differ in bit 64 of z_1 alone"""
    a, b = VB.picture("cancel_wide", 3), VB.picture("cancel_wide_broken", 3, seed=VB.SCALAR_KINDS.index("cancel_wide"))
    assert a.scalars == b.scalars
    assert [x - y for x, y in zip(a.multipliers, b.multipliers)] == [1 << 64, 0, 0]
    assert (a.result, b.result) == (1, 0)


def test_entry_point_is_declared_everywhere():
    text = open(os.path.join(ROOT, "include", "g16hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"int32_t\s+g16_verify_batch\s*\(", code), "include/g16hip.h does not declare g16_verify_batch"
    from nim_groth16_amd import _lib
    assert "g16_verify_batch" in _lib.SYMBOLS
    assert hasattr(_lib.VerifyingKey, "verify_batch")
    import nim_groth16_amd
    assert callable(nim_groth16_amd.verifyProofsBatch)
    for doc in ("INTEGRATION.md", os.path.join("bindings", "nim", "g16hip.nim")):
        assert "verifyProofsBatch*" in open(os.path.join(ROOT, doc)).read(), doc
