"""Every op of tests/kernels/devops.inc on the GPU, in every arithmetic configuration the product is built in
(libg16devops.so: tests/kernels/devops.hip compiled once per configuration with the flags of the product objects), over
the operand set of tests/device_ops.py: canonical edge values, lazily reduced operands at the bounds
tools/ff29_model.py proves, crafted zero tests, curve sequences with every exceptional case, signed-digit recoding with
carries through every window, the Fp12 tower / Miller loop / final exponentiation of pairing.cuh over subfield and
edge elements, points at infinity, edge coordinates and twist points outside the order-r subgroup (in the two
configurations pairing.o is built in).  Bit for bit against plain Python integers.  tests/test_device_ops_cpu.py runs
the same vectors through the g++ build first.  One kernel launch per case."""
import ctypes
import glob
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import device_ops as D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nim_groth16_amd", "csrc")


@pytest.fixture(scope="module")
def oplib():
    so = os.path.join(CSRC, "libg16devops.so")
    deps = glob.glob(os.path.join(ROOT, "tests", "kernels", "devops.*")) + glob.glob(os.path.join(CSRC, "*.cuh")) + \
        glob.glob(os.path.join(CSRC, "*.inc")) + glob.glob(os.path.join(CSRC, "*.hpp")) + [os.path.join(CSRC, "Makefile")]
    stale = not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps)
    hipcc = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
    if stale and hipcc:
        subprocess.check_call(["make", "-C", CSRC, "-j", "5", "libg16devops.so", "HIPCC=" + hipcc])
    assert os.path.exists(so), so + " is missing: build it with `make -C nim_groth16_amd/csrc libg16devops.so`"
    lib = ctypes.CDLL(so)
    lib.devops_variant_name.restype = ctypes.c_char_p
    assert lib.devops_nvariants() == len(D.VARIANTS)
    assert [lib.devops_variant_name(v).decode() for v in range(len(D.VARIANTS))] == list(D.VARIANTS)
    return D.OpLibrary(lib, lib.devops_run)


def test_op_table_is_complete(oplib):
    """every build knows the whole table, and carries exactly the ops device_ops.py says it does: the pairing ops only
    where pairing.o is built that way; an op a build does not carry is an error there, not an empty result"""
    assert sorted(oplib.ops) == sorted(D.DEVICE_OPS)
    for v, name in enumerate(D.VARIANTS):
        carried = [op for op, (num, _, _) in oplib.ops.items() if oplib.lib.devops_carries(v, num) == 1]
        assert sorted(carried) == sorted(D.variant_ops(name)), name
        for op in set(D.DEVICE_OPS) - set(carried):
            with pytest.raises(AssertionError, match="returned error -2"):
                oplib.run(op, np.zeros((1, oplib.ops[op][1]), dtype=np.uint32), v)
    assert set(D.variant_ops("plain")) == set(D.variant_ops("calls")) == set(D.DEVICE_OPS)


CASES = [(v, op) for op in D.DEVICE_OPS for v, name in enumerate(D.VARIANTS) if op in D.variant_ops(name)]


@pytest.mark.parametrize("variant,op", CASES, ids=["%s-%s" % (D.VARIANTS[v], op) for v, op in CASES])
def test_device_op(oplib, variant, op):
    D.check_op(oplib, op, "variant " + D.VARIANTS[variant], variant)
