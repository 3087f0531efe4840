"""Every op of tests/kernels/devops.inc over its full operand set (tests/device_ops.py), through the g++ build of the
device headers: the portable branches, on a machine without a GPU.  This is the proof that the operand vectors and the
Python references are themselves right before a GPU sees them (tests/test_gpu_device_ops.py runs the same vectors
through the inline-asm / builtin branches), and that every vector handed to Field::inv makes its loop end."""
import ctypes
import glob
import os
import subprocess

import pytest

from tests import device_ops as D

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpu_kernels")
ROOT = os.path.dirname(os.path.dirname(HERE))


@pytest.fixture(scope="module")
def oplib():
    so = os.path.join(HERE, "libdevops_shim.so")
    src = os.path.join(HERE, "devops_shim.cpp")
    csrc = os.path.join(ROOT, "nim_groth16_amd", "csrc")
    deps = [src, os.path.join(ROOT, "tests", "kernels", "devops.inc")] + glob.glob(os.path.join(csrc, "*.cuh")) + \
        glob.glob(os.path.join(csrc, "*.inc"))
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", src, "-o", so])   # takes minutes
    lib = ctypes.CDLL(so)
    return D.OpLibrary(lib, lambda variant, op, inp, n, out: lib.devops_host_run(op, inp, n, out))


def test_op_table_is_complete(oplib):
    """the g++ build holds exactly the ops the generator knows (msm_digits needs msm.cuh: device only)"""
    assert sorted(oplib.ops) == sorted(D.HOST_OPS)


@pytest.mark.parametrize("op", D.HOST_OPS)
def test_device_op_on_cpu(oplib, op):
    n = D.check_op(oplib, op, "g++ build")
    assert n % 64 != 0      # the GPU launch of these vectors ends in a partial block
