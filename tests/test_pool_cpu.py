"""No-GPU checks of the prover pool's boundary (include/g16hip.h "prover pool"): the busy code is declared on both
sides, the Python class is exported, argument errors come back before any device work, and pinned host memory has no
CPU fallback."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _library_built():
    """the shared library is a build artefact (git-ignored): build it when the tree is fresh"""
    from nim_groth16_amd._lib import lib_path
    if not os.path.exists(lib_path()):
        import subprocess
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "nim_groth16_amd", "csrc"), "-j", "8"])


def test_ebusy_declared_in_header_and_binding():
    text = open(os.path.join(ROOT, "include", "g16hip.h")).read()
    assert re.search(r"^#define G16_EBUSY \(-6\)", text, flags=re.M)
    from nim_groth16_amd import _lib
    assert _lib.G16_EBUSY == -6
    assert len({_lib.G16_OK, _lib.G16_EINVAL, _lib.G16_ENODEV, _lib.G16_EHIP, _lib.G16_ENOMEM, _lib.G16_ESELFTEST,
                _lib.G16_EBUSY}) == 7


def test_prover_pool_exported():
    import nim_groth16_amd
    from nim_groth16_amd._lib import HostBuffer, ProverPool
    assert nim_groth16_amd.ProverPool is ProverPool
    assert nim_groth16_amd.HostBuffer is HostBuffer
    for m in ("submit", "poll", "collect", "close"):
        assert callable(getattr(ProverPool, m))


def test_prover_create_without_key_is_einval_and_leaves_null():
    from nim_groth16_amd._lib import G16_EINVAL, load_library
    lib = load_library()
    p = ctypes.c_void_p(0x1234)                       # must be overwritten with NULL
    assert lib.g16_prover_create(0, None, 3, ctypes.byref(p)) == G16_EINVAL
    assert p.value is None
    assert lib.g16_prover_create(0, None, 3, None) == G16_EINVAL
    # a NULL pool is refused by every call, never dereferenced
    t = ctypes.c_uint64()
    assert lib.g16_prover_submit(None, None, 0, None, None, ctypes.byref(t)) == G16_EINVAL
    assert lib.g16_prover_poll(None, 1) == G16_EINVAL
    assert lib.g16_prover_collect(None, 1, None) == G16_EINVAL
    lib.g16_prover_destroy(None)
    lib.g16_host_free(None)
    assert lib.g16_prover_last_error(None)


def test_host_alloc_has_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from nim_groth16_amd._lib import G16_ENODEV, G16Error, HostBuffer, load_library
    lib = load_library()
    p = ctypes.c_void_p(0x1234)
    assert lib.g16_host_alloc(0, 4096, ctypes.byref(p)) == G16_ENODEV
    assert p.value is None
    with pytest.raises(G16Error) as e:
        HostBuffer(4096)
    assert e.value.code == G16_ENODEV
