"""`g16prove --audit-key` and `prove_files.py --audit`: the audit runs before the key is loaded; a clean key proves, a
key with one pointsB2 entry outside the order-r subgroup is named, refused with a non-zero exit code, and leaves no
proof behind.  The key is the hand-built snarkjs-layout file of tests/snarkjs_layout.py."""
import os
import subprocess
import sys

import pytest

from oracle import bn254_ref as o
from tests import key_audit_pictures as KA

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """(clean .zkey, the same file with pointsB2[i] replaced by the point of order 10069, .wtns, i)"""
    from tests.test_files_cpu import _snarkjs_like
    tmp = tmp_path_factory.mktemp("audit_cli")
    zpath, wpath, oz, _, _ = _snarkjs_like(tmp)
    i = max(k for k, q in enumerate(oz.pointsB2) if not o.G2.is_inf(q))
    raw = open(zpath, "rb").read()
    old, new = o.g2_to_bytes(oz.pointsB2[i]), o.g2_to_bytes(KA.twist_outsiders()["small"])
    assert raw.count(old) == 1
    bad = str(tmp / "small_order_b2.zkey")
    open(bad, "wb").write(raw.replace(old, new))
    return zpath, bad, wpath, i, tmp


def test_native_cli_audits_before_it_proves(ctx, files):
    from tests.test_gpu_native_cli import _build
    zpath, bad, wpath, i, tmp = files
    exe = _build(tmp)
    proof, public = str(tmp / "proof.json"), str(tmp / "public.json")
    out = subprocess.run([exe, "-z", zpath, "-w", wpath, "-o", proof, "-i", public, "-n", "-y", "--audit-key"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    assert "key audit: ok" in out.stdout and "verification succeeded" in out.stdout
    assert out.stdout.index("key audit: ok") < out.stdout.index("verification succeeded")
    plain = subprocess.run([exe, "-z", zpath, "-w", wpath, "-o", str(tmp / "proof0.json"), "-i", public, "-n"],
                           capture_output=True, text=True, timeout=600)
    assert plain.returncode == 0 and "key audit" not in plain.stdout
    assert open(proof).read() == open(tmp / "proof0.json").read()          # the audit changes nothing about the proof
    proof2 = str(tmp / "proof_bad.json")
    out = subprocess.run([exe, "-z", bad, "-w", wpath, "-o", proof2, "-i", str(tmp / "public_bad.json"), "-n", "-y",
                          "--audit-key"], capture_output=True, text=True, timeout=600)
    assert out.returncode != 0
    assert "key audit: FAILED" in out.stdout and f"pointsB2[{i}] is not in the order-r subgroup" in out.stdout
    assert not os.path.exists(proof2) and not os.path.exists(tmp / "public_bad.json")


def test_python_cli_audits_before_it_proves(ctx, files):
    zpath, bad, wpath, i, tmp = files
    tool = os.path.join(ROOT, "tools", "prove_files.py")
    proof = str(tmp / "py_proof.json")
    out = subprocess.run([sys.executable, tool, "-z", zpath, "-w", wpath, "-o", proof, "-i", str(tmp / "py_public.json"),
                          "-n", "-y", "--audit"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    assert "key audit: ok" in out.stdout and "verification succeeded" in out.stdout and os.path.exists(proof)
    proof2 = str(tmp / "py_proof_bad.json")
    out = subprocess.run([sys.executable, tool, "-z", bad, "-w", wpath, "-o", proof2, "-i", str(tmp / "py_public_bad.json"),
                          "-n", "--audit"], capture_output=True, text=True, timeout=600)
    assert out.returncode != 0
    assert "key audit: FAILED" in out.stdout and f"pointsB2[{i}] is not in the order-r subgroup" in out.stdout
    assert not os.path.exists(proof2)
