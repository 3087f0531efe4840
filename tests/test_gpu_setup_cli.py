"""tools/g16prove.cpp -u -r circuit.r1cs: the reference CLI's fake setup (cli/cli_main.nim:184-193) in the native tool --
the .r1cs reader of tools/g16_files.hpp, g16_fake_setup, the proof and its verification in one process with no .zkey.
Its proof.json and public.json must equal what the Python path writes for the same files, the same toxic waste and the
trivial mask."""
import subprocess

import pytest

from oracle import bn254_ref as o
from tests.test_gpu_native_cli import _build

pytestmark = pytest.mark.gpu
SEED = 7


def _toxic_from_seed(seed):
    """--toxic-seed: five 256-bit draws of SplitMix64(seed), least significant word first, top three bits cleared"""
    from nim_groth16_amd.synthetic import SplitMix64
    rng = SplitMix64(seed)
    return [sum(rng.next() << (64 * i) for i in range(4)) & ((1 << 253) - 1) for _ in range(5)]


@pytest.mark.parametrize("circuit", ["toy", "chain8"])
def test_setup_prove_verify_without_a_zkey(ctx, tmp_path, circuit):
    from nim_groth16_amd import generateProofWithTrivialMask
    from nim_groth16_amd.fake_setup import R1CS, ToxicWaste, fakeCircuitSetup
    from nim_groth16_amd.files import exportProof, exportPublicIO, parseWitness, writeWitness
    from nim_groth16_amd.files.r1cs import writeR1CS
    from nim_groth16_amd.synthetic import squaringChain
    if circuit == "toy":
        r1cs, wit = R1CS(8, 1, 1, 3, o.toy_r1cs().constraints), o.TOY_WITNESS
    else:
        r1cs, wit = squaringChain((1 << 8) - 2, seed=4)
        r1cs = R1CS(r1cs.nWires, r1cs.nPubOut, r1cs.nPubIn, r1cs.nPrivIn, r1cs.constraints)
    rpath, wpath = str(tmp_path / "c.r1cs"), str(tmp_path / "c.wtns")
    writeR1CS(rpath, r1cs)
    writeWitness(wpath, wit)
    tox = _toxic_from_seed(SEED)
    assert all(0 < t < o.R for t in tox)
    # the Python path: the same setup through fakeCircuitSetup, then the host mirror's prover and exporters
    zk = fakeCircuitSetup(r1cs, ToxicWaste(*tox), 1, ctx, scalarSide="device")
    pr = generateProofWithTrivialMask(0, False, zk, parseWitness(wpath), ctx)
    exportProof(str(tmp_path / "py_proof.json"), pr)
    exportPublicIO(str(tmp_path / "py_public.json"), pr)
    exe = _build(tmp_path)
    out = subprocess.run([exe, "-u", "-r", rpath, "--toxic-seed", str(SEED), "-w", wpath, "-o", str(tmp_path / "proof.json"),
                          "-i", str(tmp_path / "public.json"), "-n", "-y"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "verification succeeded" in out.stdout, (out.stdout, out.stderr)
    assert open(tmp_path / "public.json").read() == open(tmp_path / "py_public.json").read()
    assert open(tmp_path / "proof.json").read() == open(tmp_path / "py_proof.json").read()
    if circuit == "toy":
        # with a random mask it still verifies; a damaged file and a missing -r are refused with a message
        out = subprocess.run([exe, "--setup", "--r1cs", rpath, "--toxic-seed", str(SEED), "-w", wpath, "-o",
                              str(tmp_path / "proof2.json"), "-i", str(tmp_path / "public2.json"), "-y"],
                             capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and "verification succeeded" in out.stdout, (out.stdout, out.stderr)
        bad = str(tmp_path / "bad.r1cs")
        open(bad, "wb").write(open(rpath, "rb").read()[:-9])
        out = subprocess.run([exe, "-u", "-r", bad, "-w", wpath], capture_output=True, text=True, timeout=600, cwd=tmp_path)
        assert out.returncode == 1 and "g16prove:" in out.stderr
        out = subprocess.run([exe, "-u", "-w", wpath], capture_output=True, text=True, timeout=600, cwd=tmp_path)
        assert out.returncode == 1 and "usage" in out.stderr
