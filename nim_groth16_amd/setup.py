"""Real circuit setup: the proving key of `snarkjs zkey new circuit.r1cs pot.ptau`, on the GPU (g16_circuit_setup,
include/g16hip.h).  No toxic waste is needed: the Lagrange form of the ceremony's powers of tau is an inverse NTT whose
elements are curve points, and every point array of the key is a sparse matrix of the R1CS applied to such a vector.

gamma is always 1, and so is delta unless the caller supplies one: the key of `snarkjs zkey new`, which is sound only
after a phase-2 contribution.  For the same (tau, alpha, beta) it is fakeCircuitSetup's key with gamma = 1, byte for byte,
and it passes files.zkey.auditCircuit against the same r1cs and ptau."""
from __future__ import annotations

from . import bn128 as F
from ._lib import default_context
from .fake_setup import r1csToCoeffArray, r1csToCoeffs
from .zkey_types import GrothHeader, ProverPoints, Snarkjs, SpecPoints, ZKey


def circuitSetup(r1cs, ptau, flavour=Snarkjs, delta: int = None, ctx=None) -> ZKey:
    """r1cs: the list form of files/r1cs.py (fake_setup.R1CS) or a synthetic.SparseR1CS, as for fakeCircuitSetup; ptau: a
    files.ptau.Ptau with power >= log2 of the key's domain + 1; delta: None (= 1) or an integer in [1, r)."""
    from .files.zkey import ptauDesc, r1csDesc
    ctx = ctx or default_context()
    rd, rkeep = r1csDesc(r1cs, flavour)
    pd, pkeep = ptauDesc(ptau)
    if delta is not None and not 0 <= delta < F.primeR:
        raise ValueError("delta must lie in [1, r)")
    logDom, pts = ctx.circuit_setup(rd, pd, None if delta is None else F.frToMontBytes(delta))
    del rkeep, pkeep
    zkey = ZKey()
    zkey.header = GrothHeader("bn128", flavour, rd.nvars, rd.npubs, 1 << logDom, logDom)
    zkey.specPoints = SpecPoints(**{k: pts[k] for k in ("alpha1", "beta1", "delta1", "beta2", "gamma2", "delta2")})
    zkey.pointsIC = pts["pointsIC"]
    zkey.pPoints = ProverPoints(**{k: pts[k] for k in ("pointsA1", "pointsB1", "pointsB2", "pointsC1", "pointsH1")})
    zkey.coeffs = r1csToCoeffArray(r1cs) if hasattr(r1cs, "values") else r1csToCoeffs(r1cs)
    return zkey
