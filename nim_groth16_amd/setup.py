"""Real circuit setup: the proving key of `snarkjs zkey new circuit.r1cs pot.ptau`, on the GPU (g16_circuit_setup,
include/g16hip.h).  No toxic waste is needed: the Lagrange form of the ceremony's powers of tau is an inverse NTT whose
elements are curve points, and every point array of the key is a sparse matrix of the R1CS applied to such a vector.

gamma is always 1, and so is delta unless the caller supplies one: the key of `snarkjs zkey new`, which is sound only
after a phase-2 contribution: `contribute` below makes one (g16_key_contribute), `verifyContributions` checks a chain of
them against the key they started from (g16_contributions_verify); the transcript hashes are phase2.py's.  For the same (tau, alpha, beta) it is fakeCircuitSetup's key with gamma = 1, byte for byte,
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


def _phase2Part(zk: ZKey) -> dict:
    sp, pp = zk.specPoints, zk.pPoints
    return {"delta1": bytes(sp.delta1), "delta2": bytes(sp.delta2), "pointsC1": bytes(pp.pointsC1),
            "pointsH1": bytes(pp.pointsH1)}


def contribute(zkey: ZKey, d: int = None, s: int = None, name: str = "", ctx=None) -> ZKey:
    """One phase-2 contribution: delta -> d delta, pointsC1 and pointsH1 -> d^-1 times themselves, and a record in the
    key's contribution log (a fresh log, hashed from `zkey`, if it has none).  d: the secret, s: the secret of the proof
    of knowledge, integers in [1, r); None draws them with `secrets`.  Both are toxic waste: forget them.  The input key
    is not changed.  The challenge follows phase2.py's rule, not snarkjs's (see there)."""
    import copy
    import secrets

    from . import phase2
    ctx = ctx or default_context()
    d = secrets.randbelow(F.primeR - 1) + 1 if d is None else d
    s = secrets.randbelow(F.primeR - 1) + 1 if s is None else s
    if not (0 < d < F.primeR and 0 < s < F.primeR):
        raise ValueError("d and s must lie in [1, r)")
    log = copy.deepcopy(zkey.contributions) if zkey.contributions is not None else \
        phase2.Contributions(cs_hash=phase2.cs_hash(zkey))
    pok = ctx.fixed_base(1, F.frSeqToMontBytes([s, d * s % F.primeR]))
    transcript = phase2.transcript_hash(log, len(log.records), pok[:64], pok[64:])
    part, record = ctx.key_contribute(_phase2Part(zkey), F.frToMontBytes(d), F.frToMontBytes(s),
                                      phase2.challenge_bytes(transcript))
    assert record[64:192] == pok, "the record's proof-of-knowledge points are not the hashed ones"
    log.records.append(record)
    log.transcripts.append(transcript)
    log.names.append(name)
    out = ZKey()
    out.header, out.pointsIC, out.coeffs, out.coeffsSection4 = zkey.header, zkey.pointsIC, zkey.coeffs, zkey.coeffsSection4
    sp, pp = zkey.specPoints, zkey.pPoints
    out.specPoints = SpecPoints(alpha1=sp.alpha1, beta1=sp.beta1, delta1=part["delta1"], beta2=sp.beta2, gamma2=sp.gamma2,
                                delta2=part["delta2"])
    out.pPoints = ProverPoints(pointsA1=pp.pointsA1, pointsB1=pp.pointsB1, pointsB2=pp.pointsB2, pointsC1=part["pointsC1"],
                               pointsH1=part["pointsH1"])
    out.contributions = log
    return out


def verifyContributions(initial: ZKey, zkey: ZKey, multipliers=None, ctx=None):
    """Do the records of zkey.contributions lead from `initial` to `zkey`?  `initial` is the anchor: the key before any
    contribution, which the caller made with circuitSetup or tied to its circuit with files.zkey.auditCircuit.  The parts
    of the key no contribution touches must be the same bytes (ValueError otherwise).  -> _lib.ChainReport: `.ok`, str()
    names every first finding.  multipliers: (one int in [1, 2^128) per point of pointsC1, one per point of pointsH1);
    None draws them with `secrets`.  A key without a log is a chain of no records."""
    import secrets

    from . import phase2
    ctx = ctx or default_context()
    for what, a, b in (("header", initial.header, zkey.header), ("pointsIC", initial.pointsIC, zkey.pointsIC),
                       ("alpha1", initial.specPoints.alpha1, zkey.specPoints.alpha1),
                       ("beta1", initial.specPoints.beta1, zkey.specPoints.beta1),
                       ("beta2", initial.specPoints.beta2, zkey.specPoints.beta2),
                       ("gamma2", initial.specPoints.gamma2, zkey.specPoints.gamma2),
                       ("pointsA1", initial.pPoints.pointsA1, zkey.pPoints.pointsA1),
                       ("pointsB1", initial.pPoints.pointsB1, zkey.pPoints.pointsB1),
                       ("pointsB2", initial.pPoints.pointsB2, zkey.pPoints.pointsB2)):
        if a != b:
            raise ValueError(f"verifyContributions: {what} of the key is not the initial key's")
    log = zkey.contributions if zkey.contributions is not None else phase2.Contributions(cs_hash=phase2.cs_hash(initial))
    ch, consistent = phase2.challenges(log)
    consistent = consistent and log.cs_hash == phase2.cs_hash(initial)
    ki, kf = _phase2Part(initial), _phase2Part(zkey)
    if multipliers is None:
        draw = lambda k: [secrets.randbelow((1 << 128) - 1) + 1 for _ in range(k)]     # noqa: E731
        multipliers = (draw(len(kf["pointsC1"]) // 64), draw(len(kf["pointsH1"]) // 64))
    rep = ctx.contributions_verify(ki, kf, log.records, ch, multipliers[0], multipliers[1])
    rep.transcript = 1 if consistent else 0
    return rep
