"""Host mirror of groth16/fake_setup.nim: a "fake" circuit-specific trusted setup from explicit toxic
waste.  Two paths to the same key bytes (fakeCircuitSetup, `scalarSide`):
  "device"  (the default with a _lib.Context) one g16_fake_setup call (include/g16hip.h): Lagrange values at tau, column sums, the combinations of
            fake_setup.nim:263-277, the H scalars and every `y ** gen` on the GPU, nothing returning in between;
  "host"    the O(n) scalar bookkeeping in Python integers as in the reference; every `y ** gen1` / `y ** gen2`
            (fake_setup.nim:258-261, 273-277, 290-302: ~4N+n G1 and N G2 scalar multiplications) on the GPU
            (g16_fixed_base_g1/g2), and so the sparse column dot products (fake_setup.nim:159-187, 254-256: ~10^7
            multiplications for a Poseidon-shaped circuit of 2^20 constraints) through the transposed matrices
            (g16_spmv_fr)."""
from __future__ import annotations

from dataclasses import dataclass

from . import bn128 as F
from ._lib import G16Error, default_context
from .zkey_types import (GrothHeader, JensGroth, MatrixA, MatrixB, ProverPoints, Snarkjs, SpecPoints, ZKey)

R = F.primeR


@dataclass
class ToxicWaste:                    # fake_setup.nim:23-29
    alpha: int
    beta: int
    gamma: int
    delta: int
    tau: int


@dataclass
class R1CS:                          # files/r1cs.nim:62-80; constraint = (A, B, C), each [(wireIdx, value)]
    nWires: int
    nPubOut: int
    nPubIn: int
    nPrivIn: int
    constraints: list
    wireToLabel: list = None


def r1csToCoeffs(r1cs: R1CS):
    """fake_setup.nim:46-65 (incl. snarkjs' dummy A rows for the public IO)."""
    coeffs = []
    n = len(r1cs.constraints)
    p = r1cs.nPubIn + r1cs.nPubOut
    for i, (A, B, _C) in enumerate(r1cs.constraints):
        for (w, v) in A:
            coeffs.append((MatrixA, i, w, F.frToMontBytes(v)))
        for (w, v) in B:
            coeffs.append((MatrixB, i, w, F.frToMontBytes(v)))
    one = F.frToMontBytes(1)
    for i in range(n, n + p + 1):
        coeffs.append((MatrixA, i, i - n, one))
    return coeffs


def r1csToCoeffArray(r1cs):
    """r1csToCoeffs for a synthetic.SparseR1CS, vectorised: -> zkey_types.CoeffArray (the g16_coeff records of
    include/g16hip.h: all A entries, all B entries, then the dummy A rows; buildABC sums per row, so the order of
    ZKey.coeffs is immaterial, prover.nim:56-73)."""
    import numpy as np
    from .zkey_types import COEFF_DTYPE, CoeffArray
    n, p = r1cs.nConstraints, r1cs.nPubIn + r1cs.nPubOut
    table = np.frombuffer(F.frSeqToMontBytes(r1cs.values + [1]), dtype=np.uint8).reshape(-1, 32)
    na, nb = len(r1cs.A[0]), len(r1cs.B[0])
    arr = np.zeros(na + nb + p + 1, dtype=COEFF_DTYPE)
    for lo, (rows, wires, vi), m in ((0, r1cs.A, MatrixA), (na, r1cs.B, MatrixB)):
        hi = lo + len(rows)
        arr["m"][lo:hi], arr["r"][lo:hi], arr["c"][lo:hi], arr["v"][lo:hi] = m, rows, wires, table[vi]
    arr["m"][na + nb:] = MatrixA
    arr["r"][na + nb:] = np.arange(n, n + p + 1)
    arr["c"][na + nb:] = np.arange(p + 1)
    arr["v"][na + nb:] = table[len(r1cs.values)]
    return CoeffArray(arr)


def _triplets(r1cs):
    """-> (values, A, B, C): the distinct coefficient values (ints) and per matrix (constraint, wire, value index) as
    numpy arrays, from the list form (files/r1cs.nim:62-80) or from a synthetic.SparseR1CS"""
    import numpy as np
    if hasattr(r1cs, "values"):
        return r1cs.values, r1cs.A, r1cs.B, r1cs.C
    values, index = [], {}
    mats = ([[], [], []], [[], [], []], [[], [], []])
    for i, con in enumerate(r1cs.constraints):
        for k in range(3):
            for (w, v) in con[k]:
                v %= R
                j = index.get(v)
                if j is None:
                    j = index[v] = len(values)
                    values.append(v)
                mats[k][0].append(i), mats[k][1].append(w), mats[k][2].append(j)
    return (values,) + tuple(tuple(np.array(x, dtype=np.uint32) for x in m) for m in mats)


def columnDots(r1cs, lag, ctx):
    """The sparse column dot products of fake_setup.nim:159-187, 254-256: taus_M[wire] = sum over the entries of
    column `wire` of matrix M of value * L_row(tau), for M = A (incl. the dummy rows of the public IO, :59-63), B, C
    -- on the GPU: the transposed matrices through the row-balanced kernel of buildABC (g16_spmv_fr)."""
    import numpy as np
    values, A, B, C = _triplets(r1cs)
    neqs = r1cs.nConstraints if hasattr(r1cs, "nConstraints") else len(r1cs.constraints)
    npub = r1cs.nPubIn + r1cs.nPubOut
    table = np.frombuffer(F.frSeqToMontBytes(list(values) + [1]), dtype=np.uint8).reshape(-1, 32)
    lagb = F.frSeqToMontBytes(lag)
    out = []
    for k, (rows, wires, vi) in enumerate((A, B, C)):
        rows, wires, vi = (np.asarray(x, dtype=np.uint32) for x in (rows, wires, vi))
        if k == 0:
            rows = np.concatenate([rows, np.arange(neqs, neqs + npub + 1, dtype=np.uint32)])
            wires = np.concatenate([wires, np.arange(npub + 1, dtype=np.uint32)])
            vi = np.concatenate([vi, np.full(npub + 1, len(values), dtype=np.uint32)])
        out.append(ctx.spmv(wires, rows, table[vi], lagb, r1cs.nWires))
    return out            # Montgomery Fr bytes, nWires elements each


_lag_cache = {}


def lagrangeTaus(logDom: int, tau: int):
    """[L_k(tau) for k < 2^logDom]  == evalLagrangePolyAt (math/poly.nim:242-250) for every k.  (The last two results
    are kept: bench.py builds two keys over one domain from the same toxic waste.)"""
    key = (logDom, tau % R)
    if key not in _lag_cache:
        while len(_lag_cache) >= 2:
            _lag_cache.pop(next(iter(_lag_cache)))
        _lag_cache[key] = _lagrangeTaus(logDom, tau)
    return _lag_cache[key]


def _lagrangeTaus(logDom: int, tau: int):
    dom = 1 << logDom
    g = F.domainGen(logDom)
    ztau = (pow(tau, dom, R) - 1) % R
    invN = F.invFr(dom % R)
    omegas, denoms, w = [], [], 1
    for _ in range(dom):
        omegas.append(w)
        d = (tau - w) % R
        if d == 0:
            raise AssertionError("point should be outside the domain")
        denoms.append(d)
        w = w * g % R
    dinv = F.batchInverseFr(denoms)
    c = ztau * invN % R
    return [omegas[k] * c % R * dinv[k] % R for k in range(dom)]


def _deviceSetup(r1cs, toxic: ToxicWaste, flavour, ctx) -> ZKey:
    """fakeCircuitSetup with the scalar side on the device: one g16_fake_setup call (include/g16hip.h)"""
    import numpy as np
    values, A, B, C = _triplets(r1cs)
    neqs = r1cs.nConstraints if hasattr(r1cs, "nConstraints") else len(r1cs.constraints)
    npub = r1cs.nPubIn + r1cs.nPubOut
    table = np.frombuffer(F.frSeqToMontBytes(list(values) + [0]), dtype=np.uint8).reshape(-1, 32)
    mats = [(rows, wires, table[np.asarray(vi, dtype=np.int64)]) for (rows, wires, vi) in (A, B, C)]
    tox = [F.frToMontBytes(x % R) for x in (toxic.alpha, toxic.beta, toxic.gamma, toxic.delta, toxic.tau)]
    try:
        logDom, pts = ctx.fake_setup(r1cs.nWires, npub, neqs, flavour, mats, tox, mont=True)
    except G16Error as e:
        if "tau lies in the domain" in str(e):
            raise AssertionError("point should be outside the domain") from e     # math/poly.nim:245
        raise
    zkey = ZKey()
    zkey.header = GrothHeader("bn128", flavour, r1cs.nWires, npub, 1 << logDom, logDom)
    zkey.specPoints = SpecPoints(**{k: pts[k] for k in ("alpha1", "beta1", "delta1", "beta2", "gamma2", "delta2")})
    zkey.pointsIC = pts["pointsIC"]
    zkey.pPoints = ProverPoints(**{k: pts[k] for k in ("pointsA1", "pointsB1", "pointsB2", "pointsC1", "pointsH1")})
    zkey.coeffs = r1csToCoeffArray(r1cs) if hasattr(r1cs, "values") else r1csToCoeffs(r1cs)
    return zkey


def fakeCircuitSetup(r1cs: R1CS, toxic: ToxicWaste, flavour=Snarkjs, ctx=None, scalarSide=None) -> ZKey:
    """fake_setup.nim:201-326.  scalarSide "device": one g16_fake_setup call with every intermediate in HBM; "host": the
    Lagrange values, the combinations and the H scalars in Python integers, the results crossing to the GPU and back
    between the stages.  The keys are the same bytes (tests/test_gpu_setup.py; profiles/fake_setup_ab.txt has the
    times).  None, the default: "device" for a context that offers g16_fake_setup -- every _lib.Context -- and "host"
    for a stand-in that implements only the two calls the host path makes (spmv, fixed_base)."""
    ctx = ctx or default_context()
    if scalarSide is None:
        scalarSide = "device" if hasattr(ctx, "fake_setup") else "host"
    if scalarSide == "device":
        return _deviceSetup(r1cs, toxic, flavour, ctx)
    if scalarSide != "host":
        raise ValueError(f"scalarSide must be 'host' or 'device', not {scalarSide!r}")
    neqs = r1cs.nConstraints if hasattr(r1cs, "nConstraints") else len(r1cs.constraints)
    npub = r1cs.nPubIn + r1cs.nPubOut
    logDom = F.ceilingLog2(neqs + npub + 1)
    dom = 1 << logDom
    nvars = r1cs.nWires
    tau = toxic.tau % R
    lag = lagrangeTaus(logDom, tau)

    bytesA, bytesB, bytesC = columnDots(r1cs, lag, ctx)
    tausA, tausB, tausC = (F.frSeqFromMontBytes(x) for x in (bytesA, bytesB, bytesC))

    gammaInv, deltaInv = F.invFr(toxic.gamma), F.invFr(toxic.delta)
    comb = [(toxic.beta * tausA[j] + toxic.alpha * tausB[j] + tausC[j]) % R for j in range(nvars)]
    if flavour == JensGroth:
        ztau = (pow(tau, dom, R) - 1) % R
        hs, tp = [], 1
        for _ in range(dom):                       # fake_setup.nim:290-292
            hs.append(deltaInv * tp % R * ztau % R)
            tp = tp * tau % R
    else:                                          # fake_setup.nim:299-302: delta^-1 L_{2i+1}(tau), doubled domain
        lag2 = lagrangeTaus(logDom + 1, tau)
        hs = [deltaInv * lag2[2 * i + 1] % R for i in range(dom)]

    enc = F.frSeqToMontBytes
    g1 = lambda xs: ctx.fixed_base(1, enc(xs))     # noqa: E731   `y ** gen1`
    g2 = lambda xs: ctx.fixed_base(2, enc(xs))     # noqa: E731   `y ** gen2`
    spec1 = g1([toxic.alpha, toxic.beta, toxic.delta])
    spec2 = g2([toxic.beta, toxic.gamma, toxic.delta])
    zkey = ZKey()
    zkey.header = GrothHeader("bn128", flavour, nvars, npub, dom, logDom)
    zkey.specPoints = SpecPoints(alpha1=spec1[0:64], beta1=spec1[64:128], delta1=spec1[128:192],
                                 beta2=spec2[0:128], gamma2=spec2[128:256], delta2=spec2[256:384])
    zkey.pointsIC = g1([gammaInv * comb[j] % R for j in range(npub + 1)])
    zkey.pPoints = ProverPoints(
        pointsA1=ctx.fixed_base(1, bytesA), pointsB1=ctx.fixed_base(1, bytesB), pointsB2=ctx.fixed_base(2, bytesB),
        pointsC1=g1([deltaInv * comb[j] % R for j in range(npub + 1, nvars)]),
        pointsH1=g1(hs))
    zkey.coeffs = r1csToCoeffArray(r1cs) if hasattr(r1cs, "values") else r1csToCoeffs(r1cs)
    return zkey


def fakePtau(tau: int, alpha: int, beta: int, power: int, ctx=None):
    """The powers of tau a ceremony with this toxic waste would publish (files/ptau.py): tau^k gen1 for k < 2^(power+1) - 1,
    tau^k gen2, alpha tau^k gen1 and beta tau^k gen1 for k < 2^power, beta gen2 -- the scalars by g16_powers_fr, the points
    by g16_fixed_base_g1/g2.  A key that fakeCircuitSetup builds from the same (tau, alpha, beta) passes the circuit audit
    (files/zkey.auditCircuit) against it, whatever its gamma and delta."""
    from .files.ptau import Ptau
    ctx = ctx or default_context()
    enc = F.frToMontBytes
    n1, n = (2 << power) - 1, 1 << power
    taus = ctx.powers(enc(tau % R), n1)
    return Ptau(power=power, tauG1=ctx.fixed_base(1, taus), tauG2=ctx.fixed_base(2, taus[:32 * n]),
                alphaTauG1=ctx.fixed_base(1, ctx.powers(enc(tau % R), n, scale=enc(alpha % R))),
                betaTauG1=ctx.fixed_base(1, ctx.powers(enc(tau % R), n, scale=enc(beta % R))),
                betaG2=ctx.fixed_base(2, enc(beta % R)))
