"""groth16/files/zkey.nim: the snarkjs proving key.  Point sections (3, 5-9) and the spec points hold
little-endian Montgomery (R = 2^256) coordinates -- byte for byte the in-memory G1/G2 layout the GPU library
takes (bn128/io.nim:103-131), so they are passed through unparsed.  Section 4 coefficients are *doubly*
Montgomery encoded (zkey.nim:57, io.nim:134-139)."""
from __future__ import annotations

import struct

import numpy as np

from .. import bn128 as F
from ..zkey_types import GrothHeader, ProverPoints, Snarkjs, SpecPoints, ZKey
from .container import parseContainer, parsePrimeField, writeContainer

_R = F.primeR


def checkZKeyPoints(zk: ZKey, ctx=None) -> None:
    """The reference asserts that every loaded point lies on its curve (mkG1/mkG2, curves.nim:95-107).  Here the
    check is one GPU pass per section, run on request (parseZKey(..., check=True))."""
    from .._lib import default_context
    ctx = ctx or default_context()
    sp, pp = zk.specPoints, zk.pPoints
    for name, group, buf in (("spec G1", 1, sp.alpha1 + sp.beta1 + sp.delta1), ("spec G2", 2, sp.beta2 + sp.gamma2 + sp.delta2),
                             ("pointsIC", 1, zk.pointsIC), ("pointsA1", 1, pp.pointsA1), ("pointsB1", 1, pp.pointsB1),
                             ("pointsB2", 2, pp.pointsB2), ("pointsC1", 1, pp.pointsC1), ("pointsH1", 1, pp.pointsH1)):
        bad = ctx.points_check(group, buf)
        assert bad is None, f"mkG{group}: {name}[{bad}] is not a G{group} curve point"


def auditZKey(zk: ZKey, ctx=None, multipliers=None):
    """Is an untrusted key fit to prove with?  One g16_key_audit over every section of the key (include/g16hip.h):
    canonical encodings, curve membership, the order-r subgroup for the G2 points, coefficient values < r, and the
    relations pointsB1 ~ pointsB2, beta1 ~ beta2, delta1 ~ delta2.  -> _lib.KeyReport: `.ok`, and str() names the
    section, index and check of every first finding.  multipliers: one int in [1, 2^128) per wire for the batched
    relation; None draws them with `secrets`, as verifyProofsBatch does.  A key parsed with rawCoeffs is audited on
    its coefficient section as it lies in the file.  What no audit can tell: whether the key belongs to a circuit."""
    import ctypes
    import secrets

    from .._lib import VkeyDesc, default_context
    from ..prover import pkeyDesc
    ctx = ctx or default_context()
    desc, bufs, raw4 = pkeyDesc(zk)
    sp = zk.specPoints
    vbufs = [ctypes.create_string_buffer(x, len(x)) for x in (sp.alpha1, sp.beta2, sp.gamma2, sp.delta2, zk.pointsIC)]
    va = [ctypes.cast(b, ctypes.c_void_p) for b in vbufs]
    vk = VkeyDesc(zk.header.npubs, va[0], va[1], va[2], va[3], va[4])
    if multipliers is None:
        multipliers = [secrets.randbelow((1 << 128) - 1) + 1 for _ in range(zk.header.nvars)]
    rep = ctx.key_audit(desc, vk, section4=raw4, multipliers=multipliers)
    del bufs, vbufs
    return rep


def r1csDesc(r1cs, flavour: int):
    """The g16_r1cs_desc of an R1CS (the list form of files/r1cs.py or a synthetic.SparseR1CS) -> (desc, keepalive)"""
    from .._lib import SCALARS_MONT, R1csDesc, _buf
    from ..fake_setup import _triplets
    values, A, B, C = _triplets(r1cs)
    table = np.frombuffer(F.frSeqToMontBytes(list(values) + [0]), dtype=np.uint8).reshape(-1, 32)
    d = R1csDesc()
    d.nvars, d.npubs = r1cs.nWires, r1cs.nPubIn + r1cs.nPubOut
    d.nconstraints = r1cs.nConstraints if hasattr(r1cs, "nConstraints") else len(r1cs.constraints)
    d.flavour, d.flags = flavour, SCALARS_MONT
    keep = []
    for k, (rows, wires, vi) in enumerate((A, B, C)):
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        wires = np.ascontiguousarray(wires, dtype=np.uint32)
        vals = np.ascontiguousarray(table[np.asarray(vi, dtype=np.int64)])
        keep += [rows, wires, vals]
        d.nnz[k] = len(rows)
        if len(rows):
            d.row[k], d.col[k], d.val[k] = (_buf(x).value for x in (rows, wires, vals))
    return d, keep


def ptauDesc(ptau):
    """The g16_ptau_desc of a files.ptau.Ptau -> (desc, keepalive)"""
    import ctypes

    from .._lib import PTAU_SECTIONS, PtauDesc
    bufs = [ctypes.create_string_buffer(x, len(x)) for x in (getattr(ptau, name) for name in PTAU_SECTIONS)]
    return PtauDesc(ptau.power, *[ctypes.cast(b, ctypes.c_void_p) for b in bufs]), bufs


def auditCircuit(zk: ZKey, r1cs, ptau, ctx=None, multipliers=None):
    """Does an untrusted key belong to THIS circuit and THIS powers of tau?  One g16_circuit_audit (include/g16hip.h):
    the key audit of auditZKey, the same element checks over the ptau, the key's coefficients against the r1cs as linear
    maps, and every point array of the key against the powers of tau -- what `snarkjs zkey verify` checks before the
    contribution chain.  r1cs: as parseR1CS returns it; ptau: a files.ptau.Ptau.  -> _lib.CircuitReport: `.ok`, str()
    names every first finding.  multipliers: (one int in [1, 2^128) per wire, one per domain element); None draws them
    with `secrets`.  Not covered: the ptau's own consistency, and the contribution chain (section 10)."""
    import ctypes
    import secrets

    from .._lib import VkeyDesc, default_context
    from ..prover import pkeyDesc
    ctx = ctx or default_context()
    desc, bufs, raw4 = pkeyDesc(zk)
    sp = zk.specPoints
    vbufs = [ctypes.create_string_buffer(x, len(x)) for x in (sp.alpha1, sp.beta2, sp.gamma2, sp.delta2, zk.pointsIC)]
    va = [ctypes.cast(b, ctypes.c_void_p) for b in vbufs]
    vk = VkeyDesc(zk.header.npubs, va[0], va[1], va[2], va[3], va[4])
    rd, rkeep = r1csDesc(r1cs, zk.header.flavour)
    pd, pkeep = ptauDesc(ptau)
    if multipliers is None:
        draw = lambda k: [secrets.randbelow((1 << 128) - 1) + 1 for _ in range(k)]     # noqa: E731
        multipliers = (draw(zk.header.nvars), draw(zk.header.domainSize))
    rep = ctx.circuit_audit(desc, vk, raw4, rd, pd, multipliers[0], multipliers[1])
    del bufs, vbufs, rkeep, pkeep
    return rep


def parseZKey(fname: str, check: bool = False, ctx=None, rawCoeffs: bool = False) -> ZKey:
    """zkey.nim:241-246.  rawCoeffs: keep the coefficient section as it lies in the file (ZKey.coeffsSection4, handed to
    the GPU unparsed by loadProvingKey -> g16_pkey_create_zkey) instead of un-Montgomerying every entry on the host
    (io.nim:134-139): what a large key wants -- a Poseidon-Merkle circuit of 2^20 constraints has ~10^7 entries."""
    sec = parseContainer("zkey", 1, fname)
    one = lambda i: sec[i][0]                                            # noqa: E731
    s1 = one(1)                                                          # zkey.nim:104-107
    assert len(s1) == 4, "unexpected section length"
    assert struct.unpack_from("<I", s1, 0)[0] == 1, "expecting `.zkey` file for a Groth16 prover"
    s2 = one(2)                                                          # zkey.nim:114-165
    n8p, p, pos = parsePrimeField(s2, 0)
    n8r, r, pos = parsePrimeField(s2, pos)
    assert len(s2) == 2 * 4 + n8p + n8r + 3 * 4 + 3 * 64 + 3 * 128, "unexpected section length"
    assert n8p == 32 and n8r == 32, "expecting 256 bit primes"
    assert p == F.primeP and r == F.primeR, "expecting the alt-bn128 curve"
    nvars, npubs, domsiz = struct.unpack_from("<III", s2, pos)
    pos += 12
    log2siz = F.ceilingLog2(domsiz)
    assert (1 << log2siz) == domsiz, "domain size should be a power of two"
    zk = ZKey()
    zk.header = GrothHeader("bn128", Snarkjs, nvars, npubs, domsiz, log2siz)   # parsed keys are Snarkjs (zkey.nim:129)

    def take(k):
        nonlocal pos
        b = bytes(s2[pos:pos + k])
        pos += k
        return b
    a1, b1, b2, g2, d1, d2 = take(64), take(64), take(128), take(128), take(64), take(128)
    zk.specPoints = SpecPoints(alpha1=a1, beta1=b1, beta2=b2, gamma2=g2, delta1=d1, delta2=d2)

    def pts(i, psz, n):
        s = one(i)
        assert len(s) == psz * n, "unexpected section length"
        return s.tobytes()
    zk.pointsIC = pts(3, 64, npubs + 1)                                  # zkey.nim:196-199
    zk.pPoints = ProverPoints(pointsA1=pts(5, 64, nvars), pointsB1=pts(6, 64, nvars), pointsB2=pts(7, 128, nvars),
                              pointsC1=pts(8, 64, nvars - npubs - 1), pointsH1=pts(9, 64, domsiz))
    s4 = one(4)                                                          # zkey.nim:169-192
    (ncoeffs,) = struct.unpack_from("<I", s4, 0)
    assert len(s4) == 4 + ncoeffs * (32 + 12), "unexpected section length"
    rec = np.frombuffer(s4, dtype=np.dtype([("m", "<u4"), ("r", "<u4"), ("c", "<u4"), ("v", "u1", (32,))]),
                        count=ncoeffs, offset=4)
    assert ncoeffs == 0 or int(rec["m"].max()) <= 2, "invalid matrix selector"
    assert ncoeffs == 0 or int(rec["r"].max()) < domsiz, "row index out of range"
    assert ncoeffs == 0 or int(rec["c"].max()) < nvars, "column index out of range"
    if rawCoeffs:
        zk.coeffs, zk.coeffsSection4 = [], bytes(s4)
        if check:
            checkZKeyPoints(zk, ctx)
        return zk
    raw = rec["v"].tobytes()
    # file integer = c * R^2 ; in-memory Montgomery limbs of c = c * R = file integer * R^-1   (unmarshalFrWTF)
    ms, rs, cs = rec["m"].tolist(), rec["r"].tolist(), rec["c"].tolist()
    coeffs = []
    for i in range(ncoeffs):
        v = int.from_bytes(raw[32 * i:32 * i + 32], "little")
        coeffs.append((ms[i], rs[i], cs[i], (v * F.frInvMontR % _R).to_bytes(32, "little")))
    zk.coeffs = coeffs
    if check:
        checkZKeyPoints(zk, ctx)
    return zk


def zkeySections(zk: ZKey):
    """sections 1-9 of the .zkey of a key, [(id, data)] in file order (zkey.nim:6-91)"""
    h, sp, pp = zk.header, zk.specPoints, zk.pPoints
    le32 = lambda x: int(x).to_bytes(32, "little")                       # noqa: E731
    s2 = (struct.pack("<I", 32) + le32(F.primeP) + struct.pack("<I", 32) + le32(F.primeR) +
          struct.pack("<III", h.nvars, h.npubs, h.domainSize) +
          sp.alpha1 + sp.beta1 + sp.beta2 + sp.gamma2 + sp.delta1 + sp.delta2)
    if zk.coeffsSection4 is not None and not zk.coeffs:
        s4 = bytes(zk.coeffsSection4)
    else:
        s4 = bytearray(struct.pack("<I", len(zk.coeffs)))
        for (m, r, c, v) in zk.coeffs:
            x = int.from_bytes(v, "little") * F.frMontR % _R             # c*R -> c*R^2
            s4 += struct.pack("<III", m, r, c) + x.to_bytes(32, "little")
    return [(1, struct.pack("<I", 1)), (2, s2), (3, zk.pointsIC), (4, bytes(s4)), (5, pp.pointsA1), (6, pp.pointsB1),
            (7, pp.pointsB2), (8, pp.pointsC1), (9, pp.pointsH1)]


def contributionsSection(log) -> bytes:
    """Section 10 of a .zkey from a phase2.Contributions: csHash (64 B) | u32 count | per record deltaAfter | g1_s | g1_sx
    (64 B each) | g2_spx (128 B) | transcript (64 B) | u32 type = 0 | u32 params length | params (the name, UTF-8).
    The maintainers' reading of snarkjs's layout, UNPINNED: no snarkjs-written file was at hand to hold it to; and the
    hashes in it follow this project's own rule (phase2.py), not snarkjs's."""
    assert len(log.cs_hash) == 64 and len(log.records) == len(log.transcripts) == len(log.names)
    out = bytearray(log.cs_hash) + struct.pack("<I", len(log.records))
    for rec, tr, name in zip(log.records, log.transcripts, log.names):
        assert len(rec) == 320 and len(tr) == 64
        params = name.encode("utf-8")
        out += rec + tr + struct.pack("<II", 0, len(params)) + params
    return bytes(out)


def parseContributions(fname: str):
    """Section 10 of a .zkey written by writeZKey -> phase2.Contributions; None when the file has no section 10.  Raises
    ValueError on a section that is not laid out as contributionsSection writes it (parseZKey itself never reads the
    section: a prover has no use for it)."""
    from ..phase2 import Contributions
    sec = parseContainer("zkey", 1, fname)
    if 10 not in sec:
        return None
    s = bytes(sec[10][0])
    if len(s) < 68:
        raise ValueError("section 10: shorter than csHash and the record count")
    (count,) = struct.unpack_from("<I", s, 64)
    log, pos = Contributions(cs_hash=s[:64]), 68
    for j in range(count):
        if pos + 320 + 64 + 8 > len(s):
            raise ValueError(f"section 10: record {j} is truncated")
        rec, tr = s[pos:pos + 320], s[pos + 320:pos + 384]
        typ, plen = struct.unpack_from("<II", s, pos + 384)
        pos += 392
        if typ != 0:
            raise ValueError(f"section 10: record {j} has contribution type {typ} (only 0 is written here)")
        if pos + plen > len(s):
            raise ValueError(f"section 10: the params of record {j} are truncated")
        try:
            name = s[pos:pos + plen].decode("utf-8")
        except UnicodeDecodeError:
            raise ValueError(f"section 10: the name of record {j} is not UTF-8") from None
        pos += plen
        log.records.append(rec)
        log.transcripts.append(tr)
        log.names.append(name)
    if pos != len(s):
        raise ValueError("section 10: bytes left over after the last record")
    return log


def writeZKey(fname: str, zk: ZKey) -> None:
    """Inverse of parseZKey (sections 1-9 of zkey.nim:6-91).  Section 10, the ceremony contributions, is not needed for
    proving; it is written when the key carries a contribution log (zk.contributions, contributionsSection).
    A key parsed with rawCoeffs (coeffsSection4 set, `coeffs` empty) is written with that section as it lay in its file;
    before the contribution log existed such a key was written with an EMPTY coefficient section, which made a file
    nothing could prove from, and its cs_hash would have differed from the same key parsed entry by entry."""
    sections = zkeySections(zk)
    if getattr(zk, "contributions", None) is not None:
        sections.append((10, contributionsSection(zk.contributions)))
    writeContainer("zkey", 1, fname, sections)
