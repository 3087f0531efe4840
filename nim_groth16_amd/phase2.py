"""The transcript of a phase-2 ceremony, in pure Python: what ties the records of the contributions to the key they
started from and gives every contribution its challenge point.  The arithmetic on the key is the library's
(g16_key_contribute, g16_contributions_verify, include/g16hip.h), which hashes nothing and draws nothing; the hashes live
here.

    cs_hash      = BLAKE2b-512 over sections 2-9 of the INITIAL key as files.zkey.writeZKey lays them out, each as
                   id (u32) | size (u64) | data
    transcript_j = BLAKE2b-512(cs_hash | record_0 | transcript_0 | ... | record_(j-1) | transcript_(j-1) | g1_s_j | g1_sx_j)
    challenge_j  = hash_to_g2(transcript_j)
    hash_to_g2(h): for ctr = 0, 1, ...: x = (c0, c1) in Fp2 from the two halves of BLAKE2b-512(h | b"g16hip-g2" | ctr as
                   u32), each reduced mod p; y^2 = x^3 + b' on the twist; the first ctr with a square root wins; of the two
                   roots the one with the smaller (c1, c0) pair; the point times the cofactor 2p - r

UNPINNED, and NOT snarkjs's rule: snarkjs derives its challenge with a ChaCha stream seeded from the transcript hash
(`hashToG2`) and hashes its own serialisation of the key.  A snarkjs verifier will reject the proof of knowledge in a
record written here, and verifyContributions rejects snarkjs's records.  The rescaled key itself (sections 2, 8, 9 of
the .zkey) is a plain snarkjs key either way: it proves, verifies and passes files.zkey.auditCircuit like any other."""
from __future__ import annotations

import hashlib
import struct
from dataclasses import dataclass, field
from typing import List

from . import bn128 as F

P, R = F.primeP, F.primeR
COFACTOR_G2 = 2 * P - R
DOMAIN_TAG = b"g16hip-g2"
RECORD_BYTES = 320


# ---- Fp2 = Fp[i] / (i^2 + 1) and the twist, for hash_to_g2 only (a few hundred point operations per challenge) ----------
def _mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def _sqr(a):
    return _mul(a, a)


def _add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def _sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def _inv(a):
    t = pow(a[0] * a[0] + a[1] * a[1], -1, P)
    return (a[0] * t % P, -a[1] * t % P)


def _pow(a, e):
    out = (1, 0)
    while e:
        if e & 1:
            out = _mul(out, a)
        a = _sqr(a)
        e >>= 1
    return out


TWIST_B = _mul((3, 0), _inv((9, 1)))          # b' = 3 / (9 + i)
_ZERO, _ONE = (0, 0), (1, 0)


def fp2_sqrt(a):
    """a square root of a in Fp2 (p = 3 mod 4), or None"""
    if a == _ZERO:
        return _ZERO
    a1 = _pow(a, (P - 3) // 4)
    alpha = _mul(_sqr(a1), a)
    x0 = _mul(a1, a)
    if alpha == (P - 1, 0):
        x = _mul((0, 1), x0)
    else:
        x = _mul(_pow(_add(_ONE, alpha), (P - 1) // 2), x0)
    return x if _sqr(x) == a else None


def _jdbl(p):
    X, Y, Z = p
    if Z == _ZERO:
        return p
    A, B = _sqr(X), _sqr(Y)
    C = _sqr(B)
    D = _sub(_sub(_sqr(_add(X, B)), A), C)
    D = _add(D, D)
    E = _add(_add(A, A), A)
    X3 = _sub(_sqr(E), _add(D, D))
    C8 = _add(C, C)
    C8 = _add(C8, C8)
    C8 = _add(C8, C8)
    Z3 = _mul(Y, Z)
    return (X3, _sub(_mul(E, _sub(D, X3)), C8), _add(Z3, Z3))


def _jadd(p, q):
    if p[2] == _ZERO:
        return q
    if q[2] == _ZERO:
        return p
    z1, z2 = _sqr(p[2]), _sqr(q[2])
    u1, u2 = _mul(p[0], z2), _mul(q[0], z1)
    s1, s2 = _mul(p[1], _mul(q[2], z2)), _mul(q[1], _mul(p[2], z1))
    h, r = _sub(u2, u1), _sub(s2, s1)
    if h == _ZERO:
        return _jdbl(p) if r == _ZERO else (_ONE, _ONE, _ZERO)
    hh = _sqr(h)
    hhh, v = _mul(h, hh), _mul(u1, hh)
    x3 = _sub(_sub(_sqr(r), hhh), _add(v, v))
    return (x3, _sub(_mul(r, _sub(v, x3)), _mul(s1, hhh)), _mul(_mul(p[2], q[2]), h))


def g2_mul(k: int, pt):
    """k * pt on the twist; pt = (x, y) affine with Fp2 coordinates as integer pairs, ((0,0),(0,0)) = infinity"""
    if pt == (_ZERO, _ZERO):
        return pt
    base, acc = (pt[0], pt[1], _ONE), (_ONE, _ONE, _ZERO)
    for bit in bin(k)[2:] if k else "":
        acc = _jdbl(acc)
        if bit == "1":
            acc = _jadd(acc, base)
    if acc[2] == _ZERO:
        return (_ZERO, _ZERO)
    zi = _inv(acc[2])
    zi2 = _sqr(zi)
    return (_mul(acc[0], zi2), _mul(acc[1], _mul(zi2, zi)))


def g2_to_bytes(pt) -> bytes:
    """the library's layout: x.c0 | x.c1 | y.c0 | y.c1, Montgomery, little-endian"""
    return b"".join(F.fpToMontBytes(c) for c in (pt[0][0], pt[0][1], pt[1][0], pt[1][1]))


def hash_to_g2(h: bytes):
    """the challenge point of a transcript hash (module docstring) -> affine point of the order-r subgroup of the twist"""
    ctr = 0
    while True:
        d = hashlib.blake2b(h + DOMAIN_TAG + struct.pack("<I", ctr)).digest()
        x = (int.from_bytes(d[:32], "little") % P, int.from_bytes(d[32:], "little") % P)
        y = fp2_sqrt(_add(_mul(_sqr(x), x), TWIST_B))
        ctr += 1
        if y is None:
            continue
        neg = ((-y[0]) % P, (-y[1]) % P)
        if (neg[1], neg[0]) < (y[1], y[0]):
            y = neg
        pt = g2_mul(COFACTOR_G2, (x, y))
        if pt != (_ZERO, _ZERO):
            return pt


# ---- the transcript --------------------------------------------------------------------------------------------------------
def cs_hash(zk) -> bytes:
    """BLAKE2b-512 over sections 2-9 of a key as writeZKey lays them out (each: id u32 | size u64 | data)"""
    from .files.zkey import zkeySections
    h = hashlib.blake2b()
    for sid, data in zkeySections(zk):
        if 2 <= sid <= 9:
            h.update(struct.pack("<IQ", sid, len(data)))
            h.update(data)
    return h.digest()


@dataclass
class Contributions:
    """the contribution log of a key: what section 10 of its .zkey holds"""
    cs_hash: bytes
    records: List[bytes] = field(default_factory=list)       # 320 bytes each: delta_after | g1_s | g1_sx | g2_spx
    transcripts: List[bytes] = field(default_factory=list)   # 64 bytes each
    names: List[str] = field(default_factory=list)


def transcript_hash(log: Contributions, j: int, g1_s: bytes, g1_sx: bytes) -> bytes:
    """transcript_j from the first j records of `log` and the two G1 points of contribution j"""
    assert len(g1_s) == 64 and len(g1_sx) == 64 and len(log.cs_hash) == 64 and 0 <= j <= len(log.records)
    h = hashlib.blake2b(log.cs_hash)
    for rec, tr in zip(log.records[:j], log.transcripts[:j]):
        assert len(rec) == RECORD_BYTES and len(tr) == 64
        h.update(rec)
        h.update(tr)
    h.update(g1_s)
    h.update(g1_sx)
    return h.digest()


def challenge_bytes(transcript: bytes) -> bytes:
    return g2_to_bytes(hash_to_g2(transcript))


def challenges(log: Contributions):
    """-> (the challenge point of every record as the library takes it, whether every stored transcript hash is the one
    its predecessors give)"""
    out, consistent = [], len(log.records) == len(log.transcripts)
    for j, rec in enumerate(log.records):
        tr = transcript_hash(log, j, rec[64:128], rec[128:192])
        consistent = consistent and j < len(log.transcripts) and tr == log.transcripts[j]
        out.append(challenge_bytes(tr))
    return out, consistent
