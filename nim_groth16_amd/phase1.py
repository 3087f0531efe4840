"""Phase 1 of a ceremony, in pure Python around g16_ptau_contribute (include/g16hip.h): a .ptau of generators, contributions
nobody else knows, and the transcript that gives every contribution its three challenge points.  The library hashes
nothing and draws nothing; the hashes live here.

    start        = BLAKE2b-512(b"g16hip-ptau" | power as u32)
    transcript_j = BLAKE2b-512(start | record_0 | ... | record_(j-1) | the six proof-of-knowledge G1 points of
                   contribution j: s_t gen1 | t s_t gen1 | s_a gen1 | a s_a gen1 | s_b gen1 | b s_b gen1)
    challenge_jx = phase2.hash_to_g2(transcript_j | one byte x), x = 0, 1, 2 for t, a, b

UNPINNED, and NOT snarkjs's rule, exactly as phase2.py says of its own: snarkjs derives its challenges with a ChaCha stream
seeded from its own hash of the previous response file.  A snarkjs verifier will reject the proofs of knowledge in a record
written here, and a verifier of these records rejects snarkjs's.  Sections 2-6 of the file are a plain .ptau either way:
g16_circuit_setup, g16_circuit_audit and snarkjs read them like any other.

verifyPtau is the check of a .ptau and of its chain of records (`snarkjs powersoftau verify`): run it on a .ptau from a
third party before the circuit setup or the circuit audit takes it as their anchor."""
from __future__ import annotations

import hashlib
import struct
from dataclasses import dataclass, field
from typing import List

from . import bn128 as F
from . import phase2
from .files.ptau import PTAU_RECORD_BYTES, Ptau

R = F.primeR
START_TAG = b"g16hip-ptau"
GEN1 = (1, 2)
# the library's generator of G2 (what g16_fixed_base_g2 multiplies; tests/test_phase1_cpu.py holds it to the oracle's)
GEN2 = ((12150282371940648588025820750256225345313886663747209662093324632631129970433,
         4481220487248307175821185836875007335888437113144368396302892639365759218235),
        (2452391235344852000785071949405254134959145083090483303540469249230552133576,
         6781711448666880737227463812604550784213209308689191484025779914572346631004))
MAX_POWER = 25


@dataclass
class PtauContributions:
    """the contribution log of a .ptau: what section 7 holds (files/ptau.py)"""
    power: int
    records: List[bytes] = field(default_factory=list)       # 1216 bytes each: g16_ptau_contribution
    names: List[str] = field(default_factory=list)


def gen1_bytes() -> bytes:
    return F.fpToMontBytes(GEN1[0]) + F.fpToMontBytes(GEN1[1])


def gen2_bytes() -> bytes:
    return phase2.g2_to_bytes(GEN2)


def newPtau(power: int) -> Ptau:
    """the file every ceremony starts from: tau = alpha = beta = 1, every element its generator"""
    if not 1 <= power <= MAX_POWER:
        raise ValueError(f"power must lie in [1, {MAX_POWER}]")
    n, g1, g2 = 1 << power, gen1_bytes(), gen2_bytes()
    return Ptau(power=power, tauG1=g1 * (2 * n - 1), tauG2=g2 * n, alphaTauG1=g1 * n, betaTauG1=g1 * n, betaG2=g2)


def transcript_hash(log: PtauContributions, j: int, pok_g1: bytes) -> bytes:
    """transcript_j from the first j records of `log` and the six proof-of-knowledge G1 points of contribution j"""
    assert len(pok_g1) == 6 * 64 and 0 <= j <= len(log.records)
    h = hashlib.blake2b(hashlib.blake2b(START_TAG + struct.pack("<I", log.power)).digest())
    for rec in log.records[:j]:
        assert len(rec) == PTAU_RECORD_BYTES
        h.update(rec)
    h.update(pok_g1)
    return h.digest()


def challenge_bytes(transcript: bytes) -> bytes:
    """the three challenge points of a transcript hash as the library takes them (3 x 128 bytes: for t, a, b)"""
    return b"".join(phase2.challenge_bytes(transcript + bytes([x])) for x in range(3))


def record_pok_g1(record: bytes) -> bytes:
    """the six G1 points of a record's proofs of knowledge, in the order the transcript hashes them"""
    assert len(record) == PTAU_RECORD_BYTES
    return b"".join(record[448 + 256 * x:448 + 256 * x + 128] for x in range(3))


def challenges(log: PtauContributions) -> List[bytes]:
    """the 384 challenge bytes of every record, re-derived from the records before it"""
    return [challenge_bytes(transcript_hash(log, j, record_pok_g1(rec))) for j, rec in enumerate(log.records)]


def contribute(ptau: Ptau, log: PtauContributions = None, t: int = None, a: int = None, b: int = None, name: str = "",
               ctx=None, pok_secrets=None):
    """One phase-1 contribution: (tau, alpha, beta) -> (t tau, a alpha, b beta), and a record in the log (a fresh one if
    None).  t, a, b and the three proof-of-knowledge secrets: integers in [1, r); None draws them with `secrets`.  All six
    are toxic waste: forget them.  -> (the new Ptau, the new log); the inputs are not changed."""
    import copy
    import secrets

    from ._lib import default_context
    ctx = ctx or default_context()
    draw = lambda: secrets.randbelow(R - 1) + 1          # noqa: E731
    t, a, b = (draw() if v is None else v for v in (t, a, b))
    s3 = [draw() for _ in range(3)] if pok_secrets is None else list(pok_secrets)
    if not all(0 < v < R for v in [t, a, b] + s3) or len(s3) != 3:
        raise ValueError("t, a, b and the three proof-of-knowledge secrets must lie in [1, r)")
    log = copy.deepcopy(log) if log is not None else PtauContributions(power=ptau.power)
    if log.power != ptau.power:
        raise ValueError("the log belongs to a file of another power")
    pok = ctx.fixed_base(1, F.frSeqToMontBytes([v for x, s in zip((t, a, b), s3) for v in (s, x * s % R)]))
    ch = challenge_bytes(transcript_hash(log, len(log.records), pok))
    arrays = {k: getattr(ptau, k) for k in ("tauG1", "tauG2", "alphaTauG1", "betaTauG1", "betaG2")}
    new, record = ctx.ptau_contribute(arrays, F.frToMontBytes(t), F.frToMontBytes(a), F.frToMontBytes(b),
                                      F.frSeqToMontBytes(s3), ch, power=ptau.power)
    assert record_pok_g1(record) == pok, "the record's proof-of-knowledge points are not the hashed ones"
    log.records.append(record)
    log.names.append(name)
    return Ptau(power=ptau.power, ceremonyPower=ptau.ceremonyPower, **new), log


def verifyPtau(ptau: Ptau, log: PtauContributions = None, multipliers=None, ctx=None):
    """Is `ptau` the powers of some tau, alpha, beta, and, with a log, do its records lead to it from the generators?  One
    g16_ptau_verify (include/g16hip.h) -> _lib.PtauReport: `.ok`, str() names every finding.  The challenges are re-derived
    from the records.  multipliers: 2^(power+1) - 2 ints in [1, 2^128); None draws them with `secrets`."""
    import secrets

    from ._lib import default_context
    ctx = ctx or default_context()
    if log is not None and log.power != ptau.power:
        raise ValueError("the log belongs to a file of another power")
    if multipliers is None:
        multipliers = b"".join((secrets.randbelow((1 << 128) - 1) + 1).to_bytes(16, "little")
                               for _ in range((2 << ptau.power) - 2))
    arrays = {k: getattr(ptau, k) for k in ("tauG1", "tauG2", "alphaTauG1", "betaTauG1", "betaG2")}
    return ctx.ptau_verify(arrays, None if log is None else log.records, None if log is None else challenges(log),
                           multipliers, power=ptau.power)
