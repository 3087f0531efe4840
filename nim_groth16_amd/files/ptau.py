"""The `.ptau` file of a powers-of-tau ceremony (snarkjs), as far as the circuit audit reads it (include/g16hip.h,
g16_circuit_audit).  The iden3 container with magic `ptau`, version 1:

    section 1   n8 u32 | the prime q (n8 bytes) | power u32 | ceremonyPower u32
    section 2   tauG1        2^(power+1) - 1 G1 points   tau^k gen1
    section 3   tauG2        2^power G2 points           tau^k gen2
    section 4   alphaTauG1   2^power G1 points           alpha tau^k gen1
    section 5   betaTauG1    2^power G1 points           beta tau^k gen1
    section 6   betaG2       one G2 point                beta gen2
    section 7   the contribution log, in THIS project's layout (phase1.py; parsePtauContributions / contributionsSection):
                count u32 | count records of 1216 bytes (g16_ptau_contribution) | count names, each length u32 | UTF-8
    sections 12-15 (the Lagrange forms a prepared file carries) are skipped if present; parsePtau skips section 7 too

Points are uncompressed, little-endian, in Montgomery form: byte for byte what a .zkey's point sections hold and what
the GPU library takes, so they are passed through unparsed.

This is the maintainers' reading of the format.  Like the .zkey writer it is NOT pinned against a file that snarkjs
wrote: the reference has no .ptau reader and none was at hand."""
from __future__ import annotations

import struct
from dataclasses import dataclass

from .. import bn128 as F
from .container import parseContainer, parsePrimeField, writeContainer


@dataclass
class Ptau:
    power: int
    tauG1: bytes            # (2^(power+1) - 1) x 64 bytes
    tauG2: bytes            # 2^power x 128
    alphaTauG1: bytes       # 2^power x 64
    betaTauG1: bytes        # 2^power x 64
    betaG2: bytes           # 128
    ceremonyPower: int = None


_SECTIONS = ((2, "tauG1", 64), (3, "tauG2", 128), (4, "alphaTauG1", 64), (5, "betaTauG1", 64), (6, "betaG2", 128))


def _count(name: str, power: int) -> int:
    return {"tauG1": (2 << power) - 1, "betaG2": 1}.get(name, 1 << power)


def parsePtau(fname: str) -> Ptau:
    sec = parseContainer("ptau", 1, fname)
    s1 = sec[1][0]
    n8, q, pos = parsePrimeField(s1, 0)
    assert n8 == 32 and q == F.primeP, "expecting the alt-bn128 curve"
    assert len(s1) == 4 + n8 + 8, "unexpected section length"
    power, ceremony = struct.unpack_from("<II", s1, pos)
    assert power <= 28 and power <= ceremony, "power out of range"
    got = {}
    for sid, name, psz in _SECTIONS:
        assert sid in sec, f"section {sid} ({name}) is missing"
        s = sec[sid][0]
        assert len(s) == psz * _count(name, power), f"unexpected length of section {sid} ({name})"
        got[name] = s.tobytes()
    return Ptau(power=power, ceremonyPower=ceremony, **got)


def writePtau(fname: str, ptau: Ptau, extraSections=()) -> None:
    """extraSections: (id, bytes) pairs written after section 6, e.g. the contributions (7) of a real ceremony"""
    for _, name, psz in _SECTIONS:
        assert len(getattr(ptau, name)) == psz * _count(name, ptau.power), f"wrong length of {name}"
    cer = ptau.power if ptau.ceremonyPower is None else ptau.ceremonyPower
    s1 = struct.pack("<I", 32) + F.primeP.to_bytes(32, "little") + struct.pack("<II", ptau.power, cer)
    writeContainer("ptau", 1, fname, [(1, s1)] + [(sid, getattr(ptau, name)) for sid, name, _ in _SECTIONS] +
                   list(extraSections))


PTAU_RECORD_BYTES = 1216


def contributionsSection(records, names) -> bytes:
    """section 7 from the records (1216 bytes each) and the contributors' names: pass it to writePtau as
    extraSections=[(7, ...)]"""
    assert len(records) == len(names) and all(len(r) == PTAU_RECORD_BYTES for r in records)
    out = [struct.pack("<I", len(records))] + [bytes(r) for r in records]
    for name in names:
        raw = name.encode("utf-8")
        out.append(struct.pack("<I", len(raw)) + raw)
    return b"".join(out)


def parsePtauContributions(fname: str):
    """-> (records, names) of section 7, or None if the file has none.  ValueError if the section is not in this project's
    layout (a snarkjs-written file: its records are not ours, see phase1.py)."""
    sec = parseContainer("ptau", 1, fname)
    if 7 not in sec:
        return None
    s = bytes(sec[7][0])
    if len(s) < 4:
        raise ValueError("section 7 is shorter than its count")
    (count,) = struct.unpack_from("<I", s, 0)
    pos = 4 + PTAU_RECORD_BYTES * count
    if len(s) < pos:
        raise ValueError("section 7 is truncated: it ends inside its records")
    records = [s[4 + PTAU_RECORD_BYTES * j:4 + PTAU_RECORD_BYTES * (j + 1)] for j in range(count)]
    names = []
    for _ in range(count):
        if len(s) < pos + 4:
            raise ValueError("section 7 is truncated: it ends inside its names")
        (ln,) = struct.unpack_from("<I", s, pos)
        if len(s) < pos + 4 + ln:
            raise ValueError("section 7 is truncated: it ends inside its names")
        try:
            names.append(s[pos + 4:pos + 4 + ln].decode("utf-8"))
        except UnicodeDecodeError:
            raise ValueError("section 7: a name is not UTF-8") from None
        pos += 4 + ln
    if pos != len(s):
        raise ValueError("section 7: bytes left over after the names")
    return records, names
