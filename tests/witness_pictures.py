"""Circuits and witnesses with planted defects for the witness check (g16_witness_check), and the integer model of what
it must report.  Plain Python integers over a circuit_audit_pictures.Circuit-style constraint list; the model owes
nothing to the library.

    model(circuit, witness, form)   the full report: counts, first indices, the ordered list, the three sums
    encode(values, form)            residues -> the bytes the library is handed (raw patterns pass through unchanged)
    planted(specs, ...)             a satisfied circuit in which exactly a chosen set of constraints can be broken
    broken(pc, which)               its witness with the constraints `which` broken

A planted circuit: wire 0 is the constant 1, a few BASE wires carry fixed values (0, 1 and r - 1 among them), and every
constraint i that has a C row owns a FRESH wire that appears only there, with coefficient 1.  A, B and the rest of C
draw on the base wires; the fresh wire is solved for.  Adding 1 to the fresh wire of constraint i changes (C z)_i and
nothing else: constraint i fails, every other one still holds."""
from dataclasses import dataclass, field

from oracle import bn254_ref as o
from tests.circuit_audit_pictures import Circuit

R = o.R
MONT_R = o.FR_MONT_R
MONT, STD = "mont", "std"
F_CANONICAL, F_ONE, F_CONSTRAINTS = 1, 2, 4
LIST = 16


def encode(values, form) -> bytes:
    """ints in [0, r) -> nvars x 32 bytes in `form`; an entry that is already 32 bytes is a raw pattern and stays"""
    out = []
    for v in values:
        if isinstance(v, (bytes, bytearray)):
            assert len(v) == 32
            out.append(bytes(v))
        else:
            assert 0 <= v < R
            out.append((v * MONT_R % R if form == MONT else v).to_bytes(32, "little"))
    return b"".join(out)


def one_bytes(form) -> bytes:
    return (MONT_R % R if form == MONT else 1).to_bytes(32, "little")


def lc(terms, z):
    return sum(v * z[w] for w, v in terms) % R


def model(circuit, witness, form) -> dict:
    """witness: ints (residues) or raw bytes (nvars x 32).  The report of g16_witness_check, entry for entry."""
    raw = witness if isinstance(witness, (bytes, bytearray)) else encode(witness, form)
    assert len(raw) == 32 * circuit.nvars
    pat = [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(circuit.nvars)]
    bad_values = [i for i, p in enumerate(pat) if p >= R]
    rep = {"failed": 0, "constraints": 1, "noncanonical_count": len(bad_values),
           "first_noncanonical": bad_values[0] if bad_values else None, "bad_count": 0, "first_bad": [],
           "az": 0, "bz": 0, "cz": 0}
    if raw[:32] != one_bytes(form):
        rep["failed"] |= F_ONE
    if bad_values:
        rep["failed"] |= F_CANONICAL
        rep["constraints"] = -1
        return rep
    inv = pow(MONT_R, -1, R)
    z = [p * inv % R if form == MONT else p for p in pat]
    sums = [(lc(A, z), lc(B, z), lc(C, z)) for A, B, C in circuit.constraints]
    bad = [i for i, (a, b, c) in enumerate(sums) if a * b % R != c]
    if bad:
        rep["failed"] |= F_CONSTRAINTS
        rep["constraints"] = 0
        rep["bad_count"] = len(bad)
        rep["first_bad"] = sorted(bad)[:LIST]
        rep["az"], rep["bz"], rep["cz"] = sums[min(bad)]
    return rep


@dataclass
class Planted:
    circuit: Circuit
    witness: list                     # residues: every constraint holds
    fresh: dict = field(default_factory=dict)   # constraint -> its fresh wire


FEW = (1, R - 1, 2, 5)                # coefficients of a circuit with a value dictionary


def planted(specs, seed=1, nbase=8, many_values=False, pad_to=0) -> Planted:
    """specs: per constraint (len A, len B, len C).  len C >= 1: the fresh wire and len C - 1 base terms; len C == 0: the
    constraint holds as 0 == 0 (A or B must be empty) and cannot be broken.  many_values: every coefficient is a fresh
    random residue (no value dictionary can form); else they come from FEW.  pad_to: explicit zero entries are added to
    the B rows, round robin, until the three matrices hold that many entries (a dictionary needs >= 1024)."""
    rng = o.SplitMix64(seed)
    base = [0, 1, R - 1] + [rng.fr() for _ in range(nbase - 3)]
    nvars = 1 + nbase + len(specs)
    z = [1] + base + [0] * len(specs)
    coeff = (lambda: rng.fr() or 1) if many_values else (lambda: FEW[rng.next() % len(FEW)])
    wire = lambda: 1 + rng.next() % nbase                                     # noqa: E731
    cons, fresh = [], {}
    for i, (la, lb, lcn) in enumerate(specs):
        A = [(wire(), coeff()) for _ in range(la)]
        B = [(wire(), coeff()) for _ in range(lb)]
        C = [(wire(), coeff()) for _ in range(max(lcn - 1, 0))]
        if lcn:
            f = 1 + nbase + i
            z[f] = (lc(A, z) * lc(B, z) - lc(C, z)) % R
            C.insert(rng.next() % (len(C) + 1), (f, 1))
            fresh[i] = f
        else:
            assert la == 0 or lb == 0, "a constraint without a C row must have an empty factor"
        cons.append((A, B, C))
    nnz = sum(len(A) + len(B) + len(C) for A, B, C in cons)
    for k in range(max(pad_to - nnz, 0)):
        cons[k % len(cons)][1].append((wire(), 0))
    c = Circuit(nvars, 1, cons)
    assert all(lc(A, z) * lc(B, z) % R == lc(C, z) for A, B, C in cons)
    return Planted(c, z, fresh)


def broken(pc: Planted, which) -> list:
    z = list(pc.witness)
    for i in which:
        z[pc.fresh[i]] = (z[pc.fresh[i]] + 1) % R
    return z


def plain_specs(ncons):
    """`ncons` short constraints: one to three terms a side, every one breakable"""
    return [(1 + i % 3, 1 + (i // 3) % 2, 1 + i % 2) for i in range(ncons)]


# every bin of spmv_params.hpp on each of the three matrices, and the looping last bin
BIN_LENGTHS = (0, 1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 300)


def bin_specs():
    specs = []
    for L in BIN_LENGTHS:
        specs.append((L, 2, 2))                   # A of length L (L == 0: 0 * Bz == Cz must hold)
        specs.append((3, L, 1))
        specs.append((0 if L == 0 else 2, 2, L))  # C of length L (L == 0: an empty C row, 0 == 0)
    return specs


def sizes_pictures(pc: Planted):
    """name -> set of broken constraints, for a planted circuit whose constraints can all be broken: none, single
    failures at 0, at each side of the bitmap-word, wave and workgroup boundaries that exist, and at the last row; 15,
    16 and 17 failures; every row"""
    n = pc.circuit.ncons
    assert len(pc.fresh) == n
    pics = {"satisfied": ()}
    for at in sorted({0, n - 1} | {b + d for b in (32, 64, 256, 512) for d in (-1, 0) if b + d < n}):
        pics[f"single_{at}"] = (at,)
    for k in (15, 16, 17):
        if k <= n:                    # spread over the rows, first and last included (k distinct ones: the step is >= 1)
            pics[f"many_{k}"] = tuple(sorted({j * (n - 1) // (k - 1) for j in range(k)}))
            assert len(pics[f"many_{k}"]) == k
    pics["all"] = tuple(range(n))
    return pics


def operands():
    """products that hold only mod r, zero products against non-zero sums and the converse, the values 0, 1, r - 1"""
    # wires: 0 = one, 1 = 0, 2 = 1, 3 = r - 1, 4 = 7
    z = [1, 0, 1, R - 1, 7]
    w = lambda i: [(i, 1)]                                                    # noqa: E731
    cons = [(w(3), w(3), w(2)),           # (r - 1)^2 == 1 only mod r                holds
            (w(1), w(4), w(4)),           # 0 * 7 against 7                           fails
            (w(4), w(4), w(1)),           # 49 against 0                              fails
            (w(1), w(1), w(1)),           # 0 * 0 == 0                                holds
            (w(3), w(2), w(3)),           # (r - 1) * 1 == r - 1                      holds
            (w(3), w(4), [(4, R - 1)]),   # (r - 1) * 7 == -7                         holds
            (w(2), w(2), w(3))]           # 1 against r - 1                           fails
    return Circuit(5, 1, cons), z
