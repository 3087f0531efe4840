"""The scalars every test of the per-point scaling runs (g16_points_scale_each_g1/g2, scale_each.cuh): the edge scalars of
the uniform scaling (tests/phase2_pictures.py) and those that matter once every lane splits a scalar of its own.  Python
integers only; owes nothing to the code under test."""
import functools

from oracle import bn254_ref as o
from tests import phase2_pictures as PP

R = o.R
LAMBDA = PP.LAMBDA


@functools.lru_cache(None)
def extreme_half_scalars():
    """k = k1 + k2 lambda for halves at the corners of what a split may return: one half at +-(2^127 - 1) beside a
    zero, a one and a long other half.  (The library's own split of such a k is another pair: the test asserts the
    identity and the bound, not these halves.)"""
    top = (1 << 127) - 1
    out = []
    for k1, k2 in ((top, 0), (-top, 0), (0, top), (0, -top), (top, 1), (1, -top), (top, top), (top, -top), (-top, top),
                   (-top, -top)):
        out.append((k1 + k2 * LAMBDA) % R)
    return out


@functools.lru_cache(None)
def edge_scalars():
    """0, 1, r - 1; lambda, lambda^2; 1 - lambda (pure P - phi P), -1 - lambda (pure -(P + phi P)) and their negatives;
    the neighbours of 2^127 and 2^128, alone and times lambda; the scalars with the longest halves"""
    lam2 = LAMBDA * LAMBDA % R
    near = [(1 << e) + d for e in (127, 128) for d in (-1, 0, 1)]
    ks = PP.edge_scalars() + [lam2, R - lam2, (1 - LAMBDA) % R, (LAMBDA - 1) % R, (-1 - LAMBDA) % R, (1 + LAMBDA) % R]
    ks += near + [x * LAMBDA % R for x in near] + [R - x for x in near]
    ks += extreme_half_scalars()
    seen, out = set(), []
    for k in ks:
        if k not in seen:
            seen.add(k)
            out.append(k)
    return out


def powers_of_two():
    return [1 << i for i in range(254)]


def random_scalars(count, seed):
    rng = o.SplitMix64(seed)
    return [rng.fr() for _ in range(count)]
