"""tests/msm_pictures.py on the CPU: every picture that tests/test_gpu_msm_tail_edges.py runs fits its window, reaches
the additions it is built for (the log-space walk), the knob sets cover every reduce2 / fold form of the launch plan, and
the closed-form expected values agree with the oracle's naive MSM."""
from collections import Counter, defaultdict

import pytest

from oracle import bn254_ref as o
from tests import inputs as I
from tests import msm_pictures as mp
from tests.test_device_headers_cpu import shim  # noqa: F401  (the fixture that builds and loads the CPU shim)
from tests.test_msm_plan_cpu import (CLASSES, CLASSES_QUAD, MERGED, NARROW, PLAIN, QUAD64, QUAD128, WAVE, WIDE, run_plan)

COMBOS = [(registered, is_g1) for registered in (False, True) for is_g1 in (True, False)]
KINDS = ("inf", "equal", "opposite")


@pytest.fixture(scope="module")
def realised():
    """{(knob set index, registered, is_g1): [(picture, geometry, (scalars, logs, infinities)), ...]}, built once"""
    return {(i, registered, is_g1): list(mp.cases(knobs, families, registered, is_g1))
            for i, (knobs, families) in enumerate(mp.KNOB_SETS) for registered, is_g1 in COMBOS}


@pytest.fixture(scope="module")
def walked(realised):
    return {key: [(pic, g, data, mp.walk(g, data)) for pic, g, data in runs] for key, runs in realised.items()}


def test_class_bucket_restatement(shim):  # noqa: F811
    """msm_class_bucket as restated here: the shim's own check of the header, then bucket <-> magnitude both ways"""
    import ctypes
    shim.shim_class_buckets_check.restype = ctypes.c_uint32
    for c in (15, 16, 20):
        assert shim.shim_class_buckets_check(c) == 0
        h, seen = 1 << (c - 1), Counter()
        for t in range(1, h + 1):
            b, sel = mp.class_bucket(t, c)
            assert mp.class_weight(b, c) << sel == t and sel in (0, 1)
            seen[b] += 1
        nb = h // 2 + h // 8 + h // 32 + h // 64
        assert sorted(seen) == list(range(nb)) and set(seen.values()) <= {1, 2}
        assert all(mp.class_bucket(mp.class_weight(b, c), c) == (b, 0) for b in range(nb))


def test_every_picture_fits_its_window(realised):
    names = set()
    for (i, registered, is_g1), runs in realised.items():
        assert runs, (i, registered, is_g1)
        for pic, g, (scalars, logs, infs) in runs:
            where = (mp.knob_id(mp.KNOB_SETS[i][0]), registered, is_g1, pic.name)
            names.add(pic.name)
            n = len(scalars)
            assert g.n == n == len(logs) and 1 <= n <= 1 << 14, where
            assert all(0 < s < o.R for s in scalars) and all(0 <= k < o.R for k in logs), where
            assert all(logs[j] == 0 for j in infs) and all(0 <= j < n for j in infs), where
            for s in scalars:
                d = mp.digits(s, g.c, g.nwin)
                assert d and all(1 <= mag <= g.H and w < g.nwin for w, mag, _ in d), where
                if pic.family != "every" and not pic.name.startswith("with_infinity_points.every"):
                    assert len(d) == 1 and not d[0][2], where         # one positive digit: one bucket, the point as given
            if pic.family == "infpts":
                assert 3 * len(infs) >= n and (not registered or len(infs) * 100 >= mp.INF_COMPACT_PCT * n), where
            if pic.family == "heavy":
                extra = (max(Counter(scalars).values()) - 1) // g.seg
                assert (extra >= mp.HEAVY_MIN) == (not pic.name.endswith(".thread")) and extra >= 1, where
    # every picture of the list runs somewhere
    assert names == {p.name for p in mp.pictures()}, {p.name for p in mp.pictures()} - names


def test_walk_adds_up_and_reaches_what_each_picture_is_built_for(walked):
    for (i, registered, is_g1), runs in walked.items():
        for pic, g, (scalars, logs, infs), t in runs:
            where = (mp.knob_id(mp.KNOB_SETS[i][0]), registered, is_g1, pic.name, {k: dict(v) for k, v in t.items()})
            # the walk is a faithful regrouping of the sum (this is a check OF the walk, not an expected value)
            assert t["result"]["log"] == sum(s * k for s, k in zip(scalars, logs)) % o.R, where
            for cell, kind in pic.reach:
                assert t[cell][kind] >= 1, (cell, kind, where)
            if pic.name == "total_is_infinity":
                assert t["result"]["log"] == 0 and any(t[c]["opposite"] for c in t), where


def test_every_stage_of_every_knob_set_meets_all_three_kinds(walked):
    for i, (knobs, families) in enumerate(mp.KNOB_SETS):
        for registered, is_g1 in COMBOS:
            seen = defaultdict(Counter)
            for pic, g, data, t in walked[(i, registered, is_g1)]:
                for cell, kinds in t.items():
                    seen[mp.coarse(cell)].update(kinds)
            # a merged set of one slice (the default window of a small registered set) leaves its fold nothing to add
            # but infinities: the fold is held where a relation picture applies
            related = any(pic.family == "relations" for pic, g, data, t in walked[(i, registered, is_g1)])
            stages = ["reduce1", "r2"] + (["fold"] if related else []) + (["heavy"] if "heavy" in families else [])
            for stage in stages:
                for kind in KINDS:
                    assert seen[stage][kind] >= 1, (mp.knob_id(knobs), registered, is_g1, stage, kind, dict(seen[stage]))
            if "heavy" in families:                                   # both phases of msm_heavy
                cells = {c for pic, g, data, t in walked[(i, registered, is_g1)] for c in t}
                assert {"heavy1", "heavy2"} <= cells


def test_knob_sets_cover_the_plan(shim, realised):  # noqa: F811
    """the plans of the C++ header for every (knob set, set kind, group, picture size) that runs"""
    r2 = defaultdict(set)        # (variant, is_g1) -> {per == 1, per > 1}
    folds, rcs = set(), set()
    for (i, registered, is_g1), runs in realised.items():
        for pic, g, (scalars, _, _) in runs:
            p = run_plan(shim, len(scalars), registered, is_g1, False, mp.KNOB_SETS[i][0])
            assert p.raw == g.plan.raw, (mp.KNOB_SETS[i][0], registered, is_g1, pic.name)
            slots = p.r2_lds
            r2[(p.r2, is_g1)].add(-(-p.cps // slots) > 1)
            folds.add((p.fold, is_g1))
            rcs.add(p.rc)
    for variant in (QUAD64, WIDE, NARROW, WAVE):
        for is_g1 in (True, False):
            assert r2[(variant, is_g1)] == {False, True}, (mp.R2_NAME[variant], is_g1, r2[(variant, is_g1)])
    # the 128-slot kernel is launched from 512 chunks per set on, so its slots never hold fewer than 4 chunks; G1 only
    assert r2[(QUAD128, True)] == {True} and (QUAD128, False) not in r2
    assert folds == {(f, g1) for f in (CLASSES_QUAD, CLASSES, MERGED, PLAIN) for g1 in (True, False)}
    assert {2, 4, 16} <= rcs


def test_expected_values_equal_the_naive_msm(realised):
    """(sum s_i k_i) G against the definition sum s_i P_i (oracle/bn254_ref.py: Curve.msm_naive) for every picture of
    at most 64 points, once per picture and group"""
    done = set()
    for (i, registered, is_g1), runs in realised.items():
        for pic, g, (scalars, logs, infs) in runs:
            if len(scalars) > 64 or (pic.name, is_g1) in done:
                continue
            done.add((pic.name, is_g1))
            C, gen, enc = (o.G1, o.GEN1, o.g1_to_bytes) if is_g1 else (o.G2, o.GEN2, o.g2_to_bytes)
            points = {k: C.mul(k, gen) for k in set(logs)}
            got = enc(C.msm_naive(scalars, [points[k] for k in logs]))
            assert got == I.expected_from_logs(1 if is_g1 else 2, scalars, logs), (pic.name, is_g1)
    assert len(done) >= 80
