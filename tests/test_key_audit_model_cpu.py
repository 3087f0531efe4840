"""The integer model of the key audit (tests/key_audit_pictures.py) held to itself, and the compile-time half of the
order-r kernel: the digit schedule of nim_groth16_amd/csrc/subgroup_plan.hpp, built with g++ and evaluated here with
Python integers.  No GPU."""
import os
import re
import subprocess

import pytest

from oracle import bn254_ref as o
from tests import key_audit_pictures as KA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOTHING = {"failed": 0, "spec_infinity": 0, "relation": [1, 1, 1],
           "first_bad": [[None] * 3 for _ in KA.SECTIONS], "bad_count": [[0] * 3 for _ in KA.SECTIONS]}


def test_clean_toy_key_reports_nothing():
    pics = KA.key_pictures()
    assert pics["clean"].report == NOTHING
    assert pics["clean_section4"].report == NOTHING
    assert pics["clean_no_vk"].report == NOTHING
    assert pics["clean_no_multipliers"].report == dict(NOTHING, relation=[-1, 1, 1])
    # the toy key is the oracle's: its own proof verifies against it
    zk = KA.toy_zkey()
    assert o.verify_proof(zk, o.generate_proof_with_mask(zk, o.TOY_WITNESS, 3, 4))


def _expect(name, **changes):
    """the report of picture `name` is the clean one except for `changes`: section -> (check, first, count), or a
    top-level entry"""
    want = {k: (v if not isinstance(v, list) else [list(x) if isinstance(x, list) else x for x in v])
            for k, v in NOTHING.items()}
    for key, val in changes.items():
        if key in KA.SECTIONS:
            check, first, count = val
            s = KA.SECTIONS.index(key)
            want["first_bad"][s][check] = first
            want["bad_count"][s][check] = count
        else:
            want[key] = val
    got = KA.key_pictures()[name].report
    assert got == want, (name, got, want)


def test_each_planted_defect_changes_exactly_its_entries():
    C, V, S = KA.CANONICAL, KA.CURVE, KA.SUBGROUP
    _expect("a1_alias", pointsA1=(0, 7, 1), failed=C)
    _expect("h1_off_curve", pointsH1=(1, 0, 1), failed=V)
    _expect("c1_coord_is_p", pointsC1=(0, 2, 1), failed=C)
    _expect("ic_off_curve", pointsIC=(1, 1, 1), failed=V)
    _expect("ic_off_curve_no_vk")                                        # the section is not looked at
    _expect("b2_small_order", pointsB2=(2, 3, 1), failed=S, relation=[-1, 1, 1])
    _expect("b2_full_twist", pointsB2=(2, 7, 1), failed=S, relation=[-1, 1, 1])
    _expect("b2_small_plus_g", pointsB2=(2, 0, 1), failed=S, relation=[-1, 1, 1])
    _expect("b2_alias_c1", pointsB2=(0, 4, 1), failed=C, relation=[-1, 1, 1])
    _expect("b2_alias_of_small", pointsB2=(0, 4, 1), failed=C, relation=[-1, 1, 1])       # precedence: counted once
    _expect("b1_alias_of_off_curve", pointsB1=(0, 5, 1), failed=C, relation=[-1, 1, 1])   # precedence: counted once
    _expect("gamma2_small_order", gamma2=(2, 0, 1), failed=S)
    _expect("beta2_off_curve", beta2=(1, 0, 1), failed=V, relation=[1, -1, 1])
    _expect("alpha1_alias", alpha1=(0, 0, 1), failed=C)
    _expect("two_sections", pointsA1=(1, 0, 2), pointsB2=(2, 2, 1), failed=V | S, relation=[-1, 1, 1])
    for sfx in ("", "_section4"):
        last = len(KA.toy_key().coeffs) - 1
        _expect("coeff_is_r" + sfx, coeffs=(0, 1, 1), failed=C)
        _expect("coeff_all_ones" + sfx, coeffs=(0, last, 1), failed=C)
        _expect("coeff_r_minus_1" + sfx)
        _expect("coeff_two" + sfx, coeffs=(0, 0, 2), failed=C)
    R_ = KA.RELATION
    _expect("rel_b1_swapped", relation=[0, 1, 1], failed=R_)
    _expect("rel_cancel_bit127", relation=[0, 1, 1], failed=R_)
    _expect("rel_cancel_equal_z")                                        # the check IS the equation: it holds
    _expect("rel_cancel_weighted")
    _expect("rel_b1_inf", relation=[0, 1, 1], failed=R_)
    _expect("rel_beta1_doubled", relation=[1, 0, 1], failed=R_)
    _expect("rel_delta2_inf", relation=[1, 1, 0], spec_infinity=1 << 5, failed=R_ | KA.SPEC_INFINITY)


def test_array_pictures_cover_sizes_positions_and_kinds():
    pics = KA.array_pictures()
    assert len({p.name for p in pics}) == len(pics)
    for group in (1, 2):
        mixed = [p for p in pics if p.name.startswith(f"g{group}_mixed_")]
        assert sorted(len(p.raw) // (64 * group) for p in mixed) == sorted(KA.SIZES)
        seen = [0, 0, 0]
        for p in mixed:
            seen = [a + b for a, b in zip(seen, p.bad_count)]
        assert seen[0] and seen[1] and (seen[2] if group == 2 else not seen[2])
    big = next(p for p in pics if p.name == "g2_mixed_301")
    assert sum(big.bad_count) >= 6 and KA.positions(301) == [0, 7, 9, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300]
    # precedence: the alias of a point of small order is not canonical and nothing else
    p = next(p for p in pics if p.name == "g2_alias_of_small_at_3")
    assert (p.first_bad, p.bad_count) == ([3, None, None], [1, 0, 0])
    p = next(p for p in pics if p.name == "g2_small_at_255_256")
    assert (p.first_bad, p.bad_count) == ([None, None, 255], [0, 0, 2])


def test_relation_pictures():
    pics = KA.relation_pictures()
    for p in pics:
        kind = p.name.rsplit("_", 1)[0]
        if kind in KA.RELATION_KINDS:
            assert p.result == KA.RELATION_KINDS[kind], p.name
    # in log space the verdict is the linear form: the pairing agrees with it on every picture
    for p in pics:
        lin = sum(z * (x - y) for z, x, y in zip(p.multipliers, p.a, p.b)) % KA.R
        assert p.result == (1 if lin == 0 else 0), p.name


def test_header_declares_the_three_calls():
    text = open(os.path.join(ROOT, "include", "g16hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("g16_points_audit_g1", "g16_points_audit_g2", "g16_points_pairs_check", "g16_key_audit"):
        assert re.search(r"\bint32_t\s+" + name + r"\s*\(", code), name
    assert "g16_key_report" in code and "G16_AUDIT_SPEC_INFINITY" in code
    assert "CANNOT establish" in text                       # ... and says what no audit can tell
    from nim_groth16_amd import _lib
    assert tuple(_lib.AUDIT_SECTIONS) == KA.SECTIONS
    assert (_lib.AUDIT_CANONICAL, _lib.AUDIT_CURVE, _lib.AUDIT_SUBGROUP, _lib.AUDIT_RELATION,
            _lib.AUDIT_SPEC_INFINITY) == (KA.CANONICAL, KA.CURVE, KA.SUBGROUP, KA.RELATION, KA.SPEC_INFINITY)
    for k, name in enumerate(KA.SECTIONS):
        m = re.search(r"enum\s*\{(.*?)\}", code, flags=re.S)
        assert m.group(1).split(",")[k].split("=")[0].strip() == "G16_SEC_" + re.sub(r"points", "POINTS_", name).upper()


PLAN_MAIN = r"""
#include <cstdio>
#include "subgroup_plan.hpp"
int main() {
  const g16::SubgroupPlan& p = g16::SUBGROUP_PLAN;
  std::printf("%d %d\n", p.nsteps, p.ndbl);
  for (int s = 0; s < p.nsteps; ++s) std::printf("%d %d\n", (int)p.step[s].dbls, (int)p.step[s].digit);
  return 0;
}
"""


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """the schedule as g++ builds it: [(doublings, digit)]"""
    tmp = tmp_path_factory.mktemp("plan")
    src, exe = tmp / "plan.cpp", tmp / "plan"
    src.write_text(PLAN_MAIN)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "nim_groth16_amd", "csrc"),
                           str(src), "-o", str(exe)])
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    nsteps, ndbl = map(int, lines[0].split())
    steps = [tuple(map(int, ln.split())) for ln in lines[1:1 + nsteps]]
    assert len(steps) == nsteps and sum(d for d, _ in steps) == ndbl
    return steps


def test_subgroup_plan_evaluates_to_r(plan):
    k = 1                                                   # the ladder starts at acc = Q
    for dbls, digit in plan:
        assert dbls >= 2 and digit in (1, -1)               # non-adjacent form
        k = (k << dbls) + digit
    assert k == o.R
    assert sum(d for d, _ in plan) == o.R.bit_length() - 1 or sum(d for d, _ in plan) == o.R.bit_length()
    # fewer additions than the binary ladder has
    assert len(plan) < bin(o.R).count("1") - 1


def test_subgroup_plan_prefixes_modulo_the_small_order(plan, capsys):
    """Which exceptional additions the point of order 10069 reaches: before an addition the accumulator holds k Q, and the
    addition is +-Q.  k = 0 mod 10069: the accumulator is infinity; k = +-digit: equal or opposite operands.  Printed for the
    record; what is asserted is that the last addition of an honest point, and only it, meets opposite operands mod r."""
    from tests import device_ops as D
    n = D.SMALL_ORDER
    k, hits = 1, []
    with capsys.disabled():
        print()
        for s, (dbls, digit) in enumerate(plan):
            k <<= dbls
            m = k % n
            tag = "infinity" if m == 0 else "equal" if (m - digit) % n == 0 else "opposite" if (m + digit) % n == 0 else ""
            print(f"step {s:3d}: {dbls:2d} doublings, digit {digit:+d}, accumulator {m:5d} Q (mod {n}) {tag}")
            if tag:
                hits.append((s, tag))
            honest = k % o.R
            assert ((honest + digit) % o.R == 0) == (s == len(plan) - 1)
            assert honest != 0 and (honest - digit) % o.R != 0
            k += digit
        print("exceptional additions of the order-%d point: %s" % (n, hits or "none"))
    assert k == o.R and k % n != 0                          # [r] small is not infinity: the verdict is "outside"
