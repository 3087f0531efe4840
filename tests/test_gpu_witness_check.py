"""g16_witness_check on the GPU against the integer model of tests/witness_pictures.py (held to synthetic.checkWitness and
to the oracle's toy circuit in tests/test_witness_check_cpu.py): every report must equal the model entry for entry.

The three forms the sums can be in (header comment of spmv.hip) are forced by the circuit and the witness form: a
Montgomery witness; a standard witness against a circuit with a value dictionary (few distinct coefficients, >= 1024
entries); a standard witness against one without (every coefficient distinct).  g16_r1cs_info says which one ran."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import bn254_ref as o
from tests import inputs as I
from tests import witness_pictures as WP
from tests.circuit_audit_pictures import Circuit, circuits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = o.R
FORMS = (WP.MONT, WP.STD)
COUNTS = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 513)


def _desc(circuit: Circuit, std_values=False, flavour=1):
    from nim_groth16_amd._lib import SCALARS_MONT, SCALARS_STD, R1csDesc
    rd = R1csDesc()
    rd.nvars, rd.npubs, rd.nconstraints, rd.flavour = circuit.nvars, circuit.npubs, circuit.ncons, flavour
    rd.flags = SCALARS_STD if std_values else SCALARS_MONT
    keep = []
    for k, ent in enumerate(circuit.triplets()):
        rows = np.array([e[0] for e in ent], dtype=np.uint32)
        cols = np.array([e[1] for e in ent], dtype=np.uint32)
        raw = (I.fr_std_bytes if std_values else I.fr_mont_bytes)([e[2] for e in ent])
        vals = ctypes.create_string_buffer(raw, len(raw)) if raw else ctypes.create_string_buffer(1)
        keep += [rows, cols, vals]
        rd.nnz[k] = len(ent)
        if ent:
            rd.row[k], rd.col[k] = rows.ctypes.data, cols.ctypes.data
            rd.val[k] = ctypes.cast(vals, ctypes.c_void_p).value
    return rd, keep


def _load(ctx, circuit, **kw):
    rd, keep = _desc(circuit, **kw)
    return ctx.r1cs_load(rd, keep)


def _same(system, circuit, witness, form, label, **kw):
    """the library's report of `witness` (ints or raw bytes) equals the model's, entry for entry"""
    raw = witness if isinstance(witness, (bytes, bytearray)) else WP.encode(witness, form)
    want = WP.model(circuit, raw, form)
    got = system.check(bytes(raw), mont=form == WP.MONT, **kw)
    assert got.as_dict() == want, (label, form, got.as_dict(), want)
    assert got.ok == (want["failed"] == 0)
    return got


def _pair(ctx, specs, seed, **kw):
    """the same constraint shapes twice: with a value dictionary (few coefficients, padded to >= 1024 entries) and
    without (every coefficient distinct); g16_r1cs_info must say so"""
    out = []
    for many in (False, True):
        pc = WP.planted(specs, seed=seed, many_values=many, pad_to=0 if many else 1100, **kw)
        system = _load(ctx, pc.circuit, std_values=many)          # (both forms of desc->flags on the way)
        info = system.info()
        assert info["nvars"] == pc.circuit.nvars and info["nconstraints"] == pc.circuit.ncons
        assert info["nnz"] == sum(len(m) for m in pc.circuit.triplets())
        assert (info["dict_values"] == 0) == many, info
        if not many:                                              # (some of) FEW and the explicit zeros of the padding
            assert info["dict_values"] == len({v for m in pc.circuit.triplets() for _, _, v in m}) <= 5
        out.append((pc, system))
    return out


@pytest.mark.parametrize("ncons", COUNTS)
def test_sizes_in_all_three_sum_forms(ctx, ncons):
    for pc, system in _pair(ctx, WP.plain_specs(ncons), seed=100 + ncons):
        dict_state = "dict" if system.info()["dict_values"] else "plain"
        for name, which in WP.sizes_pictures(pc).items():
            z = WP.broken(pc, which)
            for form in FORMS:
                rep = _same(system, pc.circuit, z, form, (ncons, dict_state, name))
                assert rep.bad_count == len(which) and rep.first_bad == sorted(which)[:16]
        system.destroy()


def test_row_shapes_hit_every_bin(ctx):
    specs = WP.bin_specs()
    assert {s[k] for s in specs for k in range(3)} >= set(WP.BIN_LENGTHS)
    for pc, system in _pair(ctx, specs, seed=9, nbase=40):
        c = pc.circuit
        assert any(not A and C for A, B, C in c.constraints) and any(not C for A, B, C in c.constraints)
        some = sorted(pc.fresh)[::5]
        for form in FORMS:
            assert _same(system, c, pc.witness, form, "bins").ok
            assert _same(system, c, WP.broken(pc, some), form, "bins broken").first_bad == some[:16]
            assert _same(system, c, WP.broken(pc, pc.fresh), form, "bins all").bad_count == len(pc.fresh)
        system.destroy()


def test_dup_nopriv_and_toy(ctx):
    cs = circuits()
    for std_values in (False, True):
        for name, witnesses in (("toy", (o.TOY_WITNESS, o.TOY_WITNESS[:6] + [78, 1001])),
                                ("dup", (o.TOY_WITNESS, [1, 0, 0, 0, 5, 13, 0, 0], [1, 9, 4, 7, 3, 1, 630, 630])),
                                ("nopriv", ([1, 2, 3], [1, 2, 4], [1, 0, 0]))):
            system = _load(ctx, cs[name], std_values=std_values)
            assert system.info()["dict_values"] == 0
            for z in witnesses:
                for form in FORMS:
                    _same(system, cs[name], [v % R for v in z], form, name)
            system.destroy()
    # the dup circuit: (3, 1) + (3, 2) act as 3 w3 and the pair (4, 5), (4, -5) cancels
    want = WP.model(cs["dup"], [1, 9, 4, 7, 3, 1, 630, 630], WP.STD)
    assert want["first_bad"] == [0] and want["cz"] == -9 + 4 + 630


def test_operands(ctx):
    c, z = WP.operands()
    for std_values in (False, True):
        system = _load(ctx, c, std_values=std_values)
        for form in FORMS:
            rep = _same(system, c, z, form, "operands")
            assert rep.first_bad == [1, 2, 6] and (rep.az, rep.bz, rep.cz) == (0, 7, 7)
            ok = list(z)
            ok[4] = 0                                             # 7 -> 0: constraints 1, 2 and 5 hold, 6 still fails
            assert _same(system, c, ok, form, "operands 2").first_bad == [6]
        system.destroy()


PATTERNS = {WP.STD: (R, R + 1, (1 << 256) - 1), WP.MONT: (R, (1 << 256) - 1)}


def test_canonical_pass_runs_first(ctx):
    for pc, system in _pair(ctx, WP.plain_specs(65), seed=65):
        c = pc.circuit
        nv = c.nvars
        z = WP.broken(pc, (3, 40))                                # the constraint pass would have something to say
        for form in FORMS:
            pats = [p.to_bytes(32, "little") for p in PATTERNS[form]]
            plants = [{i: p} for i in (0, nv // 2, nv - 1) for p in pats]
            plants += [{0: pats[0], nv - 1: pats[-1]}, {nv // 2: pats[-1], nv // 2 + 1: pats[0], nv - 1: pats[0]},
                       {i: pats[i % len(pats)] for i in range(nv)}]
            for plant in plants:
                w = list(z)
                for i, p in plant.items():
                    w[i] = p
                rep = _same(system, c, w, form, sorted(plant))
                assert rep.constraints == -1 and rep.noncanonical_count == len(plant)
                assert rep.first_noncanonical == min(plant) and rep.bad_count == 0 and rep.first_bad == []
                assert (rep.az, rep.bz, rep.cz) == (0, 0, 0)
                assert bool(rep.failed & WP.F_ONE) == (0 in plant)
        system.destroy()


def test_witness_zero_is_one(ctx):
    from nim_groth16_amd._lib import WITNESS_CANONICAL, WITNESS_CONSTRAINTS, WITNESS_ONE
    pc = WP.planted(WP.plain_specs(33), seed=7)
    system = _load(ctx, pc.circuit)
    rep = _same(system, pc.circuit, [(1 + R).to_bytes(32, "little")] + pc.witness[1:], WP.STD, "1 + r")
    assert rep.failed == WITNESS_CANONICAL | WITNESS_ONE and rep.constraints == -1
    for form in FORMS:
        rep = _same(system, pc.circuit, [2] + pc.witness[1:], form, "2")
        assert rep.failed == WITNESS_ONE and rep.constraints == 1           # no constraint reads wire 0 here
        rep = _same(system, pc.circuit, [2] + WP.broken(pc, (32,))[1:], form, "2 and a broken row")
        assert rep.failed == WITNESS_ONE | WITNESS_CONSTRAINTS and rep.first_bad == [32]
    # the other form's 1 is not this form's
    assert _same(system, pc.circuit, WP.encode(pc.witness, WP.STD), WP.MONT, "std 1 as mont").failed & WITNESS_ONE
    system.destroy()


def test_host_and_device_witness_two_contexts(ctx):
    import torch

    from nim_groth16_amd import Context
    other = Context(0)
    try:
        for pc, system in _pair(ctx, WP.plain_specs(257), seed=3):
            z = WP.broken(pc, range(0, 257, 9))
            for form in FORMS:
                raw = WP.encode(z, form)
                host = _same(system, pc.circuit, raw, form, "host")
                d_w = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
                torch.cuda.synchronize()
                for c in (ctx, other, ctx):
                    dev = system.check(d_w.data_ptr(), mont=form == WP.MONT, device=True, ctx=c)
                    assert dev.as_dict() == host.as_dict()
                    assert system.check(raw, mont=form == WP.MONT, ctx=c).as_dict() == host.as_dict()
            system.destroy()
    finally:
        other.close()


def test_system_outlives_its_context_and_the_reverse():
    from nim_groth16_amd import Context
    pc = WP.planted(WP.plain_specs(64), seed=5)
    a, b = Context(0), Context(0)
    s1, s2 = _load(a, pc.circuit), _load(a, pc.circuit)
    s1.destroy()                                                  # before its context
    a.close()
    assert _same(s2, pc.circuit, WP.broken(pc, (63,)), WP.STD, "after the creating context", ctx=b).first_bad == [63]
    s2.destroy()                                                  # after it
    b.close()


def _chain_key(ctx, m):
    from nim_groth16_amd import loadProvingKey
    from nim_groth16_amd.fake_setup import ToxicWaste, fakeCircuitSetup
    from nim_groth16_amd.synthetic import squaringChain
    r1cs, wit = squaringChain(m, seed=4)
    rng = o.SplitMix64(5)
    zk = fakeCircuitSetup(r1cs, ToxicWaste(*[rng.fr() for _ in range(5)]), 1, ctx)
    return r1cs, wit, zk, loadProvingKey(zk, ctx)


def test_a_check_changes_no_context_state(ctx):
    from nim_groth16_amd import bn128 as F
    r1cs, wit, zk, pk = _chain_key(ctx, 510)
    c = Circuit(r1cs.nWires, 1, r1cs.constraints)
    system = _load(ctx, c)
    try:
        wb, rb, sb = F.frSeqToMontBytes(wit), F.frToMontBytes(11), F.frToMontBytes(13)
        before = pk.prove(wb, r=rb, s=sb)
        bad = list(wit)
        bad[100] = (bad[100] + 1) % R
        for z in (wit, bad):
            for form in FORMS:
                _same(system, c, z, form, "between proofs")
        assert pk.prove(wb, r=rb, s=sb) == before
    finally:
        system.destroy()
        pk.destroy()


def test_r1cs_create_rejects(ctx):
    from nim_groth16_amd._lib import G16_EINVAL, G16Error, R1csDesc
    c = circuits()["toy"]

    def refused(edit, words, **kw):
        rd, keep = _desc(c, **kw)
        edit(rd, keep)
        with pytest.raises(G16Error) as e:
            ctx.r1cs_load(rd, keep)
        assert e.value.code == G16_EINVAL
        for w in words:
            assert w in str(e.value), (w, str(e.value))

    def row_out(rd, keep):
        keep[3][1] = c.ncons                                      # matrix B (keep[3] = its rows), entry 1
    refused(row_out, ("r1cs matrix 1 entry 1 out of range",))

    def col_out(rd, keep):
        keep[7][2] = c.nvars                                      # matrix C's wires, entry 2
    refused(col_out, ("r1cs matrix 2 entry 2 out of range",))
    for std_values in (False, True):
        def big(rd, keep):
            ctypes.memmove(ctypes.addressof(keep[2]) + 0, R.to_bytes(32, "little"), 32)    # matrix A's values, entry 0
        refused(big, ("r1cs matrix 0 entry 0", "not canonical"), std_values=std_values)

    def flags(rd, keep):
        rd.flags = 2
    refused(flags, ("flags",))

    def flavour(rd, keep):
        rd.flavour = 7
    refused(flavour, ("flavour",))

    def null(rd, keep):
        rd.val[1] = None
    refused(null, ("null",))
    with pytest.raises(G16Error) as e:
        ctx._check(ctx._lib.g16_r1cs_create(ctx._h, None, ctypes.byref(ctypes.c_void_p())))
    assert e.value.code == G16_EINVAL
    rd, keep = _desc(c)
    assert ctx._lib.g16_r1cs_create(ctx._h, ctypes.byref(rd), None) == G16_EINVAL
    # no constraint at all is legal: every check reports constraints = 1
    empty = Circuit(3, 1, [])
    system = _load(ctx, empty)
    assert system.info() == {"nvars": 3, "nconstraints": 0, "nnz": 0, "dict_values": 0}
    for form in FORMS:
        assert _same(system, empty, [1, 5, 6], form, "empty").constraints == 1
        assert _same(system, empty, [1, R.to_bytes(32, "little"), 6], form, "empty, not canonical").constraints == -1
    # flags of the check itself
    from nim_groth16_amd._lib import WitnessReportC
    rep = WitnessReportC()
    assert ctx._lib.g16_witness_check(ctx._h, system._h, bytes(96), 4, ctypes.byref(rep)) == G16_EINVAL
    assert ctx._lib.g16_witness_check(ctx._h, system._h, None, 1, ctypes.byref(rep)) == G16_EINVAL
    assert ctx._lib.g16_witness_check(ctx._h, None, bytes(96), 1, ctypes.byref(rep)) == G16_EINVAL
    system.destroy()


@pytest.mark.parametrize("circuit", ["chain510", "poseidon10"])
def test_verdict_agrees_with_the_prover(ctx, circuit):
    """a clean report and a proof that verifies; one wire changed: exactly the model's constraints, and no proof"""
    from nim_groth16_amd import (Mask, Witness, extractVKey, generateProofWithMask, loadProvingKey, verifyProof,
                                 witnessCheck)
    from nim_groth16_amd import bn128 as F
    from nim_groth16_amd.fake_setup import ToxicWaste, fakeCircuitSetup
    from nim_groth16_amd.synthetic import poseidonMerkle, squaringChain
    r1cs, wit = squaringChain(510, seed=4) if circuit == "chain510" else poseidonMerkle(10, seed=4)
    rng = o.SplitMix64(21)
    zk = fakeCircuitSetup(r1cs, ToxicWaste(*[rng.fr() for _ in range(5)]), 1, ctx)
    pk = loadProvingKey(zk, ctx)
    c = Circuit(r1cs.nWires, r1cs.nPubIn + r1cs.nPubOut, r1cs.constraints)
    vk = extractVKey(zk)
    bad = list(wit)
    bad[len(wit) // 2] = (bad[len(wit) // 2] + 1) % R
    try:
        for z, clean in ((wit, True), (bad, False)):
            want = WP.model(c, z, WP.STD)
            assert (want["failed"] == 0) == clean and (clean or want["bad_count"] >= 1)
            for std in (False, True):
                wt = Witness("bn128", len(z), F.frSeqToStdBytes(z) if std else F.frSeqToMontBytes(z), std=std)
                rep = witnessCheck(r1cs, wt, ctx)
                assert rep.as_dict() == WP.model(c, z, WP.STD if std else WP.MONT), (circuit, clean, std)
                pr = generateProofWithMask(0, False, zk, wt, Mask(rng.fr(), rng.fr()), ctx, pkey=pk)
                assert verifyProof(vk, pr, ctx) == clean == rep.ok
    finally:
        pk.destroy()


def test_both_tools_refuse_a_broken_witness(ctx, tmp_path):
    from nim_groth16_amd.fake_setup import ToxicWaste, fakeCircuitSetup
    from nim_groth16_amd.files import writeR1CS, writeWitness, writeZKey
    from nim_groth16_amd.synthetic import squaringChain
    from tests.test_gpu_native_cli import _build
    r1cs, wit = squaringChain(62, seed=4)
    rng = o.SplitMix64(77)
    zk = fakeCircuitSetup(r1cs, ToxicWaste(*[rng.fr() for _ in range(5)]), 1, ctx)
    zpath, rpath = str(tmp_path / "c.zkey"), str(tmp_path / "c.r1cs")
    writeZKey(zpath, zk)
    writeR1CS(rpath, r1cs)
    good, bad = str(tmp_path / "good.wtns"), str(tmp_path / "bad.wtns")
    writeWitness(good, wit)
    broken = list(wit)
    broken[2 + 37] = (broken[2 + 37] + 1) % R            # w_37: the C row of constraint 36, A and B of constraint 37
    writeWitness(bad, broken)
    c = Circuit(r1cs.nWires, 1, r1cs.constraints)
    assert WP.model(c, broken, WP.STD)["first_bad"] == [36, 37]
    exe = _build(tmp_path)
    tools = {"python": lambda w, out: [sys.executable, os.path.join(ROOT, "tools", "prove_files.py"), "-z", zpath, "-w", w,
                                       "--check-witness", rpath, "-y", "-o", out, "-i", out + ".public"],
             "native": lambda w, out: [exe, "-z", zpath, "-w", w, "--check-witness-r1cs", rpath, "-y", "-o", out, "-i",
                                       out + ".public"]}
    for name, cmd in tools.items():
        out = str(tmp_path / f"{name}_good.json")
        r = subprocess.run(cmd(good, out), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (name, r.stdout[-2000:], r.stderr[-2000:])
        assert "witness check: ok" in r.stdout and "verification succeeded" in r.stdout
        assert json.load(open(out))["protocol"] == "groth16"
        out = str(tmp_path / f"{name}_bad.json")
        r = subprocess.run(cmd(bad, out), capture_output=True, text=True, timeout=600)
        assert r.returncode == 2, (name, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        assert "witness check: FAILED" in r.stdout and "constraint 36:" in r.stdout and "37" in r.stdout
        assert not os.path.exists(out) and not os.path.exists(out + ".public")
