"""Every NTT pass plan (ntt_plan.hpp) of the three workgroup geometries held to every output of the C oracle.

The pass planner splits a 2^log2n transform into passes by the geometry G16_NTT_TILE selects; each (geometry, log2n)
launches its own sequence of pass shapes.  Here every log2n 0..24 runs in both directions in every geometry, plus 2^25
(the first four-pass plan of the 1024 geometry) and 2^26 (the first rho-9 middle pass of the 2048 and 4096 geometries):
together they launch every pass shape the planner produces up to 2^28 (test_plans_reach_every_pass_shape).  The
quotient (both flavours, the fused last pass), the device entry points (in place, scattered quotient inputs) and the
twiddle / coset caches switching sizes are held to the oracle the same way.

G16_NTT_TILE is read once per process, so the 1024 and 4096 geometries run in child processes.  The single-threaded
oracle computes each output once: this module caches its SHA-256 digests, and the children compare against those.

Inputs are canonical Montgomery residues over the whole range of the top limb, with the Montgomery forms of 0, 1 and
r - 1 at indices 0, 1, n/2 and n - 1."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import bn254_ref as o
from tests.test_device_headers_cpu import ntt_plan_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = o.R


# ---- inputs ------------------------------------------------------------------------------------------------------
def _mont(x):
    return x * (1 << 256) % R


def _limbs(x):
    return [(x >> (64 * j)) & ((1 << 64) - 1) for j in range(4)]


EDGES = (_mont(0), _mont(1), _mont(R - 1), _mont(R - 1))        # at indices 0, 1, n/2, n - 1


def fr_vector(log2n, seed) -> bytes:
    """2^log2n canonical Montgomery residues: three uniform low limbs, the top limb uniform below r's top limb"""
    n = 1 << log2n
    rng = np.random.default_rng([seed, log2n])
    raw = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    raw[:, 3] = rng.integers(0, R >> 192, size=n, dtype=np.uint64)
    for i, v in zip((0, 1, n // 2, n - 1), EDGES):
        raw[i % n] = _limbs(v)
    return raw.astype("<u8").tobytes()


def ntt_input(log2n):
    return fr_vector(log2n, 1)


def quotient_inputs(log2n):
    return tuple(fr_vector(log2n, s) for s in (2, 3, 4))


# ---- the oracle, once per output -----------------------------------------------------------------------------------
# key: ("ntt", log2n, inverse) or ("quotient", log2n, flavour)   (flavour 1 = snarkjs, 0 = JensGroth)
_DIGESTS = {}


def _sha(b):
    return hashlib.sha256(b).hexdigest()


def oracle_output(orc, key) -> bytes:
    op, log2n, arg = key
    if op == "ntt":
        return orc.ntt(ntt_input(log2n), log2n, inverse=bool(arg))
    a, b, c = quotient_inputs(log2n)
    return (orc.quotient_snarkjs if arg == 1 else orc.quotient_jensgroth)(a, b, c, log2n)


def oracle_digest(orc, key) -> str:
    if key not in _DIGESTS:
        _DIGESTS[key] = _sha(oracle_output(orc, key))
    return _DIGESTS[key]


def first_difference(got: bytes, want: bytes):
    """None if equal, else a description naming the first differing element"""
    if got == want:
        return None
    if len(got) != len(want):
        return f"{len(got)} bytes, expected {len(want)}"
    a = np.frombuffer(got, dtype=np.uint8).reshape(-1, 32)
    b = np.frombuffer(want, dtype=np.uint8).reshape(-1, 32)
    bad = np.nonzero((a != b).any(axis=1))[0]
    i = int(bad[0])
    return (f"{len(bad)} of {len(a)} elements differ, the first at index {i}: "
            f"got {bytes(a[i])[::-1].hex()} expected {bytes(b[i])[::-1].hex()}")


def _label(key, entry="", tile=2048):
    op, log2n, arg = key
    what = ("inverse" if arg else "forward") if op == "ntt" else ("snarkjs" if arg == 1 else "jensgroth")
    return f"G16_NTT_TILE={tile} {op}{entry} log2n={log2n} {what}"


def check(orc, key, got, entry=""):
    """got == the oracle's output for `key`, byte for byte (through its digest once the oracle has run)"""
    want = None
    if key not in _DIGESTS:
        want = oracle_output(orc, key)
        _DIGESTS[key] = _sha(want)
        if got == want:
            return
    elif _sha(got) == _DIGESTS[key]:
        return
    pytest.fail(f"{_label(key, entry)}: {first_difference(got, want or oracle_output(orc, key))}")


# ---- the product's entry points ------------------------------------------------------------------------------------
def run_case(ctx, entry, key) -> bytes:
    """one output of the product.  entry: "" (host memory), "_dev" (torch device buffers, out of place), "_dev_inplace"
    (NTT, d_dst == d_src), "_dev_split" (quotient, Az / Bz / Cz apart and out of order)"""
    op, log2n, arg = key
    n = 1 << log2n
    if not entry:
        if op == "ntt":
            return ctx.ntt(ntt_input(log2n), log2n, bool(arg))
        return ctx.quotient(*quotient_inputs(log2n), log2n, arg)
    import torch

    def dev(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    if op == "ntt":
        xb = ntt_input(log2n)
        src = dev(xb)
        dst = src if entry == "_dev_inplace" else torch.empty_like(src)
        torch.cuda.synchronize()
        ctx.ntt(src.data_ptr(), log2n, bool(arg), dst=dst.data_ptr(), device=True)
        ctx.synchronize()
        if entry != "_dev_inplace":
            assert src.cpu().numpy().tobytes() == xb, f"{_label(key, entry)}: the input was modified"
        return dst.cpu().numpy().tobytes()
    abc = quotient_inputs(log2n)
    if entry == "_dev_split":       # [Bz][gap][Az][gap][Cz]: d_Bz != d_Az + n, so the inputs are staged
        buf = dev(abc[1] + bytes(32) + abc[0] + bytes(32) + abc[2])
        m = 32 * n
        ptrs = [buf.data_ptr() + m + 32, buf.data_ptr(), buf.data_ptr() + 2 * m + 64]
    else:                           # Az | Bz | Cz contiguous, read where they lie
        buf = dev(b"".join(abc))
        ptrs = [buf.data_ptr() + 32 * n * v for v in range(3)]
    before = buf.cpu().numpy().tobytes()
    out = torch.empty(32 * n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.quotient(*ptrs, log2n, arg, out=out.data_ptr(), device=True)
    ctx.synchronize()
    assert buf.cpu().numpy().tobytes() == before, f"{_label(key, entry)}: the inputs were modified"
    return out.cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def pctx():
    """a context of this module's own: it drops the 2^26 staging buffers when the module is done"""
    from nim_groth16_amd import Context
    c = Context(0)
    c.selftest()
    yield c
    c.close()


# ---- which plans run ----------------------------------------------------------------------------------------------
NTT_SIZES = [(log2n, inv) for log2n in range(25) for inv in (0, 1)]
BIG = {2048: [(25, 0), (25, 1), (26, 0)], 1024: [(25, 0)], 4096: [(25, 0), (26, 0)]}
QUOTIENTS = {2048: [(18, 1), (19, 1), (21, 1), (23, 1), (24, 1), (21, 0), (23, 0)],
             1024: [(17, 1), (17, 0), (23, 1), (23, 0)], 4096: [(21, 1), (21, 0), (23, 1), (23, 0)]}
# device entry points: one-pass size, multi-pass sizes
DEV_SIZES = {2048: (10, 11, 21), 1024: (8, 11, 21), 4096: (10, 11, 21)}


def _dev_cases(tile):
    one, *multi = DEV_SIZES[tile]
    cases = []
    for log2n in (one, *multi):
        for inv in (0, 1):
            cases += [("_dev", ("ntt", log2n, inv)), ("_dev_inplace", ("ntt", log2n, inv))]
    for log2n in (one, multi[-1]):
        for flavour in (1, 0):
            cases += [("_dev", ("quotient", log2n, flavour)), ("_dev_split", ("quotient", log2n, flavour))]
    return cases


def _shapes(tile, log2n):
    plan = ntt_plan_rule(tile, log2n)
    pos = lambda p: "only" if len(plan) == 1 else "first" if p == 0 else "last" if p == len(plan) - 1 else "middle"  # noqa: E731
    return {(pos(p), rho, log2b) for p, (rho, log2b, *_) in enumerate(plan)}


def test_plans_reach_every_pass_shape():
    """the sizes this module runs launch every (position, rho, log2b) pass shape that log2n 1..28 can produce, in
    every geometry, and every pass count (the 1024 geometry's four-pass plans among them)"""
    for tile in (1024, 2048, 4096):
        run = {log2n for log2n, _ in NTT_SIZES + BIG[tile]}
        want = set().union(*(_shapes(tile, k) for k in range(1, 29)))
        have = set().union(*(_shapes(tile, k) for k in run))
        assert want <= have, (tile, sorted(want - have))
        assert {len(ntt_plan_rule(tile, k)) for k in range(29)} == {len(ntt_plan_rule(tile, k)) for k in run}, tile


def test_comparison_harness_names_the_first_difference(tmp_path):
    """the checks themselves (CPU): one corrupted byte is reported at its element, a corrupted digest makes a child
    name its case and leave the output behind"""
    want = fr_vector(6, 9)
    bad = bytearray(want)
    bad[32 * 37 + 5] ^= 1
    msg = first_difference(bytes(bad), want)
    assert msg.startswith("1 of 64 elements differ, the first at index 37:"), msg
    assert first_difference(want, want) is None
    assert first_difference(want[:-32], want) == f"{len(want) - 32} bytes, expected {len(want)}"
    key, digest = ("ntt", 6, 1), _sha(want)
    r = _child_check(key, "", want, ("1" if digest[0] == "0" else "0") + digest[1:], str(tmp_path))
    assert r == "MISMATCH " + _label(key, "", 2048), r
    with open(os.path.join(tmp_path, "mismatch.bin"), "rb") as f:
        assert f.read() == want
    with open(os.path.join(tmp_path, "mismatch.json")) as f:
        assert json.load(f) == {"entry": "", "key": list(key)}
    assert _child_check(key, "", want, digest, str(tmp_path)) is None
    # the parent's report of such a child names the first differing element
    assert "the first at index 37" in _report_mismatch(lambda k: want, 1024, bytes(bad), "", key)


def _child_check(key, entry, got, digest, dump_dir, tile=2048):
    """child side: None, or writes the output and the case to dump_dir and returns the MISMATCH line"""
    if _sha(got) == digest:
        return None
    with open(os.path.join(dump_dir, "mismatch.bin"), "wb") as f:
        f.write(got)
    with open(os.path.join(dump_dir, "mismatch.json"), "w") as f:
        json.dump({"entry": entry, "key": list(key)}, f)
    return "MISMATCH " + _label(key, entry, tile)


def _report_mismatch(oracle, tile, got, entry, key):
    return f"{_label(key, entry, tile)}: {first_difference(got, oracle(key))}"


# ---- default geometry, in process ---------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("log2n", range(25))
def test_ntt_default_geometry_every_size(pctx, orc, log2n):
    for inv in (0, 1):
        key = ("ntt", log2n, inv)
        check(orc, key, run_case(pctx, "", key))


@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize("log2n,inv", BIG[2048], ids=lambda v: str(v))
def test_ntt_default_geometry_large(pctx, orc, log2n, inv):
    key = ("ntt", log2n, inv)
    check(orc, key, run_case(pctx, "", key))


@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize("log2n,flavour", QUOTIENTS[2048], ids=lambda v: str(v))
def test_quotient_default_geometry(pctx, orc, log2n, flavour):
    key = ("quotient", log2n, flavour)
    check(orc, key, run_case(pctx, "", key))


@pytest.mark.gpu
@pytest.mark.parametrize("entry,key", _dev_cases(2048), ids=lambda v: v if isinstance(v, str) else "-".join(map(str, v)))
def test_device_entry_points(pctx, orc, entry, key):
    """g16_ntt_fr_dev out of place and in place, g16_quotient_dev on contiguous and on scattered inputs"""
    check(orc, key, run_case(pctx, entry, key), entry)


@pytest.mark.gpu
def test_cached_tables_follow_the_size(orc):
    """the twiddle table and the two coset tables are cached by log2n (ntt.hip): one fresh context switching sizes"""
    from nim_groth16_amd import Context
    c = Context(0)
    try:
        for key in (("ntt", 21, 0), ("quotient", 12, 1), ("quotient", 12, 0), ("ntt", 5, 0), ("ntt", 21, 1),
                    ("quotient", 21, 0), ("quotient", 21, 1), ("ntt", 12, 1)):
            check(orc, key, run_case(c, "", key))
    finally:
        c.close()


# ---- the other two geometries, one child process each ------------------------------------------------------------
_CHILD = r"""
import json, sys
sys.path.insert(0, {root!r})
from nim_groth16_amd import Context
from tests.test_gpu_ntt_plans import _child_check, run_case
job = json.load(open(sys.argv[1]))
ctx = Context(0)
ctx.selftest()
for entry, key, digest in job["cases"]:
    key = tuple(key)
    bad = _child_check(key, entry, run_case(ctx, entry, key), digest, job["dump"], job["tile"])
    if bad:
        print(bad, flush=True)
        sys.exit(1)
ctx.close()
print("plans ok", len(job["cases"]))
"""


@pytest.mark.gpu
@pytest.mark.timeout(1200)
@pytest.mark.parametrize("tile", [1024, 4096])
def test_other_geometries_every_plan(orc, tmp_path, tile):
    cases = [("", ("ntt", log2n, inv)) for log2n, inv in NTT_SIZES + BIG[tile]]
    cases += [("", ("quotient", log2n, fl)) for log2n, fl in QUOTIENTS[tile]] + _dev_cases(tile)
    job = {"tile": tile, "dump": str(tmp_path), "cases": [(e, k, oracle_digest(orc, k)) for e, k in cases]}
    path = os.path.join(tmp_path, "job.json")
    with open(path, "w") as f:
        json.dump(job, f)
    env = {k: v for k, v in os.environ.items() if not k.startswith("G16_")}
    env["G16_NTT_TILE"] = str(tile)
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT), path], env=env, capture_output=True, text=True,
                       timeout=1000)
    if r.returncode and os.path.exists(os.path.join(tmp_path, "mismatch.json")):
        with open(os.path.join(tmp_path, "mismatch.json")) as f:
            m = json.load(f)
        with open(os.path.join(tmp_path, "mismatch.bin"), "rb") as f:
            got = f.read()
        pytest.fail(_report_mismatch(lambda k: oracle_output(orc, k), tile, got, m["entry"], tuple(m["key"])))
    assert r.returncode == 0 and f"plans ok {len(cases)}" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
