"""The proof's launch sequence issues the kernels it always did: per-kernel launch counts of one proof of the
2^11-constraint circuit of test_gpu_knobs.py, under the schedule knobs that change them, against counts recorded from the
launch code as it stood before the schedule became a plan (tests/golden/proof_launch_counts.json; recorded at commit
bfef9c6, the parent of the change that introduced nim_groth16_amd/csrc/proof_plan.hpp).  The counts are a function of the
schedule alone; the proof itself is compared with the oracle's bit for bit.  One process per knob set: the knobs are read
once per process."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "proof_launch_counts.json")

SCRIPT = r"""
import json, sys
sys.path.insert(0, {root!r})
from tests.oracle_c import load_oracle
from tests.parity import check_gpu_proof
from nim_groth16_amd import Context, Mask, Witness, generateProofWithMask, loadProvingKey
from nim_groth16_amd import bn128 as F
from nim_groth16_amd.fake_setup import ToxicWaste, fakeCircuitSetup
from nim_groth16_amd.synthetic import SplitMix64, mixedCircuit
orc = load_oracle()
ctx = Context(0)
m = (1 << 11) - 2
r1cs, wit = mixedCircuit(m, seed=4)
rng = SplitMix64(5)
zk = fakeCircuitSetup(r1cs, ToxicWaste(*[rng.fr() for _ in range(5)]), 1, ctx)
pk = loadProvingKey(zk, ctx)
wb = F.frSeqToMontBytes(wit)
mask = Mask(rng.fr(), rng.fr())
ctx.profile(1)
pr = generateProofWithMask(0, False, zk, Witness("bn128", m + 2, wb), mask, ctx, pkey=pk)
counts = {{name: v["calls"] for name, v in ctx.profile_report().items()}}
ctx.profile(0)
check_gpu_proof(orc, zk, wit, wb, mask.r, mask.s, (pr.pi_a, pr.pi_b, pr.pi_c), ctx)
pk.destroy()
print("LAUNCHES " + json.dumps(counts, sort_keys=True))
"""

KNOB_SETS = [{}, {"G16_G1_BATCH": "1"}, {"G16_CHAIN_CH": "0"}, {"G16_QUOTIENT_FIRST": "0"}, {"G16_CU_SPLIT": "8"},
             {"G16_INF_COMPACT": "0"}]


def knob_id(knobs):
    return ",".join(f"{a[4:]}={b}" for a, b in knobs.items()) or "default"


def launch_counts(knobs):
    """one proof in a process of its own -> {kernel name: launches}; the child has compared the proof with the oracle"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("G16_")}
    env.update(knobs)
    r = subprocess.run([sys.executable, "-c", SCRIPT.format(root=ROOT)], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("LAUNCHES ")]
    assert len(line) == 1, r.stdout[-2000:]
    return json.loads(line[0][len("LAUNCHES "):])


@pytest.mark.parametrize("knobs", KNOB_SETS, ids=knob_id)
def test_a_proof_launches_what_it_did_before_the_plan(knobs):
    with open(GOLDEN) as f:
        want = json.load(f)[knob_id(knobs)]
    got = launch_counts(knobs)
    print(knob_id(knobs), json.dumps(got, sort_keys=True))
    assert got == want, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}
