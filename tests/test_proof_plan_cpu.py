"""proof_plan.hpp on the CPU: the launch schedule of a proof -- every kernel launch, copy, event record and wait of
g16_prove_partials, g16_prove_partials_begin and g16_prove_partials_end, stream by stream -- held to a restatement of
the launch code and to the ordering that a proof's correctness rests on, for every knob set that
tests/test_gpu_knobs.py runs on the GPU.

The restatement below was written from nim_groth16_amd/csrc/prover.hip as it stood at commit bfef9c6 ("Hold the
proof's last step to integers: record sums and mask algebra"), the last one in which that file decided the schedule
while it launched: launch_witness_sorts, launch_witness_msms, launch_h_sort, launch_h_and_collect, prove_partials_impl
and the two entry points of the task-parallel quotient."""
import ctypes
import os
import subprocess

from tests.test_device_headers_cpu import HERE, shim  # noqa: F401  (the fixture that builds and loads the CPU shim)
from tests.test_gpu_knobs import KNOBS

# proof_plan.hpp
MAIN = 5
EV_NONE, EV_A, EV_B, EV_Q, EV_B2, EV_C, EV_G2, EV_DONE0 = -1, 0, 1, 2, 3, 4, 5, 6
RUN_A1, RUN_B1, RUN_C1, RUN_B2, RUN_H = range(5)
SORT_W, SORT_H, SORT_WA, SORT_WB = range(4)
(UPLOAD, WAIT, RECORD, SORT_WIT, SORT_HS, BUILD_ABC, QUOTIENT, COSET, POINTWISE, MSM, COPY_OUT,
 HOST_SYNC) = range(12)
WHOLE, BEGIN, END = range(3)
CAP = 48
WORKSPACE = {RUN_A1: 0, RUN_B1: 2, RUN_C1: 3, RUN_B2: 1, RUN_H: 4}   # the lane whose accumulate buffer a run owns
G2_FIRST_MAX = 1 << 18


def parse_knobs(env):
    """G16_* variables -> the knob values as the library reads them at start-up (ranges, defaults and spellings
    restated); the variables that neither the schedule nor the helpers next to it look at are ignored"""
    def flag(name, default):
        return int(env[name][0] != "0") if name in env else default
    cu = int(env.get("G16_CU_SPLIT", 0))
    k = dict(quotient_first=flag("G16_QUOTIENT_FIRST", 1), lanes_after_quotient=flag("G16_LANES_AFTER_QUOTIENT", 0),
             g1_batch=flag("G16_G1_BATCH", 0), chain_ch=flag("G16_CHAIN_CH", 1), cu_split=cu if 1 <= cu <= 24 else 0,
             cz_on_the_fly=flag("G16_CZ_FLY", 1), g2_first=-1, g1_lanes=(3, 2, 0))
    if "G16_G2_FIRST" in env:
        k["g2_first"] = 2 if env["G16_G2_FIRST"][0] == "2" else int(env["G16_G2_FIRST"][0] != "0")
    v = env.get("G16_G1_LANES", "")
    if len(v) == 3 and set(v) <= set("023"):
        k["g1_lanes"] = tuple(int(c) for c in v)
    return k


def knob_vector(k):
    return [k["quotient_first"], k["lanes_after_quotient"], k["g1_batch"], k["chain_ch"], k["cu_split"],
            k["cz_on_the_fly"], k["g2_first"], *k["g1_lanes"]]


# ---- the restatement ----------------------------------------------------------------------------------------------------
def chain_c_into_h(k, s):
    return bool(k["chain_ch"] and s["nw"] and s["nh"] and s["cfg_equal"])


def witness_sorts(out, k, s):
    if not s["nw"]:
        return
    out.append((WAIT, 0, EV_A))
    out.append((SORT_WIT, 0, SORT_W, 0, RUN_A1))
    if s["liveA"]:
        out.append((SORT_WIT, 0, SORT_WA, 1, RUN_A1))
    out.append((RECORD, 0, EV_B))
    if s["liveB"]:
        out.append((WAIT, 1, EV_A))
        out.append((SORT_WIT, 1, SORT_WB, 2, RUN_B2))
        out.append((RECORD, 1, EV_B2))


def witness_msms(out, k, s, after):
    if not s["nw"]:
        return
    batch = k["g1_batch"] != 0
    chain = chain_c_into_h(k, s)
    la, lb, lc = (0, 0, 0) if batch else k["g1_lanes"]
    nlanes = 2 if batch else 4
    for i in range(1, nlanes):
        out.append((WAIT, i, EV_B2 if i == 1 and s["liveB"] else EV_B))
    if s["liveB"]:
        out.append((WAIT, lb, EV_B2))
    if s["liveA"] and la != 0:
        out.append((WAIT, la, EV_B))
    if after != EV_NONE:
        for i in range(nlanes):
            out.append((WAIT, i, after))
    g2_first = k["g2_first"] != 0 if k["g2_first"] >= 0 else s["nw"] <= G2_FIRST_MAX
    out.append((MSM, 1, RUN_B2, 1, 1, EV_G2 if g2_first else EV_NONE, 0))
    if g2_first:
        out.append((WAIT, la, EV_G2))
        out.append((WAIT, lb, EV_G2))
        if not chain or k["g2_first"] == 2:
            out.append((WAIT, lc, EV_G2))
    ev_c = EV_C if chain else EV_NONE
    if batch:
        out.append((MSM, 0, RUN_A1, 3, 2 if chain else 3, ev_c, 0))
    else:
        out.append((MSM, la, RUN_A1, 1, 1, EV_NONE, 0))
        out.append((MSM, lb, RUN_B1, 1, 1, EV_NONE, 0))
        out.append((MSM, lc, RUN_C1, 1, 0 if chain else 1, ev_c, 0))
    for i in range(nlanes):
        out.append((RECORD, i, EV_DONE0 + i))


def h_and_collect(out, k, s, is_sorted, host_sync):
    if s["nh"]:
        if not is_sorted:
            out.append((SORT_HS, MAIN))
        chain = chain_c_into_h(k, s)
        hs = 4 if k["cu_split"] else MAIN
        if hs != MAIN:
            out.append((RECORD, MAIN, EV_Q))
            out.append((WAIT, hs, EV_Q))
        if chain:
            out.append((WAIT, hs, EV_C))
        out.append((MSM, hs, RUN_H, 1, 1, EV_NONE, int(chain)))
        if hs != MAIN:
            out.append((RECORD, hs, EV_DONE0 + 4))
            out.append((WAIT, MAIN, EV_DONE0 + 4))
    if s["nw"]:
        for i in range(2 if k["g1_batch"] else 4):
            out.append((WAIT, MAIN, EV_DONE0 + i))
    out.append((COPY_OUT, MAIN))
    if host_sync:
        out.append((HOST_SYNC, MAIN))


def parent_schedule(k, entry, task_mask, host_sync, s):
    """what the launch code issued, call by call, in issue order"""
    out = []
    if entry == END:
        out.append((POINTWISE, MAIN))
        h_and_collect(out, k, s, False, host_sync)
        return out
    out.append((UPLOAD, MAIN))
    out.append((RECORD, MAIN, EV_A))
    if entry == BEGIN:
        if task_mask:
            out.append((BUILD_ABC, MAIN, int(task_mask & 4 != 0)))
            for v in range(3):
                if task_mask & (1 << v):
                    out.append((COSET, MAIN, v))
        after = EV_NONE
        if task_mask and k["quotient_first"] and k["lanes_after_quotient"]:
            out.append((RECORD, MAIN, EV_Q))
            after = EV_Q
        witness_sorts(out, k, s)
        witness_msms(out, k, s, after)
        if host_sync:
            out.append((HOST_SYNC, MAIN))
        return out
    fly = int(s["log2n"] >= 1 and k["cz_on_the_fly"] != 0)
    if not k["quotient_first"]:
        witness_sorts(out, k, s)
        witness_msms(out, k, s, EV_NONE)
        out.append((BUILD_ABC, MAIN, int(fly == 0)))
        out.append((QUOTIENT, MAIN, fly))
        h_and_collect(out, k, s, False, host_sync)
        return out
    out.append((BUILD_ABC, MAIN, int(fly == 0)))
    out.append((QUOTIENT, MAIN, fly))
    if s["nh"]:
        out.append((SORT_HS, MAIN))
    after = EV_NONE
    if k["lanes_after_quotient"]:
        out.append((RECORD, MAIN, EV_Q))
        after = EV_Q
    witness_sorts(out, k, s)
    witness_msms(out, k, s, after)
    h_and_collect(out, k, s, True, host_sync)
    return out


def pad(step):
    return tuple(step) + (0,) * (7 - len(step))


def records(step, ev):
    return (step[0] == RECORD and step[2] == ev) or (step[0] == MSM and step[5] == ev)


def drop_repeated_waits(steps):
    """the one licence the plan has: a wait that repeats an earlier wait of the same stream for the same event, with
    no new record of the event in between, is a no-op.  -> (steps without them, the waits dropped)"""
    kept, dropped = [], []
    for st in map(pad, steps):
        if st[0] == WAIT:
            repeated = False
            for prev in reversed(kept):
                if records(prev, st[2]):
                    break
                if prev[0] == WAIT and prev[1] == st[1] and prev[2] == st[2]:
                    repeated = True
                    break
            if repeated:
                dropped.append(st)
                continue
        kept.append(st)
    return kept, dropped


# ---- the C++ plan -------------------------------------------------------------------------------------------------------
class Plan:
    def __init__(self, ok, count, narrow_tail, sort_a, sort_b, steps):
        self.ok, self.count, self.narrow_tail, self.sort_a, self.sort_b, self.steps = (ok, count, narrow_tail, sort_a,
                                                                                       sort_b, steps)


def run_plan(shim, k, entry, task_mask, host_sync, s, cap=CAP):  # noqa: F811
    knobs = (ctypes.c_int * 10)(*knob_vector(k))
    shape = (ctypes.c_uint64 * 6)(s["nw"], s["nh"], s["log2n"], s["liveA"], s["liveB"], s["cfg_equal"])
    out = (ctypes.c_int32 * (5 + 7 * CAP))()
    shim.shim_proof_plan.restype = ctypes.c_int
    shim.shim_proof_plan.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_uint32, ctypes.c_int,
                                     ctypes.POINTER(ctypes.c_uint64), ctypes.c_int, ctypes.POINTER(ctypes.c_int32)]
    n = shim.shim_proof_plan(knobs, entry, task_mask, int(host_sync), shape, cap, out)
    v = list(out)
    assert n == v[1] and 0 <= n <= CAP
    return Plan(v[0], n, v[2], v[3], v[4], [tuple(v[5 + 7 * i: 12 + 7 * i]) for i in range(n)])


# ---- the grid -----------------------------------------------------------------------------------------------------------
def knob_sets():
    """every knob set of the GPU suite, none, and the lane assignments and G2 orders; sets that the library parses to
    the same schedule knobs are one input of the plan and are built once"""
    envs = [{}] + KNOBS + [{"G16_G1_LANES": v} for v in ("320", "023", "000", "302")] + \
        [{"G16_G2_FIRST": v} for v in ("0", "1", "2")]
    seen = {}
    for env in envs:
        k = parse_knobs(env)
        seen.setdefault(tuple(knob_vector(k)), k)
    return list(seen.values())


def shapes():
    for nw in (0, 1, 2046, 1 << 18, (1 << 18) + 1, 1 << 20):
        for nh in (0, 1, 1 << 11):
            for live in range(4):
                for cfg_equal in (0, 1):
                    for log2n in (0, 11):
                        yield dict(nw=nw, nh=nh, log2n=log2n, liveA=live & 1, liveB=live >> 1, cfg_equal=cfg_equal)


ENTRIES = ((WHOLE, 0), (BEGIN, 0), (BEGIN, 5), (BEGIN, 7), (END, 0))


def test_knob_grid_holds_the_gpu_suite_s_schedules():
    assert len(KNOBS) == 34
    ks = knob_sets()
    for key in ("quotient_first", "lanes_after_quotient", "g1_batch", "chain_ch", "cz_on_the_fly"):
        assert {k[key] for k in ks} == {0, 1}, key
    assert {k["g2_first"] for k in ks} == {-1, 0, 1, 2} and {k["cu_split"] for k in ks} == {0, 4, 8}
    assert {k["g1_lanes"] for k in ks} == {(3, 2, 0), (0, 2, 3), (0, 0, 0), (3, 0, 2)}


def test_plan_equals_the_restated_schedule_on_the_whole_grid(shim):  # noqa: F811
    dropped_kinds = set()
    longest = 0
    for k in knob_sets():
        for s in shapes():
            for entry, task_mask in ENTRIES:
                for host_sync in ((0, 1) if k == parse_knobs({}) else (1,)):
                    p = run_plan(shim, k, entry, task_mask, host_sync, s)
                    want, dropped = drop_repeated_waits(parent_schedule(k, entry, task_mask, host_sync, s))
                    where = (k, s, entry, task_mask, host_sync)
                    assert p.ok == 1 and p.steps == want, (where, p.steps, want)
                    assert p.narrow_tail == 1, where
                    assert (p.sort_a, p.sort_b) == (SORT_WA if s["liveA"] else SORT_W,
                                                    SORT_WB if s["liveB"] else SORT_W), where
                    dropped_kinds |= {(st[2], k["g1_batch"], len(set(k["g1_lanes"])) < 3) for st in dropped}
                    longest = max(longest, p.count)
    # the waits the plan leaves out: A1's lane waiting a second time for the witness sort (the key has entry lists of
    # its own for A1), and lanes that carry two or three of the G1 MSMs waiting once each for B2's accumulation
    assert {ev for ev, _, _ in dropped_kinds} == {EV_B, EV_G2}
    assert all(batch or shared for ev, batch, shared in dropped_kinds if ev == EV_G2)
    assert longest <= CAP
    print("longest plan:", longest, "steps")


def test_a_plan_that_does_not_fit_fails_and_stays_inside(shim):  # noqa: F811
    k, s = parse_knobs({}), dict(nw=2046, nh=2048, log2n=11, liveA=1, liveB=1, cfg_equal=1)
    full = run_plan(shim, k, WHOLE, 0, 1, s)
    for cap in (0, 1, full.count - 1):
        p = run_plan(shim, k, WHOLE, 0, 1, s, cap=cap)
        assert p.ok == 0 and p.count == cap and p.steps == full.steps[:cap]
    assert run_plan(shim, k, WHOLE, 0, 1, s, cap=full.count).ok == 1
    assert run_plan(shim, k, WHOLE, 0, 1, s, cap=10 * CAP).ok == 1      # never more than the array holds


# ---- ordering -----------------------------------------------------------------------------------------------------------
def expand(steps):
    """an MSM with an `after_heavy` event records it between its accumulation and its tail: three nodes.
    -> nodes (kind, stream, step) with kind in 'acc', 'tail', 'msm' (both), or the op"""
    nodes = []
    for st in steps:
        if st[0] == MSM and st[5] != EV_NONE:
            nodes += [("acc", st[1], st), (RECORD, st[1], (RECORD, st[1], st[5], 0, 0, 0, 0)), ("tail", st[1], st)]
        else:
            nodes.append(("msm" if st[0] == MSM else st[0], st[1], st))
    return nodes


def ancestors(nodes):
    """happens-before as bit sets: stream order, a wait behind the latest earlier record of its event, and everything
    issued after a host wait behind what the main stream held then.  -> (sets, waits without a record)"""
    anc, last_on, last_record, unbound, synced = [], {}, {}, [], None
    for i, (kind, stream, st) in enumerate(nodes):
        preds = [p for p in (last_on.get(stream), synced) if p is not None]
        if kind == WAIT:
            if st[2] in last_record:
                preds.append(last_record[st[2]])
            else:
                unbound.append(st)
        a = 0
        for p in preds:
            a |= anc[p] | (1 << p)
        anc.append(a)
        last_on[stream] = i
        if kind == RECORD:
            last_record[st[2]] = i
        if kind == HOST_SYNC:
            synced = i
    return anc, unbound


def ordering_faults(steps, sort_a, sort_b):
    nodes = expand(steps)
    anc, unbound = ancestors(nodes)
    before = lambda i, j: bool(anc[j] >> i & 1)                                       # noqa: E731
    faults = [("wait without a record", st) for st in unbound]                                         # 1
    index = lambda pred: [i for i, n in enumerate(nodes) if pred(n)]                   # noqa: E731
    uploads = index(lambda n: n[0] == UPLOAD)
    slot_of = {RUN_A1: sort_a, RUN_B1: sort_b, RUN_B2: sort_b, RUN_C1: SORT_W, RUN_H: SORT_H}
    sort_nodes = {}
    for i in index(lambda n: n[0] in (SORT_WIT, SORT_HS)):
        sort_nodes.setdefault(SORT_H if nodes[i][0] == SORT_HS else nodes[i][2][2], []).append(i)
    use = {}                                                  # resource -> nodes that write it or read what another wrote
    for slot, ii in sort_nodes.items():
        use[("sort", slot)] = list(ii)
    for i, (kind, stream, st) in enumerate(nodes):
        if kind in ("acc", "msm"):
            for run in range(st[2], st[2] + st[3]):
                writers = sort_nodes.get(slot_of[run], [])
                if not writers or not all(before(w, i) for w in writers):                                # 2
                    faults.append(("MSM not behind its sort", st, run))
                use.setdefault(("acc", WORKSPACE[run]), []).append(i)
            if st[6]:                                                                                    # 5
                rec = [j for j in index(lambda n: n[0] == RECORD and n[2][2] == EV_C) if j < i]
                c1 = [j for j in rec if nodes[j - 1][0] == "acc" and
                      nodes[j - 1][2][2] <= RUN_C1 < nodes[j - 1][2][2] + nodes[j - 1][2][3]]
                if not rec or rec[-1:] != c1[-1:] or not before(rec[-1], i):
                    faults.append(("H not behind C1's bucket sums", st))
                use.setdefault(("acc", WORKSPACE[RUN_C1]), []).append(i)
        if kind in (SORT_WIT, SORT_HS, BUILD_ABC) and not (uploads and before(uploads[-1], i)):                  # 3
            faults.append(("reads the witness before it is there", st))
    record_writers = index(lambda n: n[0] in ("tail", "msm") and n[2][4] > 0)
    for i in record_writers:
        if not (uploads and before(uploads[-1], i)):                                                     # 4
            faults.append(("writes the record before it is cleared", nodes[i][2]))
    for res, ii in use.items():                                                                          # 6
        for x in range(len(ii)):
            for y in range(x + 1, len(ii)):
                if not (before(ii[x], ii[y]) or before(ii[y], ii[x])):
                    faults.append(("unordered on " + str(res), nodes[ii[x]][2], nodes[ii[y]][2]))
    for c in index(lambda n: n[0] == COPY_OUT):                                                          # 7
        faults += [("copy-out not behind a writer", nodes[i][2]) for i in record_writers if not before(i, c)]
    return faults


def test_ordering_walk_finds_what_it_looks_for():
    """the walk on schedules with one edge taken out"""
    k, s = parse_knobs({}), dict(nw=2046, nh=2048, log2n=11, liveA=1, liveB=1, cfg_equal=1)
    good, _ = drop_repeated_waits(parent_schedule(k, WHOLE, 0, 1, s))
    assert ordering_faults(good, SORT_WA, SORT_WB) == []
    kinds = set()
    for i, st in enumerate(good):
        if st[0] in (WAIT, RECORD):
            kinds |= {f[0].split(" on ")[0] for f in ordering_faults(good[:i] + good[i + 1:], SORT_WA, SORT_WB)}
    assert kinds >= {"wait without a record", "MSM not behind its sort", "reads the witness before it is there",
                     "writes the record before it is cleared", "H not behind C1's bucket sums", "unordered",
                     "copy-out not behind a writer"}, kinds
    assert ordering_faults(good, SORT_W, SORT_WB) == []        # (the shared arrangement is there as well)
    assert ordering_faults([st for st in good if st[:3] != (SORT_WIT, 0, SORT_WA)], SORT_WA, SORT_WB) != []


def test_every_reader_is_behind_its_writer_on_the_whole_grid(shim):  # noqa: F811
    for k in knob_sets():
        for s in shapes():
            whole = run_plan(shim, k, WHOLE, 0, 1, s)
            assert ordering_faults(whole.steps, whole.sort_a, whole.sort_b) == [], (k, s)
            end = run_plan(shim, k, END, 0, 1, s)
            for task_mask in (0, 5, 7):
                begin = run_plan(shim, k, BEGIN, task_mask, 0, s)      # without the host wait: the weaker order
                assert ordering_faults(begin.steps + end.steps, begin.sort_a, begin.sort_b) == [], (k, s, task_mask)


# ---- the helpers next to the plan -----------------------------------------------------------------------------------------
def test_one_sparsity_predicate(shim):  # noqa: F811
    shim.shim_points_sparse.restype = ctypes.c_int
    shim.shim_points_sparse.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int]
    for pct in (0, 10, 101):
        for n in (1, 10, 1000, 2046, 1 << 20):
            at = pct * n // 100
            for n_inf in {0, max(at - 1, 0), at, at + 1, n}:
                want = n_inf != 0 and n_inf * 100 >= pct * n             # g16_points_live_if_sparse
                assert want == (not (n_inf == 0 or n_inf * 100 < pct * n))   # the key's B1 | B2 decision, negated
                assert shim.shim_points_sparse(n_inf, n, pct) == int(want), (pct, n, n_inf)
    assert shim.shim_points_sparse(0, 0, 0) == 0 and shim.shim_points_sparse(1000, 1000, 101) == 0


def test_cu_masks_partition_the_device(shim):  # noqa: F811
    shim.shim_cu_mask.restype = None
    shim.shim_cu_mask.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_uint32)]
    for k in (1, 8, 24):
        masks = []
        for front in (1, 0):
            m = (ctypes.c_uint32 * 8)()
            shim.shim_cu_mask(k, front, m)
            masks.append(sum(w << (32 * i) for i, w in enumerate(m)))
        front, back = masks
        assert front & back == 0 and front | back == (1 << 256) - 1
        assert bin(front).count("1") == 8 * k
        assert front == (1 << (8 * k)) - 1                      # CUs 0 .. k - 1 of each of the 8 XCDs


def test_stream_priorities(shim):  # noqa: F811
    shim.shim_stream_priority.restype = ctypes.c_int
    shim.shim_stream_priority.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lo, hi = 0, -2
    for cfg in (b"lhllln", b"nnnnnn", b"hhhlll"):
        for i in range(6):
            want = {"h": hi, "l": lo, "n": (lo + hi) // 2}[chr(cfg[i])]
            assert shim.shim_stream_priority(cfg, i, lo, hi) == want


# ---- bounds of the fixed-size step array ------------------------------------------------------------------------------
def test_every_plan_of_the_grid_under_sanitizers(tmp_path):
    """a stand-alone program builds every plan of the grid above, each also at capacities below its length, under
    AddressSanitizer and UndefinedBehaviorSanitizer"""
    exe = str(tmp_path / "proof_plan_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(HERE, "proof_plan_main.cpp"), "-o", exe])
    knobs = [",".join(map(str, knob_vector(k))) for k in knob_sets()]
    r = subprocess.run([exe] + knobs, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "proof plans ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
