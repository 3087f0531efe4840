"""Exceptional bucket pictures for the MSM tail (msm_heavy, msm_reduce1, the msm_reduce2 variants, the folds of msm.cuh).

Pure Python: no GPU, no ctypes.  A *geometry* is the launch plan a process with given knobs runs for n points (the
restated rule of tests/test_msm_plan_cpu.py) plus what follows from it: which bucket a digit magnitude lands in, and
which chunk, slot range and set (window / slice) a bucket belongs to.  A *picture* is a function of a geometry that
returns (scalars, logs, planted infinities): the points are logs[i] * G, so a scalar that is a single digit puts a
chosen multiple of ONE random point Q into exactly one bucket, and any linear relation between bucket sums, chunk sums,
set sums and set totals can be dictated through the C ABI.  The expected value of every picture is
(sum s_i k_i mod r) * G (tests.inputs.expected_from_logs) -- never anything computed here.

`walk` replays the sums of the tail on integers mod r only to show that a picture reaches the additions it was built
for (tests/test_msm_pictures_cpu.py asserts that); tests/test_gpu_msm_tail_edges.py runs the pictures on the GPU.
"""
from collections import Counter, defaultdict

from oracle import bn254_ref as o
from tests.test_msm_plan_cpu import (CLASSES, CLASSES_QUAD, MERGED, NARROW, PLAIN, QUAD64, QUAD128, WAVE, WIDE, Plan,
                                     msm_plan_rule, parse_knobs)

R = o.R
HEAVY_MIN = 12                      # msm.cuh
INF_COMPACT_PCT = 10                # g16_env.hpp: registered sets with this share of (0,0) points drop them from the sort
K = o.SplitMix64(0x7a11).fr()       # log of Q
K2 = o.SplitMix64(0x7a12).fr()      # log of an unrelated point

R2_NAME = {QUAD128: "QUAD128", QUAD64: "QUAD64", WIDE: "WIDE", NARROW: "NARROW", WAVE: "WAVE"}
FOLD_NAME = {CLASSES_QUAD: "CLASSES_QUAD", CLASSES: "CLASSES", MERGED: "MERGED", PLAIN: "PLAIN"}

# The knob sets of tests/test_gpu_msm_tail_edges.py: (knobs, picture families run there)
ALL = ("every", "slot", "alt", "single", "total", "relations", "heavy", "infpts")
LEAN = ("slot", "alt", "single", "total", "relations")          # no picture with n > 2^14, no heavy bucket
KNOB_SETS = [
    ({}, ALL),
    ({"G16_TABLE_WINDOW": "15", "G16_MSM_WINDOW": "11"}, ALL),   # one-shot: 256 chunks per window on 64 quads, G1 too
    ({"G16_TABLE_WINDOW": "15", "G16_TAIL_QUAD": "0"}, ALL),
    ({"G16_TABLE_WINDOW": "15", "G16_MSM_WINDOW": "13", "G16_R2_WIDTH": "1", "G16_RED_CHUNK": "16"}, ALL),
    ({"G16_TABLE_WINDOW": "14", "G16_MSM_WINDOW": "12", "G16_R2_WIDTH": "2"}, ALL),
    ({"G16_MSM_WINDOW": "16", "G16_TABLE_WINDOW": "20", "G16_MTAB": "1"}, LEAN),
    ({"G16_TABLE_WINDOW": "16", "G16_MSM_WINDOW": "12", "G16_MTAB": "1", "G16_TAIL_QUAD": "0", "G16_RED_CHUNK": "2"}, ALL),
    ({"G16_TABLE_WINDOW": "20"}, LEAN),
    ({"G16_R2_WIDTH": "2"}, ALL),                                 # the single-wave reduce2 with one chunk per lane
]


def knob_id(knobs):
    return ",".join(f"{a[4:]}={b}" for a, b in knobs.items()) or "default"


# ---- geometry -------------------------------------------------------------------------------------------------------
def class_bucket(t, c):
    """msm_class_bucket (msm_params.hpp) restated: digit magnitude t in [1, 2^(c-1)] -> (bucket, table selector)"""
    tz, h = (t & -t).bit_length() - 1, 1 << (c - 1)
    if tz >= 6:
        return h // 2 + h // 8 + h // 32 + (t >> 6) - 1, 0
    z, v = tz >> 1, t >> (tz + 1)
    return (0, h // 2, h // 2 + h // 8)[z] + v, tz & 1


def class_weight(b, c):
    """the inverse: bucket of the class set -> its weight, which is also the magnitude served from table 0"""
    h = 1 << (c - 1)
    for z, (base, size) in enumerate(((0, h // 2), (h // 2, h // 8), (h // 2 + h // 8, h // 32))):
        if b < base + size:
            return 4 ** z * (2 * (b - base) + 1)
    return 64 * (b - (h // 2 + h // 8 + h // 32) + 1)


class Geometry:
    def __init__(self, n, registered, is_g1, env):
        self.n, self.registered, self.is_g1, self.env = n, registered, is_g1, dict(env)
        p = self.plan = Plan(msm_plan_rule(n, registered, is_g1, False, parse_knobs(env)))
        self.c, self.nwin, self.H, self.mtab, self.seg = p.c, p.nwin, 1 << (p.c - 1), p.mtab, p.seg
        self.kind = "plain" if not registered else ("class" if p.mtab == 2 else "merged")
        self.rc, self.nsets, self.cps, self.r2, self.fold = p.rc, p.nsets, p.cps, p.r2, p.fold
        self.ks = p.cps * p.rc                                    # buckets per set
        wide = 512 if is_g1 else 256
        self.slots = {QUAD128: 128, QUAD64: 64, WIDE: wide, NARROW: wide // 4, WAVE: 64}[p.r2]
        self.per = -(-p.cps // self.slots)                        # chunks per slot / thread
        self.live_slots = -(-p.cps // self.per)
        self.heavy_block = 256 if is_g1 else 128
        self.top_max = (R - 1) >> (p.c * (p.nwin - 1))            # the largest digit of the top window

    def limit(self, v):
        """local buckets of set v that a scalar < r can reach"""
        return min(self.ks, self.top_max) if self.kind == "plain" and v == self.nwin - 1 else self.ks

    def scalar(self, v, l):
        """the scalar that is ONE digit landing in local bucket l (0-based, slice-local weight l + 1) of set v"""
        assert 0 <= v < self.nsets and 0 <= l < self.limit(v), (v, l)
        if self.kind == "plain":
            return (l + 1) << (self.c * v)
        b = v * self.ks + l
        return b + 1 if self.kind == "merged" else class_weight(b, self.c)

    def weight(self, v, l):
        """what a point in that bucket is multiplied by in the MSM"""
        return self.scalar(v, l)

    def slot_range(self, v, s):
        """first and last reachable local bucket of slot range s of set v (None if none is reachable)"""
        lo, hi = s * self.per * self.rc, min((s + 1) * self.per, self.cps) * self.rc
        hi = min(hi, self.limit(v))
        return (lo, hi - 1) if lo < hi else None

    def describe(self):
        return dict(c=self.c, mtab=self.mtab, rc=self.rc, nsets=self.nsets, cps=self.cps, r2=R2_NAME[self.r2],
                    fold=FOLD_NAME[self.fold], per=self.per)


def geometry(n, registered, is_g1, env):
    return Geometry(n, registered, is_g1, env)


# ---- pictures -------------------------------------------------------------------------------------------------------
class Picture:
    """name, family, build(geometry) -> (scalars, logs, planted infinities) or None where it does not apply,
    reach: the (cell, kind) pairs `walk` must report, std: also run with standard-form scalars"""

    def __init__(self, name, family, build, reach=(), std=False):
        self.name, self.family, self.build, self.reach, self.std = name, family, build, tuple(reach), std


def _pts(g, places):
    """places: (set, local bucket, multiple of Q) -> scalars, logs"""
    return [g.scalar(v, l) for v, l, _ in places], [m * K % R for _, _, m in places], set()


def _every_bucket_equal(g):
    if g.H > 1 << 14:
        return None
    if g.kind == "plain":                                         # scalars 1..H: window 0
        return list(range(1, g.H + 1)), [K] * g.H, set()
    return _pts(g, [(v, l, 1) for v in range(g.nsets) for l in range(g.ks)])


def _one_per_slot(last):
    def build(g):
        places = []
        for v in range(g.nsets):
            for s in range(g.live_slots):
                r = g.slot_range(v, s)
                if r:
                    places.append((v, r[1] if last else r[0], 1))
        return _pts(g, places)
    return build


def _alternating(level):
    def build(g):
        if level == "bucket":
            places = [(v, l, (-1) ** l) for v in range(min(g.nsets, 2)) for l in range(min(g.limit(v), 4 * g.rc))]
        elif level == "chunk":
            if g.cps < 2:
                return None
            places = [(0, j * g.rc, (-1) ** j) for j in range(min(g.cps, 8)) if j * g.rc < g.limit(0)]
        elif level == "slot":
            if g.live_slots < 2:
                return None
            places = [(v, g.slot_range(v, s)[0], (-1) ** s) for v in range(min(g.nsets, 2))
                      for s in range(g.live_slots) if g.slot_range(v, s)]
        else:
            if g.nsets < 2:
                return None
            places = [(v, 0, (-1) ** v) for v in range(g.nsets)]
        return _pts(g, places)
    return build


def _r2_tree(sign):
    """slots a = 1 and b = 1 + stride hold m Q and Q in their first bucket, alone in their set: the tree of reduce2
    meets v_a = rc per (m + 1) Q + m Q and v_b = (rc per + 1) Q, made equal or opposite by m"""
    def build(g):
        if g.live_slots < 3:
            return None
        stride = 1
        while 1 + 2 * stride < g.live_slots:
            stride *= 2
        w = g.rc * g.per
        m = _inv(w + 1) if sign > 0 else -(2 * w + 1) * _inv(w + 1) % R
        places = []
        for v in {0, g.nsets - 1}:
            a, b = g.slot_range(v, 1), g.slot_range(v, 1 + stride)
            if a and b:
                places += [(v, a[0], m), (v, b[0], 1)]
        return _pts(g, places) if places else None
    return build


def single_positions(g):
    """(label, set, local bucket) of the single_bucket pictures"""
    last = g.nsets - 1
    pos = [("t=1", 0, 0), ("last", last, g.limit(last) - 1)]
    if g.cps > 1:
        pos += [("chunk1.first", 0, g.rc), ("chunk1.last", 0, 2 * g.rc - 1)]
    if g.live_slots > 1:
        lo, hi = g.slot_range(0, 1)
        pos += [("slot1.first", 0, lo), ("slot1.last", 0, hi)]
    if g.nsets > 1:
        pos += [("set1.first", 1, 0), ("set1.last", 1, g.limit(1) - 1)]
    if g.kind == "plain":                                         # the same positions in the top window
        lim = g.limit(last)
        pos += [("top." + name, last, min(l, lim - 1)) for name, v, l in list(pos) if v == 0]
    return [(name, v, l) for name, v, l in pos if l < g.limit(v)]


SINGLE_LABELS = ("t=1", "last", "chunk1.first", "chunk1.last", "slot1.first", "slot1.last", "set1.first", "set1.last",
                 "top.t=1", "top.chunk1.first", "top.chunk1.last", "top.slot1.first", "top.slot1.last")
CLASS_DIGITS = ("1", "2", "3", "4", "16", "63", "64", "65", "128", "H-1", "H")


def _single(label):
    def build(g):
        for name, v, l in single_positions(g):
            if name == label:
                return _pts(g, [(v, l, 1)])
        return None
    return build


def _class_digit(label):
    def build(g):
        if g.kind != "class":
            return None
        t = g.H - 1 if label == "H-1" else g.H if label == "H" else int(label)
        return [t], [K], set()
    return build


def _inv(a):
    return pow(a % R, -1, R)


def _total_is_infinity(g):
    """nonzero set sums whose fold is the point at infinity: Q in one bucket, -(w0 / w1) Q in another set"""
    v1 = g.nsets - 1
    l1 = min(3, g.limit(v1) - 1)
    if (v1, l1) == (0, 0):
        return None
    m = -g.weight(0, 0) * _inv(g.weight(v1, l1)) % R
    return _pts(g, [(0, 0, 1), (v1, l1, m)])


def _one_w_one_t_infinity(g):
    """set a: Q, -Q in buckets 0, 1 (T_a = infinity, W_a = -Q); set b: 2Q, -Q (W_b = infinity, T_b = Q); Q elsewhere"""
    a, b = 0, min(1, g.nsets - 1)
    if g.limit(b) < 2:
        return None
    places = [(b, 0, 2), (b, 1, -1)]
    if a != b:
        places += [(a, 0, 1), (a, 1, -1)]
    places += [(v, 0, 1) for v in range(2, min(g.nsets, 6))]
    return _pts(g, places)


def _class_relations(which):
    def build(g):
        if g.kind != "class":
            return None
        if which == "2W=T":          # y_v = 2 W - T: the addition of -T meets its opposite
            places = [(v, 0, -3) for v in (1, 33)] + [(v, 1, 1) for v in (1, 33)]
        elif which == "2W=-T":       # ... meets itself: a doubling
            places = [(v, 0, -5) for v in (1, 33)] + [(v, 1, 3) for v in (1, 33)]
        elif which == "W=T":
            places = [(v, 0, 1) for v in (3, 35, 41)]
        elif which == "equal_T":     # neighbouring slices of a class with equal totals: the segmented scan doubles
            places = [(v, 0, 1) for v in (2, 3, 4, 5, 36, 37, 40, 41)]
        elif which == "opposite_T":
            places = [(v, 0, (-1) ** v) for v in (2, 3, 4, 5, 36, 37, 40, 41)]
        elif which == "equal_y_xor1":   # y_0 = y_1: lanes that meet in the first all-reduce step
            places = [(0, 0, 1), (1, 0, 1)]
        elif which == "equal_y_stride32":   # y_0 = 4 Q = y_32 = 4 (2 Q - Q), y_10 = 4 Q = y_42 = 64 (Q / 16): slots that meet
            places = [(0, 0, 4), (32, 0, 1), (10, 0, 4), (42, 0, _inv(16))]   # at the top of the tree / in the last step
        elif which == "opposite_y":
            places = [(0, 0, 4), (32, 0, -1), (2, 0, 1), (3, 0, -1)]
        else:                        # class X alone: first and last bucket
            places = [(42, 0, 1), (42, g.ks - 1, 1)]
        return _pts(g, places)
    return build


CLASS_RELATIONS = ("2W=T", "2W=-T", "W=T", "equal_T", "opposite_T", "equal_y_xor1", "equal_y_stride32", "opposite_y",
                   "X_only")


def _horner(sign, w):
    def build(g):
        if g.kind != "plain" or g.nwin < 3:
            return None
        lo = w if w >= 0 else g.nwin - 2 + w + 1                  # w = -1: the two top windows
        places = [(lo + 1, 0, 1), (lo, 0, sign * (1 << g.c))]
        sc, lg, inf = _pts(g, places)
        if lo:                                                    # an unrelated point in the lowest window
            sc, lg = sc + [g.scalar(0, 0)], lg + [K2]
        return sc, lg, inf
    return build


def _merged(which):
    def build(g):
        if g.kind != "merged" or g.nsets < 2:
            return None
        if which == "equal_tot":
            places = [(v, 0, 1) for v in range(g.nsets)]
        elif which == "opposite_tot":
            places = [(v, 0, (-1) ** v) for v in range(g.nsets)]
        elif which == "last_is_infinity":     # xs = Ks Q, ysum = S_0 + S_1 = -Ks Q
            places = [(1, 0, 1), (0, 0, -(g.ks + 1))]
        else:                                  # ysum = Ks Q: the last addition is a doubling
            places = [(1, 0, 1), (0, 0, g.ks - 1)]
        return _pts(g, places)
    return build


def _heavy(phase, pattern, light=False):
    def build(g):
        segs = g.heavy_block if phase == 2 else 4                 # segments of the bucket: extra = segs - 1
        n = segs * g.seg
        signs = {"equal": lambda i: 1, "pairs": lambda i: (-1) ** i, "halves": lambda i: 1 if i < n // 2 else -1}[pattern]
        sc, lg = [g.scalar(0, 0)] * n, [signs(i) * K % R for i in range(n)]
        if light:                                                 # the neighbour bucket holds the heavy bucket's sum
            sc, lg = sc + [g.scalar(0, 1)], lg + [n * K % R]
        return sc, lg, set()
    return build


def _with_infinity_points(inner):
    def build(g):
        out = inner(g)
        if out is None:
            return None
        sc, lg, _ = out
        inf = set(range(0, len(sc), 3))
        return sc, [0 if i in inf else k for i, k in enumerate(lg)], inf
    return build


def pictures():
    """every picture, in the order the GPU test runs them.  The last column is the reach table: the (cell, kind) pairs
    that `walk` reports for the picture wherever it applies (cells: heavy1 heavy2 reduce1 r2.serial r2.scan r2.mul
    r2.combine r2.tree fold.horner fold.scan fold.y fold.tree fold.last; kinds: inf equal opposite, and "empty" for
    two infinities)."""
    P = Picture
    out = [
        P("every_bucket_equal", "every", _every_bucket_equal, [("reduce1", "equal"), ("r2.scan", "equal"),
                                                               ("r2.tree", "generic")], std=True),
        P("one_per_slot.first", "slot", _one_per_slot(False), [("reduce1", "inf"), ("r2.scan", "equal")], std=True),
        P("one_per_slot.last", "slot", _one_per_slot(True), [("reduce1", "equal"), ("r2.scan", "equal")]),
        P("r2_tree.equal", "slot", _r2_tree(1), [("r2.tree", "equal")]),
        P("r2_tree.opposite", "slot", _r2_tree(-1), [("r2.tree", "opposite"), ("r2.tree", "inf")]),
        P("alternating.bucket", "alt", _alternating("bucket"), [("reduce1", "opposite"), ("reduce1", "inf")]),
        P("alternating.chunk", "alt", _alternating("chunk"), [("reduce1", "inf")]),
        P("alternating.slot", "alt", _alternating("slot"), [("r2.scan", "opposite"), ("r2.scan", "inf")]),
        P("alternating.slice", "alt", _alternating("slice"), [("reduce1", "inf")]),
    ]
    out += [P("single_bucket." + s, "single", _single(s), [("reduce1", "inf")], std=s == "last") for s in SINGLE_LABELS]
    out += [P("single_bucket.class.t=" + s, "single", _class_digit(s), [("reduce1", "inf")]) for s in CLASS_DIGITS]
    out += [
        P("total_is_infinity", "total", _total_is_infinity, [], std=True),
        P("one_W_and_one_T_infinity", "total", _one_w_one_t_infinity, [("reduce1", "opposite")]),
    ]
    class_reach = {"2W=T": [("fold.y", "opposite")], "2W=-T": [("fold.y", "equal")], "W=T": [("fold.y", "opposite")],
                   "equal_T": [("fold.scan", "equal")], "opposite_T": [("fold.scan", "opposite"), ("fold.scan", "inf")],
                   "equal_y_xor1": [("fold.tree", "equal")], "equal_y_stride32": [("fold.tree", "equal")],
                   "opposite_y": [("fold.tree", "opposite")], "X_only": [("fold.tree", "inf")]}
    # W = T: 2 W - T adds -T to 2 T -- neither equal nor opposite; what it reaches is y_v = T_v: wave A and wave B of
    # the fold then hold the same point
    class_reach["W=T"] = [("fold.tree", "inf")]
    out += [P("class_slice_relations." + w, "relations", _class_relations(w), class_reach[w], std=w == "2W=-T")
            for w in CLASS_RELATIONS]
    out += [
        P("horner_relations.doubling", "relations", _horner(1, 1), [("fold.horner", "equal")], std=True),
        P("horner_relations.doubling_low", "relations", _horner(1, 0), [("fold.horner", "equal")]),
        P("horner_relations.doubling_top", "relations", _horner(1, -1), [("fold.horner", "equal")]),
        P("horner_relations.back_to_infinity", "relations", _horner(-1, 1), [("fold.horner", "opposite"),
                                                                             ("fold.horner", "inf")]),
        P("horner_relations.back_to_infinity_top", "relations", _horner(-1, -1), [("fold.horner", "opposite"),
                                                                                  ("fold.horner", "inf")]),
        P("merged_relations.equal_tot", "relations", _merged("equal_tot"), [("fold.scan", "equal"),
                                                                            ("fold.tree", "equal")], std=True),
        P("merged_relations.opposite_tot", "relations", _merged("opposite_tot"), [("fold.scan", "opposite"),
                                                                                  ("fold.tree", "opposite")]),
        P("merged_relations.last_is_infinity", "relations", _merged("last_is_infinity"), [("fold.last", "opposite")]),
        P("merged_relations.last_is_doubling", "relations", _merged("last_is_doubling"), [("fold.last", "equal")]),
        P("heavy_equal.tree", "heavy", _heavy(2, "equal"), [("heavy2", "equal"), ("heavy2", "inf")], std=True),
        P("heavy_equal.thread", "heavy", _heavy(1, "equal"), [("heavy1", "equal")]),
        P("heavy_alternating.tree", "heavy", _heavy(2, "pairs"), [("heavy2", "empty")]),
        P("heavy_halves.tree", "heavy", _heavy(2, "halves"), [("heavy2", "opposite")]),
        P("heavy_alternating.thread", "heavy", _heavy(1, "pairs"), []),
        P("heavy_halves.thread", "heavy", _heavy(1, "halves"), [("heavy1", "opposite"), ("heavy1", "equal")]),
        P("heavy_plus_light", "heavy", _heavy(2, "equal", light=True), [("heavy2", "equal"), ("reduce1", "equal")]),
        P("with_infinity_points.every_bucket_equal", "infpts", _with_infinity_points(_every_bucket_equal), []),
        P("with_infinity_points.one_per_slot", "infpts", _with_infinity_points(_one_per_slot(True)), []),
        P("with_infinity_points.alternating", "infpts", _with_infinity_points(_alternating("bucket")), []),
    ]
    return out


def realise(pic, registered, is_g1, env):
    """the geometry of a process with these knobs for the picture's own point count (the cost model picks the window
    from n, and the picture's n follows from the window: iterate to the fixed point) and the picture there, or None
    where the picture does not apply"""
    n = 1
    for _ in range(8):
        g = geometry(n, registered, is_g1, env)
        out = pic.build(g)
        if out is None:
            return None
        if len(out[0]) == n:
            return g, out
        n = len(out[0])
    raise AssertionError(f"{pic.name}: no stable geometry for {env}")


def cases(knobs, families, registered, is_g1):
    """(picture, geometry, (scalars, logs, infinities)) of everything one (knob set, set kind, group) runs"""
    for pic in pictures():
        if pic.family in families:
            got = realise(pic, registered, is_g1, knobs)
            if got is not None:
                yield pic, got[0], got[1]


# ---- the log-space walk ---------------------------------------------------------------------------------------------
def digits(s, c, nwin):
    """msm_digits: the signed c-bit digits of a scalar -> (window, magnitude, negative)"""
    out, carry, half, mask = [], 0, 1 << (c - 1), (1 << c) - 1
    for w in range(nwin):
        raw = (s & mask) + carry
        neg = raw > half
        mag = (1 << c) - raw if neg else raw
        carry = int(neg)
        if mag:
            out.append((w, mag, neg))
        s >>= c
    return out


def bucket_entries(g, scalars, logs, infs):
    """global bucket -> the logs of the (table) points accumulated into it, in point order"""
    compact = g.registered and infs and len(infs) * 100 >= INF_COMPACT_PCT * len(scalars)
    buckets = defaultdict(list)
    for i, (s, k) in enumerate(zip(scalars, logs)):
        if s == 0 or (compact and i in infs):
            continue
        for w, mag, neg in digits(s, g.c, g.nwin):
            if g.kind == "plain":
                b, val = w * g.H + mag - 1, k
            elif g.kind == "merged":
                b, val = mag - 1, k << (g.c * w)
            else:
                b, sel = class_bucket(mag, g.c)
                val = k << (g.c * w + sel)
            buckets[b].append((-val if neg else val) % R)
    return buckets


def walk(g, picture):
    """The sums of msm_heavy, msm_reduce1, msm_reduce2 and the fold on the logs of the points, mod r, in the order and
    grouping of the kernels: segment sums of a split bucket by one thread or by an LDS tree of halving stride; running
    sums over `rc` buckets; slot ranges of `per` chunks, suffix scan by doubling distance, mul_small as double-and-add,
    tree by halving stride; the fold of the plan.  Returns {cell: Counter(kind)}: how many additions of that cell met
    exactly one operand at infinity ("inf"), equal operands, opposite operands, neither ("generic") or two infinities
    ("empty").

    It exists ONLY to show that a picture reaches the branches it is built for.  No expected value comes from it: the
    tests compare the GPU with (sum s_i k_i mod r) * G.  (Within a bucket the sort keeps no particular order; the walk
    takes point order, which matters to no picture whose reach is asserted except through equal-sized runs.)"""
    scalars, logs, infs = picture
    t = defaultdict(Counter)

    def add(cell, a, b):
        a, b = a % R, b % R
        kind = ("empty" if a == 0 and b == 0 else "inf" if a == 0 or b == 0 else "equal" if a == b
                else "opposite" if (a + b) % R == 0 else "generic")
        t[cell][kind] += 1
        return (a + b) % R

    def mul_small(cell, p, k):
        r = 0
        for bit in range(k.bit_length() - 1, -1, -1):
            r = 2 * r % R
            if (k >> bit) & 1:
                r = add(cell, r, p)
        return r

    # msm_accum (not walked) and msm_heavy
    partial = {}
    for b, vals in bucket_entries(g, scalars, logs, infs).items():
        segs = [sum(vals[i:i + g.seg]) % R for i in range(0, len(vals), g.seg)]
        e = len(segs) - 1
        if e == 0:
            acc = segs[0]
        elif e < HEAVY_MIN:
            acc = segs[0]
            for s in segs[1:]:
                acc = add("heavy1", acc, s)
        else:
            B = g.heavy_block
            sh = [0] * B
            for th in range(B):
                for s in range(th, e + 1, B):
                    sh[th] = add("heavy2", sh[th], segs[s])
            stride = B // 2
            while stride:
                for th in range(stride):
                    sh[th] = add("heavy2", sh[th], sh[th + stride])
                stride >>= 1
            acc = sh[0]
        partial[b] = acc
    # msm_reduce1: chunks without a bucket that has entries leave (infinity, infinity) and are not walked
    chunkR, chunkA = {}, {}
    for j in sorted({b // g.rc for b in partial}):
        run = acc = 0
        for k in range(g.rc - 1, -1, -1):
            b = j * g.rc + k
            if b in partial:
                run = add("reduce1", run, partial[b])
            acc = add("reduce1", acc, run)
        chunkR[j], chunkA[j] = run, acc
    # msm_reduce2 per set: sets without such a chunk give (infinity, infinity)
    M, S, per = g.cps, g.slots, g.per
    W, T = [0] * g.nsets, [0] * g.nsets
    for v in sorted({j // M for j in chunkR}):
        run, wsum, sumA = [0] * S, [0] * S, [0] * S
        for slot in range(g.live_slots):
            lo = slot * per
            for m in range(min(lo + per, M) - 1, lo - 1, -1):
                j = v * M + m
                wsum[slot] = add("r2.serial", wsum[slot], run[slot])
                run[slot] = add("r2.serial", run[slot], chunkR.get(j, 0))
                sumA[slot] = add("r2.serial", sumA[slot], chunkA.get(j, 0))
        incl, d = run[:], 1
        while d < S:
            incl = [add("r2.scan", incl[s], incl[s + d]) if s + d < S else incl[s] for s in range(S)]
            d <<= 1
        T[v] = incl[0]
        sh = []
        for slot in range(S):
            x = mul_small("r2.mul", incl[slot], per) if slot >= 1 and slot * per < M else 0
            x = add("r2.combine", x, wsum[slot])
            x = mul_small("r2.mul", x, g.rc)
            sh.append(add("r2.combine", x, sumA[slot]))
        stride = S // 2
        while stride:
            for s in range(stride):
                sh[s] = add("r2.tree", sh[s], sh[s + stride])
            stride >>= 1
        W[v] = sh[0]

    def allreduce(v):
        d = 1
        while d < 64:
            v = [add("fold.tree", v[lane], v[lane ^ d]) for lane in range(64)]
            d <<= 1
        return v[0]

    def tree64(sh):
        stride = 32
        while stride:
            for s in range(stride):
                sh[s] = add("fold.tree", sh[s], sh[s + stride])
            stride >>= 1
        return sh[0]

    if g.fold == PLAIN:
        r = 0
        for w in range(g.nwin - 1, -1, -1):
            r = add("fold.horner", r << g.c, W[w])
    elif g.fold == MERGED:
        y = allreduce([W[v] if v < g.nsets else 0 for v in range(64)])
        suf, d = [T[v] if v < g.nsets else 0 for v in range(64)], 1
        while d < 64:
            suf = [add("fold.scan", suf[lane], suf[lane + d]) if lane + d < 64 else suf[lane] for lane in range(64)]
            d <<= 1
        suf[0] = 0
        r = add("fold.last", allreduce(suf) << g.plan.log2ks, y)
    else:
        z = [0 if v < 32 else 1 if v < 40 else 2 if v < 42 else 3 for v in range(64)]
        first, end = (0, 32, 40, 42), (32, 40, 42, 43)
        suf, d = [T[v] if v < 43 and z[v] < 3 else 0 for v in range(64)], 1
        while d < 32:
            suf = [add("fold.scan", suf[v], suf[(v + d) & 63]) if v + d < end[z[v]] and z[v] < 3 else suf[v]
                   for v in range(64)]
            d <<= 1
        suf = [0 if v == first[z[v]] or z[v] == 3 or v >= 43 else suf[v] << (2 * z[v]) for v in range(64)]
        ys = []
        for v in range(64):
            y = 2 * W[v] % R if v < 43 else 0
            if v < 43 and z[v] < 3:
                y = add("fold.y", y, -T[v] % R)
            ys.append(y << (0, 2, 4, 5)[z[v]])
        if g.fold == CLASSES_QUAD:
            xs, y = tree64(suf), tree64(ys)
        else:
            y, xs = allreduce(ys), allreduce(suf)
        r = add("fold.last", xs << (g.plan.log2ks + 1), y)
    t["result"]["log"] = r % R
    return t


def coarse(cell):
    """the stage of a cell: heavy, reduce1, r2, fold"""
    return "heavy" if cell.startswith("heavy") else cell.split(".")[0]
