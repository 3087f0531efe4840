"""msm_plan.hpp on the CPU: the launch plan of an MSM -- window and parameters, the grids and the workspace of the sort,
the job workspace, and which reduce2 / fold kernel forms the tail -- held to a restatement of the rule, to invariants,
to recorded values and to its boundaries, for every knob set that tests/test_gpu_knobs.py runs on the GPU."""
import ctypes

import pytest

from tests.test_device_headers_cpu import shim  # noqa: F401  (the fixture that builds and loads the CPU shim)
from tests.test_gpu_knobs import KNOBS

# msm_params.hpp
FR_BITS, MSM_BLOCK = 254, 256
BS_LOG, BS_LOW, BS_SPLIT = 9, 512, 8
PART_TILE, PART_MAX = 4096, 8192
PERM_BINS, PERM_BLOCK = 256, 512
SCAN_TILE = 2048
CLASS_SLICES = 43

QUAD128, QUAD64, WIDE, NARROW, WAVE = range(5)           # MsmR2
CLASSES_QUAD, CLASSES, MERGED, PLAIN = range(4)          # MsmFold

SORT_PARTS = ("count", "cursor", "offset", "xoff", "heavy", "info", "tiles", "entries", "xseg", "perm", "ghist",
              "blk_base", "tile_hist", "tmp", "tiles2", "slice_hist")
ACC = {True: (128, 144), False: (256, 288)}               # is_g1 -> bytes of a standard / a reduced-radix accumulator

NS = [1, 2, 3, 64, 700, 3000, 2046, 1 << 15, (1 << 17) - 1, 1 << 17, 1 << 20, 1 << 22, 1 << 23, (1 << 26) - 1]


def parse_knobs(env):
    """G16_* variables -> the knob values as the library reads them at start-up (ranges, defaults and spellings
    restated); the variables that no MSM launch looks at are ignored"""
    def num(name, lo, hi):
        v = int(env.get(name, 0))
        return v if lo <= v <= hi else 0
    k = dict(msm_window=num("G16_MSM_WINDOW", 5, 22), table_window=num("G16_TABLE_WINDOW", 5, 22),
             msm_seg=num("G16_MSM_SEG", 8, 4096), msm_sort=ord(env["G16_MSM_SORT"][0]) if "G16_MSM_SORT" in env else 0,
             red_slice_log2=num("G16_RED_SLICE", 8, 11), r2_width=-1, mtab=2, tail_quad=1, red_chunk=0,
             heavy_grid=num("G16_HEAVY_GRID", 1, 4096))
    if "G16_R2_WIDTH" in env:
        k["r2_width"] = {"0": 0, "2": 2}.get(env["G16_R2_WIDTH"][0], 1)
    if "G16_MTAB" in env:
        k["mtab"] = 1 if env["G16_MTAB"][0] == "1" else 2
    if "G16_TAIL_QUAD" in env:
        k["tail_quad"] = 0 if env["G16_TAIL_QUAD"][0] == "0" else 1
    if "G16_RED_CHUNK" in env:
        k["red_chunk"] = int(env["G16_RED_CHUNK"]) if int(env["G16_RED_CHUNK"]) in (2, 4, 8, 16) else 0
    return k


KNOB_ORDER = ("msm_window", "table_window", "msm_seg", "msm_sort", "red_slice_log2", "r2_width", "mtab", "tail_quad",
              "red_chunk", "heavy_grid")


def pick_window(n, merged, forced, cmax):
    """the cost model: 10 modmul per mixed add over n * nwin entries + 28 per bucket over the bucket sets; no window
    whose entries overflow 31 bits or whose top window is shorter than min(c - 2, 6) bits"""
    if forced:
        return forced
    best, best_cost = 5, 1e300
    for c in range(5, cmax + 1):
        nwin = FR_BITS // c + 1
        if (nwin * n) >> 31:
            continue
        if FR_BITS - (nwin - 1) * c < min(c - 2, 6) and c > 5:
            continue
        cost = 10.0 * float(n) * nwin + 28.0 * (1.0 if merged else float(nwin)) * float(1 << (c - 1))
        if cost < best_cost:
            best, best_cost = c, cost
    return best


def table_buckets(c, mtab):
    h = 1 << (c - 1)
    return h // 2 + h // 8 + h // 32 + h // 64 if mtab == 2 else h


def carve(sizes):
    """parts one after the other, each rounded up to 256 bytes -> (offsets, total)"""
    offs, at = [], 0
    for s in sizes:
        offs.append(at)
        at += (s + 255) & ~255
    return offs, at


def msm_plan_rule(n, registered, is_g1, narrow_tail, k, flags=1):
    """the whole rule, restated from the launch code as it stood before msm_plan.hpp existed -> the 57 values of
    shim_msm_plan"""
    # window and parameters
    if registered:
        c = pick_window(max(n, 1), True, k["table_window"], 22)
        mtab = 2 if k["mtab"] == 2 and c >= 15 else 1
    else:
        c, mtab = pick_window(max(n, 1), False, k["msm_window"], 16), 1
    nwin = FR_BITS // c + 1
    tables = 1 if registered else 0
    nb = table_buckets(c, mtab) if tables else nwin << (c - 1)
    avg = (n * nwin * 2) // (1 << (c - 1)) + 1 if mtab == 2 else (n * nwin) // nb + 1
    seg = ((avg + avg // 4 + 15) // 16) * 16
    seg = max(min(seg, ((n * nwin // 65536 + 15) // 16) * 16), 32)
    if k["msm_seg"]:
        seg = k["msm_seg"]
    max_extra = n * nwin // seg + 1
    params = [n, c, nwin, nb, seg, flags & 1, tables, max_extra, mtab]
    # the sort
    lo_bits = min(c - 1, BS_LOG)
    while lo_bits and nb % (1 << lo_bits):
        lo_bits -= 1
    nparts = nb >> lo_bits
    ptiles = -(-n // PART_TILE)
    use_part = nparts <= PART_MAX and k["msm_sort"] != ord("a")
    nth = nparts * ptiles
    fused = use_part and lo_bits == BS_LOG
    sort = [lo_bits, nparts, ptiles, nth, int(use_part), int(fused), -(-n // MSM_BLOCK), -(-nb // SCAN_TILE),
            -(-nth // SCAN_TILE), -(-nb // PERM_BLOCK)]
    sort_offs, sort_total = carve([
        nb * 4, nb * 4, (nb + 1) * 4, nb * 4, nb * 4, 64, -(-nb // SCAN_TILE) * 8, n * nwin * 4, max_extra * 8, nb * 4,
        PERM_BINS * 4, -(-nb // PERM_BLOCK) * PERM_BINS * 4, nth * 4 if use_part else 4, n * nwin * 8 if use_part else 8,
        -(-nth // SCAN_TILE) * 8 + 8, nparts * BS_SPLIT * BS_LOW * 4 if use_part else 4])
    # the tail
    rc = k["red_chunk"] or (4 if nb <= 1 << 17 else 16)
    nchunks = nb // rc
    nsets, log2ks = nwin, 0
    if tables and mtab == 2:
        nsets, log2ks = CLASS_SLICES, c - 7
    elif tables:
        cps = min(nchunks, 1 << (k["red_slice_log2"] or 9))
        while nchunks // cps > 64:
            cps <<= 1
        nsets, log2ks = nchunks // cps, (cps * rc).bit_length() - 1
    cps = nchunks // nsets
    wide = 512 if is_g1 else 256
    quad = k["r2_width"] < 0 and k["tail_quad"] != 0
    if quad:
        r2, threads, lds = (QUAD128, 512, 128) if is_g1 and cps >= 512 else (QUAD64, 256, 64)
    else:
        width = k["r2_width"] if k["r2_width"] >= 0 else (1 if narrow_tail and rc > 4 else 0)
        r2, threads = {0: (WIDE, wide), 2: (WAVE, 64)}.get(width, (NARROW, wide // 4))
        lds = threads
    if tables and mtab == 2:
        fold = CLASSES_QUAD if quad else CLASSES
    else:
        fold = MERGED if tables else PLAIN
    jobs = []
    for asz, psz29 in (ACC[True], ACC[False]):
        offs, total = carve([(nb + max_extra) * psz29, nchunks * asz, nchunks * asz, (2 * 64 + 2) * asz])
        jobs += offs + [total]
    tail = [rc, nchunks, nsets, log2ks, cps, r2, threads, lds, fold, k["heavy_grid"] or 1024, k["heavy_grid"] or 512]
    return params + sort + sort_offs + [sort_total] + jobs + tail


class Plan:
    """the 57 values of shim_msm_plan by name"""

    def __init__(self, v):
        self.raw = list(v)
        (self.n, self.c, self.nwin, self.nbuckets, self.seg, self.scalars_mont, self.tables, self.max_extra,
         self.mtab) = v[0:9]
        (self.lo_bits, self.nparts, self.ptiles, self.nth, self.use_part, self.fused, self.nblk, self.ntiles, self.nt2,
         self.pblk) = v[9:19]
        self.sort_off = dict(zip(SORT_PARTS, v[19:35]))
        self.sort_bytes = v[35]
        self.job_off = {True: v[36:40], False: v[41:45]}
        self.job_bytes = {True: v[40], False: v[45]}
        (self.rc, self.nchunks, self.nsets, self.log2ks, self.cps, self.r2, self.r2_threads, self.r2_lds, self.fold,
         self.heavy1, self.heavy3) = v[46:57]


def run_plan(shim, n, registered, is_g1, narrow_tail, env, flags=1):  # noqa: F811
    k = parse_knobs(env)
    knobs = (ctypes.c_int * len(KNOB_ORDER))(*[k[name] for name in KNOB_ORDER])
    out = (ctypes.c_uint64 * 57)()
    shim.shim_msm_plan.restype = None
    shim.shim_msm_plan.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                   ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint64)]
    shim.shim_msm_plan(n, flags, int(registered), int(is_g1), int(narrow_tail), knobs, out)
    return Plan(out)


def run_tail(shim, params, is_g1, narrow_tail, env):  # noqa: F811
    """the tail plan of parameters given field by field (n c nwin nbuckets seg scalars_mont tables max_extra mtab)"""
    k = parse_knobs(env)
    knobs = (ctypes.c_int * len(KNOB_ORDER))(*[k[name] for name in KNOB_ORDER])
    out = (ctypes.c_uint64 * 11)()
    shim.shim_msm_tail_plan.restype = None
    shim.shim_msm_tail_plan.argtypes = [ctypes.POINTER(ctypes.c_uint32), ctypes.c_int, ctypes.c_int,
                                        ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint64)]
    shim.shim_msm_tail_plan((ctypes.c_uint32 * 9)(*params), int(is_g1), int(narrow_tail), knobs, out)
    return list(out)


def grid():
    for env in [{}] + KNOBS:
        for n in NS:
            for registered in (False, True):
                for is_g1 in (True, False):
                    for narrow_tail in (False, True):
                        yield env, n, registered, is_g1, narrow_tail


def test_knob_list_is_the_gpu_suite_s():
    assert len(KNOBS) == 34


def test_plan_equals_the_restated_rule_on_the_whole_grid(shim):  # noqa: F811
    for env, n, registered, is_g1, narrow_tail in grid():
        got = run_plan(shim, n, registered, is_g1, narrow_tail, env).raw
        want = msm_plan_rule(n, registered, is_g1, narrow_tail, parse_knobs(env))
        assert got == want, (env, n, registered, is_g1, narrow_tail, [(i, g, w) for i, (g, w) in
                                                                      enumerate(zip(got, want)) if g != w])
    # the Montgomery flag is bit 0 of the C ABI's flags and nothing else of them
    assert run_plan(shim, 64, False, True, False, {}, flags=0).scalars_mont == 0
    assert run_plan(shim, 64, False, True, False, {}, flags=6).scalars_mont == 0
    assert run_plan(shim, 64, False, True, False, {}, flags=7).scalars_mont == 1


def test_plan_invariants_on_the_whole_grid(shim):  # noqa: F811
    for env, n, registered, is_g1, narrow_tail in grid():
        p = run_plan(shim, n, registered, is_g1, narrow_tail, env)
        where = (env, n, registered, is_g1, narrow_tail, p.raw)
        assert p.nbuckets % (1 << p.lo_bits) == 0 and p.nparts << p.lo_bits == p.nbuckets, where
        assert not p.use_part or p.nparts <= PART_MAX, where
        assert bool(p.fused) == bool(p.use_part and p.lo_bits == BS_LOG), where
        # the parts: 256-byte aligned, in order, none overlapping its successor, and they add up to the total
        offs = [p.sort_off[name] for name in SORT_PARTS] + [p.sort_bytes]
        assert offs[0] == 0 and all(o % 256 == 0 for o in offs) and offs == sorted(offs) and len(set(offs)) == 17, where
        assert p.sort_off["cursor"] - p.sort_off["count"] == p.sort_off["offset"] - p.sort_off["cursor"], where
        assert p.sort_off["offset"] - p.sort_off["count"] >= 8 * p.nbuckets, where    # one memset clears count + cursor
        for g1 in (True, False):
            jo = list(p.job_off[g1]) + [p.job_bytes[g1]]
            assert jo[0] == 0 and all(o % 256 == 0 for o in jo) and jo == sorted(jo) and len(set(jo)) == 5, where
            assert jo[1] >= (p.nbuckets + p.max_extra) * ACC[g1][1], where
            assert jo[3] - jo[2] >= p.nchunks * ACC[g1][0] and jo[4] - jo[3] >= 130 * ACC[g1][0], where
        assert 1 <= p.nsets <= 64, where
        assert p.nsets * p.cps * p.rc == p.nbuckets and p.nchunks * p.rc == p.nbuckets, where
        assert p.r2_lds * ACC[is_g1][0] <= 64 * 1024, where
        assert p.r2_threads == (4 * p.r2_lds if p.r2 in (QUAD128, QUAD64) else p.r2_lds), where
        assert (p.fold in (CLASSES_QUAD, CLASSES)) == bool(p.tables and p.mtab == 2), where
        if p.fold in (CLASSES_QUAD, CLASSES):
            assert p.nsets == CLASS_SLICES and p.nbuckets == CLASS_SLICES << p.log2ks, where
        if p.fold == MERGED:
            assert p.nsets << p.log2ks == p.nbuckets, where
        # the grids cover what they are launched over
        assert p.nblk * MSM_BLOCK >= p.n and p.ptiles * PART_TILE >= p.n, where
        assert p.ntiles * SCAN_TILE >= p.nbuckets and p.pblk * PERM_BLOCK >= p.nbuckets, where
        assert p.nth == p.nparts * p.ptiles and p.nt2 * SCAN_TILE >= p.nth, where


def test_recorded_plan_of_a_registered_set_of_2p20(shim):  # noqa: F811
    """the figures of the 2^20 key, default knobs"""
    for is_g1 in (True, False):
        p = run_plan(shim, 1 << 20, True, is_g1, False, {})
        assert (p.c, p.nwin, p.mtab, p.nbuckets, p.seg, p.max_extra) == (20, 13, 2, 352256, 80, 170394)
        assert (p.lo_bits, p.nparts, p.ptiles, p.use_part, p.fused) == (9, 688, 256, 1, 1)
        assert p.sort_bytes == 186080256
        assert (p.rc, p.nchunks, p.nsets, p.cps, p.log2ks) == (16, 22016, 43, 512, 13)
        assert (p.job_bytes[True], p.job_bytes[False]) == (80914432, 161828864)
        assert (p.r2, p.r2_threads) == ((QUAD128, 512) if is_g1 else (QUAD64, 256))
        assert p.fold == CLASSES_QUAD
        assert (p.heavy1, p.heavy3) == (1024, 512)


def test_plan_boundaries(shim):  # noqa: F811
    n = 1 << 17
    # the reduce chunk: 4 buckets up to 2^17 buckets, 16 beyond
    p = run_plan(shim, n, True, True, False, {"G16_TABLE_WINDOW": "18"})
    assert (p.c, p.nbuckets, p.rc) == (18, 88064, 4) and p.nbuckets <= 1 << 17
    p = run_plan(shim, n, True, True, False, {"G16_TABLE_WINDOW": "19"})
    assert (p.c, p.nbuckets, p.rc) == (19, 176128, 16)
    # G1: the 128-slot quad kernel from 512 chunks per set
    assert (p.cps, p.r2, p.r2_threads, p.r2_lds) == (256, QUAD64, 256, 64)
    p = run_plan(shim, n, True, True, False, {"G16_TABLE_WINDOW": "20"})
    assert (p.cps, p.r2, p.r2_threads, p.r2_lds) == (512, QUAD128, 512, 128)
    assert run_plan(shim, n, True, False, False, {"G16_TABLE_WINDOW": "20"}).r2 == QUAD64          # never for G2
    # 511 chunks in one set: a merged bucket set of 2044 buckets, which no window produces
    t = run_tail(shim, [n, 12, 22, 2044, 32, 1, 1, 1, 1], True, False, {})
    assert t[:6] == [4, 511, 1, 10, 511, QUAD64]
    t = run_tail(shim, [n, 12, 22, 2048, 32, 1, 1, 1, 1], True, False, {})
    assert t[:6] == [4, 512, 1, 11, 512, QUAD128]
    # G16_R2_WIDTH: the one-lane kernels, whatever G16_TAIL_QUAD says, and the one-lane fold behind them
    for width, r2, g1_threads, g2_threads in (("0", WIDE, 512, 256), ("1", NARROW, 128, 64), ("2", WAVE, 64, 64)):
        for narrow_tail in (False, True):
            for is_g1 in (True, False):
                p = run_plan(shim, n, True, is_g1, narrow_tail, {"G16_R2_WIDTH": width, "G16_TAIL_QUAD": "1"})
                assert (p.r2, p.r2_threads, p.r2_lds) == (r2, *(2 * [g1_threads if is_g1 else g2_threads]))
                assert p.fold == CLASSES
    # G16_TAIL_QUAD=0: narrow only where the caller overlaps the tail and the chunks are longer than 4 buckets
    for window, narrow_tail, r2 in (("19", True, NARROW), ("19", False, WIDE), ("18", True, WIDE), ("18", False, WIDE)):
        p = run_plan(shim, n, True, True, narrow_tail, {"G16_TAIL_QUAD": "0", "G16_TABLE_WINDOW": window})
        assert (p.r2, p.fold) == (r2, CLASSES) and (p.rc > 4) == (window == "19")
    p = run_plan(shim, n, True, True, True, {"G16_TAIL_QUAD": "0", "G16_TABLE_WINDOW": "18", "G16_RED_CHUNK": "8"})
    assert (p.rc, p.r2) == (8, NARROW)
    # one table per window: the plain bucket set in <= 64 slices behind the merged fold
    p = run_plan(shim, 1 << 20, True, True, False, {"G16_MTAB": "1"})
    assert (p.mtab, p.nbuckets, p.fold, p.nsets, p.cps, p.log2ks) == (1, 1 << 19, MERGED, 64, 512, 13)
    assert run_plan(shim, n, True, True, False, {"G16_TABLE_WINDOW": "14"}).fold == MERGED           # c < 15
    # a plain MSM: the windows are the sets
    p = run_plan(shim, 1 << 20, False, True, False, {})
    assert (p.c, p.tables, p.fold, p.nsets, p.log2ks, p.nsets) == (16, 0, PLAIN, p.nwin, 0, 16)
    # the partition sort, and the global-atomic sort where it is forced or the partitions exceed the LDS histogram
    stubs = {"tile_hist": 4, "tmp": 8, "slice_hist": 4}
    p = run_plan(shim, 1 << 20, True, True, False, {})
    part_bytes = p.sort_bytes
    assert p.use_part and p.sort_off["tmp"] - p.sort_off["tile_hist"] == p.nth * 4
    assert p.sort_off["tiles2"] - p.sort_off["tmp"] == (1 << 20) * p.nwin * 8
    for env, registered in (({"G16_MSM_SORT": "a"}, True), ({"G16_MSM_WINDOW": "20"}, False)):
        p = run_plan(shim, 1 << 20, registered, True, False, env)
        assert not p.use_part and not p.fused and (p.nparts > PART_MAX) == (not registered)
        order = list(SORT_PARTS) + ["end"]
        off = dict(p.sort_off, end=p.sort_bytes)
        for name, size in stubs.items():
            assert off[order[order.index(name) + 1]] - off[name] == 256 and size <= 256
        assert off["slice_hist"] - off["tiles2"] == ((-(-p.nth // SCAN_TILE) * 8 + 8 + 255) & ~255)   # tiles2 keeps its size
    p = run_plan(shim, 1 << 20, True, True, False, {"G16_MSM_SORT": "a"})
    assert part_bytes - p.sort_bytes > (1 << 20) * 13 * 8                                     # tmp alone is 8 B per entry
    # fewer low bits than BS_LOG: the partition sort without the fused bookkeeping
    p = run_plan(shim, 3000, True, True, False, {"G16_TABLE_WINDOW": "6"})
    assert (p.lo_bits, p.nparts, p.use_part, p.fused) == (5, 1, 1, 0)
    # the split-bucket combine: 1024 workgroups for one job, 512 each for a batch, or what G16_HEAVY_GRID says
    p = run_plan(shim, n, True, True, False, {"G16_HEAVY_GRID": "64"})
    assert (p.heavy1, p.heavy3) == (64, 64)


def test_class_slice_geometry(shim):  # noqa: F811
    """msm_class_slice (msm_params.hpp), which both class folds read: the classes cut the 43 slices into 32 + 8 + 2 + 1,
    and the doublings it hands the folds give the first bucket of every slice the weight that class_weight of
    tests/msm_pictures.py -- the inverse of msm_class_bucket, which knows nothing of slices -- says it has"""
    from tests.msm_pictures import class_weight                      # imported here: that module imports this one

    def class_slice(v):
        out = (ctypes.c_int32 * 5)()
        shim.shim_class_slice(v, out)
        return tuple(out)
    slices = [class_slice(v) for v in range(CLASS_SLICES)]
    classes = sorted({(z, first, end) for z, first, end, _, _ in slices})
    assert [end - first for _, first, end in classes] == [32, 8, 2, 1]
    assert [z for z, _, _ in classes] == [0, 1, 2, 3] and classes[0][1] == 0 and classes[-1][2] == CLASS_SLICES
    assert all(a[2] == b[1] for a, b in zip(classes, classes[1:]))
    for v, (z, first, end, dbl_y, dbl_e) in enumerate(slices):
        assert first <= v < end
        assert (dbl_y, dbl_e) == ((2 * z, 2 * z) if z < 3 else (5, 0))
    # the fold's  S = sum_v y_v + 2 Ks sum_v e_v T_v  at slice-local weight l = 1 (W_v = T_v = B, one bucket):
    # y_v = 2^dbl_y (2 W_v - T_v)  (X: 2^dbl_y * 2 W_v),  e_v = 2^dbl_e * sigma  (X: none)
    for c in (15, 20):
        ks = 1 << (c - 7)
        for v, (z, first, end, dbl_y, dbl_e) in enumerate(slices):
            sigma = v - first
            y, e = ((1 << dbl_y) * (2 - 1), (1 << dbl_e) * sigma) if z < 3 else ((1 << dbl_y) * 2, 0)
            assert y + 2 * ks * e == class_weight(v * ks, c), (c, v)
            assert class_weight(v * ks, c) == (4 ** z * (2 * sigma * ks + 1) if z < 3 else 64)
