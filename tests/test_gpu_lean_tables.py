"""Lean point sets on the GPU (include/g16hip.h "lean point sets"): window tables for every s-th window only, window
w = s j + r gathering from table j into bucket set r.  Whatever the stride, an MSM and a proof are the same canonical
bytes: every result here is held to the oracle AND to the same call against a stride-1 registration.

The sizes are the smallest at which nwin is no multiple of the stride, the last table is partial, and more than one
partition and segment exist."""
import copy
import ctypes

import pytest

from oracle import bn254_ref as o
from tests import inputs as I

pytestmark = pytest.mark.gpu
R = o.R
NS = (1, 2, 37, (1 << 10) + 3)


def _nwin(c):
    return 254 // c + 1


def _strides(group, n):
    """2, 3, 5, nwin and nwin + 7 (clamped), nwin being that of the window a large stride picks"""
    from nim_groth16_amd import points_plan
    nwin = _nwin(points_plan(group, n, 255)[0])
    return (2, 3, 5, nwin, nwin + 7)


def _points(orc, group, n, seed):
    """n points; from 8 points on: (0,0) at 0, the same point at 1 and 2, a point at 3 and its negation at 4"""
    psz = 64 if group == 1 else 128
    _, pts = I.points_with_logs(orc, group, n, seed)
    if n < 8:
        return pts, 0
    p = [pts[i * psz:(i + 1) * psz] for i in range(n)]
    p[0] = bytes(psz)
    p[2] = p[1]
    if group == 1:
        q = o.g1_from_bytes(p[3])
        p[4] = o.g1_to_bytes(o.G1.neg(q))
    else:
        q = o.g2_from_bytes(p[3])
        p[4] = o.g2_to_bytes(o.G2.neg(q))
    return b"".join(p), 1


def _special_scalars(windows):
    """0, 1, r - 1, and per window size c: every digit 2^(c-1) (top window left empty to stay below r); the same with the
    lowest digit one larger, so that the carry of the signed digits runs through every window into the top one; the only
    non-zero digit in window nwin - 1; and a single non-zero digit in every window w -- every residue class w mod s of
    every stride, in its first and in later tables"""
    out = [0, 1, R - 1]
    for c in sorted(windows):
        nwin, half = _nwin(c), 1 << (c - 1)
        every = sum(half << (c * w) for w in range(nwin - 1))
        out += [every, every + 1, 1 << (c * (nwin - 1))]
        out += [(1 + w % 3) << (c * w) for w in range(nwin - 1)]
    assert all(0 <= x < R for x in out)
    return out


def _scalar_vectors(n, windows, seed):
    """the special scalars dealt over vectors of n scalars, the rest uniform; from 8 scalars on the specials start at
    index 5 and scalars 3 and 4 (a point and its negation) are equal"""
    rng = o.SplitMix64(seed)
    sp = _special_scalars(windows)
    room = n - 5 if n >= 8 else n
    vecs = []
    for at in range(0, len(sp), room):
        v = [rng.fr() for _ in range(n)]
        chunk = sp[at:at + room]
        lo = 5 if n >= 8 else 0
        v[lo:lo + len(chunk)] = chunk
        if n >= 8:
            v[4] = v[3]
        vecs.append(I.fr_mont_bytes(v))
    return vecs


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("group", [1, 2])
def test_lean_msm_equals_the_oracle_and_the_stride_one_set(ctx, orc, group, n):
    from nim_groth16_amd import points_plan
    strides = _strides(group, n)
    pts, n_inf = _points(orc, group, n, 300 + n)
    windows = {points_plan(group, n, s)[0] for s in strides}
    vecs = _scalar_vectors(n, windows, 400 + n)
    full = ctx.register_points(group, pts, n)
    want = [orc.msm_naive(group, v, pts) for v in vecs]
    try:
        assert [ctx.msm_points(full, v) for v in vecs] == want
        for s in strides:
            c, ntables, nbytes = points_plan(group, n, s)
            h = ctx.register_points(group, pts, n, table_stride=s)
            try:
                assert h.info() == (c, ntables) and ntables == -(-_nwin(c) // min(s, _nwin(c))), (s, h.info())
                assert h.table_bytes == nbytes and h.inf_count() == n_inf
                for v, w in zip(vecs, want):
                    assert ctx.msm_points(h, v) == w, (group, n, s, c)
            finally:
                h.release()
        # the last stride was clamped: one table, like the stride before it
        assert points_plan(group, n, strides[-1]) == points_plan(group, n, strides[-2])
        assert points_plan(group, n, strides[-1])[1] == 1
    finally:
        full.release()


def test_lean_msm_standard_form_scalars_and_device_points(ctx, orc):
    """the other two ways into a lean set: .wtns-layout scalars, and registration from points already on the device"""
    import torch
    n = (1 << 10) + 3
    pts, _ = _points(orc, 1, n, 31)
    sc = I.circom_like_scalars(n, 32)
    want = orc.msm_naive(1, I.fr_mont_bytes(sc), pts)
    d_pts = torch.frombuffer(bytearray(pts), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    for s in (2, 3):
        h = ctx.register_points(1, d_pts.data_ptr(), n, device=True, table_stride=s)
        try:
            assert ctx.msm_points(h, I.fr_std_bytes(sc), mont=False) == want
            assert ctx.msm_points(h, I.fr_mont_bytes(sc)) == want
        finally:
            h.release()


def test_partials_of_a_lean_and_a_full_set_sum_to_the_whole(ctx, orc):
    """G16_OUT_PARTIAL: the XYZZ partial of a lean set over one half of the points and that of a full set over the other
    half add up, through g16_g1_sum_partials, to the naive MSM over all of them"""
    n = (1 << 10) + 3
    pts, _ = _points(orc, 1, n, 41)
    sc = I.uniform_scalars(n, 42)
    sc[5], sc[n - 1] = R - 1, 0
    sb = I.fr_mont_bytes(sc)
    k = n // 2
    want = orc.msm_naive(1, sb, pts)
    for s in (2, 3, 255):
        lean = ctx.register_points(1, pts[:64 * k], k, table_stride=s)
        full = ctx.register_points(1, pts[64 * k:], n - k)
        try:
            parts = ctx.msm_points(lean, sb[:32 * k], partial=True) + ctx.msm_points(full, sb[32 * k:], partial=True)
            assert len(parts) == 256 and ctx.sum_partials(1, parts, 2) == want, s
        finally:
            lean.release()
            full.release()


def test_registered_state_follows_the_plan(ctx, orc):
    """g16_points_info, g16_points_table_bytes and g16_points_inf_count of lean sets equal g16_points_plan, and the bytes
    follow the formula: bytes(s) <= ceil(nwin / s) / nwin * bytes(1, one table per window)"""
    from nim_groth16_amd import points_plan
    for group, psz in ((1, 64), (2, 128)):
        for n in (37, (1 << 10) + 3):
            pts, n_inf = _points(orc, group, n, 51)
            for s in (2, 3, 4, 5, 16, 255):
                c, ntables, nbytes = points_plan(group, n, s)
                nwin = _nwin(c)
                h = ctx.register_points(group, pts, n, table_stride=s)
                try:
                    assert h.info() == (c, ntables) and h.table_bytes == nbytes == ntables * n * psz
                    assert h.inf_count() == n_inf
                finally:
                    h.release()
                assert ntables == -(-nwin // min(s, nwin))
                # against one table for every window of the same c (an identity of the formula, not a measurement)
                assert nbytes * nwin <= -(-nwin // s) * (nwin * n * psz)
            c1, ntab1, bytes1 = points_plan(group, n, 1)
            assert bytes1 == ntab1 * n * psz and ntab1 in (_nwin(c1), 2 * _nwin(c1))


def _toxic(seed=5):
    from nim_groth16_amd.fake_setup import ToxicWaste
    from nim_groth16_amd.synthetic import SplitMix64
    rng = SplitMix64(seed)
    return ToxicWaste(*[rng.fr() for _ in range(5)]), rng


def _key_nwin(zk):
    from nim_groth16_amd import points_plan
    return _nwin(points_plan(1, zk.header.nvars, 255)[0])


@pytest.mark.parametrize("log2n", [10, 12])
@pytest.mark.parametrize("flavour", [1, 0])
def test_lean_keys_prove_what_the_stride_one_key_and_the_oracle_prove(ctx, orc, tmp_path, flavour, log2n):
    """keys at stride 2, 3 and nwin; the unparsed coefficient section (g16_pkey_create_zkey_lean); a two-shard lean key on
    one device through g16_prove_partials / _combine; the pool at depth 2; a two-member group on device 0"""
    from nim_groth16_amd import DeviceGroup, ProverPool, loadGroupKey, loadProvingKey
    from nim_groth16_amd import bn128 as F
    from nim_groth16_amd.fake_setup import fakeCircuitSetup
    from nim_groth16_amd.files import parseZKey, writeZKey
    from nim_groth16_amd.synthetic import squaringChain
    from tests.parity import check_gpu_proof
    r1cs, wit = squaringChain((1 << log2n) - 2, seed=4)
    tox, rng = _toxic(7)
    zk = fakeCircuitSetup(r1cs, tox, flavour, ctx)
    wb, ws = F.frSeqToMontBytes(wit), F.frSeqToStdBytes(wit)
    r, s = rng.fr(), rng.fr()
    rb, sb = F.frToMontBytes(r), F.frToMontBytes(s)
    pk = loadProvingKey(zk, ctx)
    want, want0 = pk.prove(wb, r=rb, s=sb), pk.prove(wb)
    pk.destroy()
    check_gpu_proof(orc, zk, wit, wb, r, s, want, ctx)
    nwin = _key_nwin(zk)
    for stride in (2, 3, nwin):
        pk = loadProvingKey(zk, ctx, table_stride=stride)
        try:
            assert pk.prove(wb, r=rb, s=sb) == want, stride
            assert pk.prove(ws, mont=False, r=rb, s=sb) == want, stride
            assert pk.prove(wb) == want0, stride
        finally:
            pk.destroy()
    # the .zkey's section 4 as it lies on disk (a .zkey file is read as a snarkjs key: the section is taken from the
    # file and the rest of the key, whose flavour the file does not carry, from memory)
    path = str(tmp_path / "c.zkey")
    writeZKey(path, zk)
    raw = copy.copy(zk)
    raw.coeffs, raw.coeffsSection4 = [], parseZKey(path, rawCoeffs=True).coeffsSection4
    pk = loadProvingKey(raw, ctx, table_stride=3)
    try:
        assert pk.prove(ws, mont=False, r=rb, s=sb) == want
    finally:
        pk.destroy()
    # two shards of a lean key on one device
    keys = [loadProvingKey(zk, ctx, shard_index=k, shard_count=2, table_stride=2) for k in range(2)]
    try:
        recs = b"".join(k.prove_partials(wb) for k in keys)
        assert keys[0].prove_combine(recs, 2, rb, sb) == want and keys[1].prove_combine(recs, 2, rb, sb) == want
    finally:
        for k in keys:
            k.destroy()
    # the pool at depth 2
    pk = loadProvingKey(zk, ctx, table_stride=2)
    pool = ProverPool(pk, depth=2)
    try:
        t1, t2 = pool.submit(wb, r=rb, s=sb), pool.submit(wb)
        t3 = pool.submit(ws, mont=False, r=rb, s=sb)
        assert pool.collect(t2) == want0 and pool.collect(t1) == want and pool.collect(t3) == want
    finally:
        pool.close()
        pk.destroy()
    # a two-member group on device 0
    grp = DeviceGroup([0, 0])
    gk = loadGroupKey(zk, grp, table_stride=3)
    try:
        assert gk.prove(wb, r=rb, s=sb) == want and gk.prove(wb) == want0
    finally:
        gk.destroy()
        grp.close()


def test_lean_poseidon_shaped_key_on_compacted_lists(ctx, orc):
    """a Poseidon-shaped 2^10 key: a third of the B points at infinity, so B1 / B2 run on compacted entry lists"""
    from nim_groth16_amd import loadProvingKey
    from nim_groth16_amd import bn128 as F
    from nim_groth16_amd.fake_setup import fakeCircuitSetup
    from nim_groth16_amd.synthetic import poseidonMerkle
    from tests.parity import check_gpu_proof
    r1cs, wit = poseidonMerkle(10, seed=4)
    tox, rng = _toxic()
    zk = fakeCircuitSetup(r1cs, tox, 1, ctx)
    wb = F.frSeqToMontBytes(wit)
    r, s = rng.fr(), rng.fr()
    rb, sb = F.frToMontBytes(r), F.frToMontBytes(s)
    pk = loadProvingKey(zk, ctx)
    want, inf = pk.prove(wb, r=rb, s=sb), pk.inf_counts()
    pk.destroy()
    assert inf["compact_B"] and inf["B1"] * 4 > zk.header.nvars
    check_gpu_proof(orc, zk, wit, wb, r, s, want, ctx)
    for stride in (2, 3, _key_nwin(zk)):
        pk = loadProvingKey(zk, ctx, table_stride=stride)
        try:
            assert pk.inf_counts() == inf
            assert pk.prove(wb, r=rb, s=sb) == want, stride
        finally:
            pk.destroy()


def test_stride_zero_and_one_through_the_new_entry_points(ctx, orc):
    """g16_points_register_*_lean and g16_pkey_create_lean with a stride of 0 or 1 are the old entry points: the same
    g16_points_info, the same table bytes, the same MSM and proof bytes"""
    from nim_groth16_amd import loadProvingKey
    from nim_groth16_amd import bn128 as F
    from nim_groth16_amd._lib import PkeyDesc, PointSet
    from nim_groth16_amd.fake_setup import fakeCircuitSetup
    from nim_groth16_amd.prover import _cbuf
    from nim_groth16_amd.synthetic import squaringChain
    from nim_groth16_amd.zkey_types import packCoeffs
    lib = ctx._lib
    for group, n in ((1, (1 << 10) + 3), (2, 37), (1, 1 << 16)):
        ks, sc = I.uniform_scalars(n, 61), I.circom_like_scalars(n, 62)
        pts = orc.fixed_base(group, I.fr_mont_bytes(ks))
        old = ctx.register_points(group, pts, n)
        res = ctx.msm_points(old, I.fr_mont_bytes(sc))
        assert res == orc.msm(group, I.fr_mont_bytes(sc), pts)
        for stride in (0, 1):
            h = ctypes.c_void_p()
            fn = lib.g16_points_register_g1_lean if group == 1 else lib.g16_points_register_g2_lean
            ctx._check(fn(ctx._h, pts, n, stride, ctypes.byref(h)))
            new = PointSet(ctx, h, group, n)
            try:
                assert new.info() == old.info() and new.table_bytes == old.table_bytes
                assert ctx.msm_points(new, I.fr_mont_bytes(sc)) == res
            finally:
                new.release()
        old.release()
    r1cs, wit = squaringChain((1 << 10) - 2, seed=4)
    tox, rng = _toxic(9)
    zk = fakeCircuitSetup(r1cs, tox, 1, ctx)
    wb = F.frSeqToMontBytes(wit)
    rb, sb = F.frToMontBytes(rng.fr()), F.frToMontBytes(rng.fr())
    pk = loadProvingKey(zk, ctx)
    want = pk.prove(wb, r=rb, s=sb)
    pk.destroy()
    hdr, p, spec = zk.header, zk.pPoints, zk.specPoints
    bufs = [_cbuf(x) for x in (p.pointsA1, p.pointsB1, p.pointsB2, p.pointsC1, p.pointsH1, packCoeffs(zk.coeffs),
                               spec.alpha1, spec.beta1, spec.delta1, spec.beta2, spec.delta2)]
    a = [ctypes.cast(b, ctypes.c_void_p) for b in bufs]
    desc = PkeyDesc(hdr.nvars, hdr.npubs, hdr.logDomainSize, hdr.flavour, a[0], a[1], a[2], a[3], a[4], a[5],
                    len(zk.coeffs), a[6], a[7], a[8], a[9], a[10], 0, 1)
    for stride in (0, 1):
        k = ctypes.c_void_p()
        ctx._check(lib.g16_pkey_create_lean(ctx._h, ctypes.byref(desc), stride, ctypes.byref(k)))
        try:
            out = ctypes.create_string_buffer(256)
            ctx._check(lib.g16_prove(ctx._h, k, wb, 1, rb, sb, out))
            assert (out.raw[:64], out.raw[64:192], out.raw[192:]) == want, stride
        finally:
            lib.g16_pkey_destroy(k)
