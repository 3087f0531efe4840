"""The scalar side of the fake setup on the CPU: g++ builds nim_groth16_amd/csrc/setup.cuh (the code the device runs) and
the per-run function of the geometric / Lagrange kernel and the combination of a wire are held to the oracle's
eval_lagrange_poly_at (math/poly.nim:242-250) and to plain integers; g16_setup_log2_domain to ceiling_log2; and the
.r1cs reader of the native tools runs over good and damaged files in a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer."""
import ctypes
import glob
import os
import struct
import subprocess

import pytest

from oracle import bn254_ref as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "cpu_kernels")
CSRC = os.path.join(ROOT, "nim_groth16_amd", "csrc")
R = o.R
PATTERN = bytes(range(1, 33))        # what an untouched output slot holds


@pytest.fixture(scope="module")
def shim():
    so, src = os.path.join(HERE, "libsetup_shim.so"), os.path.join(HERE, "setup_shim.cpp")
    deps = [src] + glob.glob(os.path.join(CSRC, "*.cuh")) + glob.glob(os.path.join(CSRC, "*.inc"))
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", src, "-o", so])
    lib = ctypes.CDLL(so)
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    lib.shim_log2_domain.restype = lib.shim_geom_run.restype = u32
    lib.shim_log2_domain.argtypes = [u32, u32]
    lib.shim_omega.restype = lib.shim_pow.restype = lib.shim_combine.restype = None
    lib.shim_omega.argtypes = [u32, vp]
    lib.shim_pow.argtypes = [vp, u32, vp]
    lib.shim_geom_run.argtypes = [ctypes.c_int, vp, vp, vp, vp, u32, vp]
    lib.shim_combine.argtypes = [vp, u32, u32, vp]
    return lib


def mont(x):
    return o.fr_to_mont_bytes(x % R)


def unmont(b):
    return o.fr_from_mont_bytes(bytes(b))


def run(shim, lagrange, x0, s, c, tau, length):
    """-> (position of the first zero denominator or M, the `length` results as ints); checks that nothing at or beyond
    `length` was written"""
    M = shim.shim_run_length()
    out = ctypes.create_string_buffer(PATTERN * (M + 1), 32 * (M + 1))
    z = shim.shim_geom_run(int(lagrange), mont(x0), mont(s), mont(c), mont(tau), length, out)
    raw = out.raw
    for k in range(length, M + 1):
        assert raw[32 * k:32 * k + 32] == PATTERN, f"slot {k} written by a run of {length}"
    return z, [unmont(raw[32 * k:32 * k + 32]) for k in range(length)]


def test_run_length_is_what_the_gpu_tests_assume(shim):
    assert shim.shim_run_length() == 8 and shim.shim_block_size() == 256


def test_omega_and_pow(shim):
    out = ctypes.create_string_buffer(32)
    for k in (0, 1, 2, 5, 13, 27, 28):
        shim.shim_omega(k, out)
        assert unmont(out.raw) == pow(o.GEN28, 1 << (28 - k), R)
    rng = o.SplitMix64(3)
    b = rng.fr()
    for e in (0, 1, 2, 3, 255, 256, (1 << 29) - 1, (1 << 32) - 1):
        shim.shim_pow(mont(b), e, out)
        assert unmont(out.raw) == pow(b, e, R)
    shim.shim_pow(mont(0), 0, out)
    assert unmont(out.raw) == 1


def test_log2_domain_is_ceiling_log2(shim):
    for n, p in [(0, 0), (1, 0), (0, 1), (1, 1), (2, 1), (3, 4), (5, 2), (6, 1), (7, 0), (1 << 20, 1), ((1 << 20) - 2, 1),
                 ((1 << 20) - 1, 1), (1 << 27, 0), ((1 << 27) - 1, 0), (0xffffffff, 0xffffffff)]:
        assert shim.shim_log2_domain(n, p) == o.ceiling_log2(n + p + 1), (n, p)


def test_library_log2_domain_needs_no_device():
    """g16_setup_log2_domain is a pure function of the C ABI: called here with no context"""
    from nim_groth16_amd._lib import SetupDesc, load_library
    lib = load_library()
    for n, p in [(3, 2), (13, 2), (14, 2), (1022, 1), (1023, 1), (0, 0)]:
        d, out = SetupDesc(), ctypes.c_uint32(99)
        d.nconstraints, d.npubs = n, p
        assert lib.g16_setup_log2_domain(ctypes.byref(d), ctypes.byref(out)) == 0
        assert out.value == o.ceiling_log2(n + p + 1)
    assert lib.g16_setup_log2_domain(None, ctypes.byref(out)) == -1


@pytest.mark.parametrize("log2n", [3, 4, 6])
def test_lagrange_runs_against_the_oracle(shim, log2n):
    """runs of every length 1..M at every offset of a small domain, with a scale: c * x / (tau - x) summed into
    L_j(tau) = eval_lagrange_poly_at, on the domain itself and on the odd indices of the doubled domain"""
    M = shim.shim_run_length()
    rng = o.SplitMix64(100 + log2n)
    tau, scale = rng.fr(), rng.fr()
    n = 1 << log2n
    D = o.Domain(n)
    w = D.domainGen
    want = [scale * o.eval_lagrange_poly_at(D, j, tau) % R for j in range(n)]
    c = scale * (pow(tau, n, R) - 1) * pow(n, -1, R) % R
    for length in range(1, M + 1):
        for first in sorted({0, min(1, n - length), n - length, (n - length) // 2}):
            z, got = run(shim, True, pow(w, first, R), w, c, tau, length)
            assert z == M and got == want[first:first + length], (length, first)
    # odd indices of the doubled domain: w0 = omega_2n^(2 i0 + 1), s = omega_2n^2
    D2 = o.Domain(2 * n)
    w2 = D2.domainGen
    c2 = scale * (pow(tau, 2 * n, R) - 1) * pow(2 * n, -1, R) % R
    for length in range(1, M + 1):
        i0 = (n - length) // 3
        z, got = run(shim, True, pow(w2, 2 * i0 + 1, R), w2 * w2 % R, c2, tau, length)
        assert z == M
        assert got == [scale * o.eval_lagrange_poly_at(D2, 2 * (i0 + k) + 1, tau) % R for k in range(length)]


def test_powers_runs_against_pow(shim):
    M = shim.shim_run_length()
    rng = o.SplitMix64(7)
    for base in (rng.fr(), 0, 1, R - 1):
        c, x0 = rng.fr(), rng.fr()
        for length in range(1, M + 1):
            z, got = run(shim, False, x0, base, c, 0, length)
            assert z == M and got == [c * x0 * pow(base, k, R) % R for k in range(length)]


def test_zero_denominators_inside_a_run(shim):
    """tau = x_k for one k and for two k of a run (a sequence that repeats): that factor counts as one, the element is 0,
    the first such k is reported, every other element keeps its value; a zero beyond the run's length is not seen"""
    M = shim.shim_run_length()
    rng = o.SplitMix64(11)
    c = rng.fr()
    n = 16
    w = o.Domain(n).domainGen
    for k in range(M):                                        # one zero, at every position
        tau = pow(w, k + 3, R)
        z, got = run(shim, True, pow(w, 3, R), w, c, tau, M)
        assert z == k
        for i in range(M):
            x = pow(w, 3 + i, R)
            assert got[i] == (0 if i == k else c * x * pow(tau - x, -1, R) % R)
        if k >= 1:                                            # ... and cut off before it
            z, got = run(shim, True, pow(w, 3, R), w, c, tau, k)
            assert z == M and got == [c * pow(w, 3 + i, R) * pow(tau - pow(w, 3 + i, R), -1, R) % R for i in range(k)]
    w4 = o.Domain(4).domainGen                                # two zeros: x_k has period 4, so x_1 = x_5 = tau
    tau = w4
    z, got = run(shim, True, 1, w4, c, tau, M)
    assert z == 1
    for i in range(M):
        x = pow(w4, i, R)
        assert got[i] == (0 if i % 4 == 1 else c * x * pow(tau - x, -1, R) % R)
    z, got = run(shim, True, 1, w4, c, tau, 5)                # the second zero lies beyond a run of 5
    assert z == 1 and got[1] == 0 and got[4] == c * pow(tau - 1, -1, R) % R


def test_tau_zero_and_tau_elsewhere_in_the_domain(shim):
    M = shim.shim_run_length()
    n = 32
    D = o.Domain(n)
    w = D.domainGen
    inv_n = pow(n, -1, R)
    for first in (0, 5, n - M):                               # tau = 0: every L_j = 1/n
        z, got = run(shim, True, pow(w, first, R), w, (0 - 1) * inv_n % R, 0, M)
        assert z == M and got == [inv_n] * M
        assert got == [o.eval_lagrange_poly_at(D, first + k, 0) for k in range(M)]
    # tau^n = 1 but tau is not among the requested indices: c = (tau^n - 1)/n = 0 and every value is zero
    tau = pow(w, 20, R)
    c = (pow(tau, n, R) - 1) * inv_n % R
    assert c == 0
    z, got = run(shim, True, pow(w, 4, R), w, c, tau, M)      # indices 4..11
    assert z == M and got == [0] * M
    # ... the same on the doubled domain: tau at an even index, odd indices requested
    w2 = o.Domain(2 * n).domainGen
    tau = pow(w2, 6, R)
    z, got = run(shim, True, w2, w2 * w2 % R, 0, tau, M)
    assert z == M and got == [0] * M


def test_combination_against_integers(shim):
    rng = o.SplitMix64(21)
    out = ctypes.create_string_buffer(32)
    for trial in range(8):
        a, b, c, alpha, beta, gamma, delta = ((0 if trial == 0 else R - 1 if trial == 1 else rng.fr()) for _ in range(7))
        if trial < 2:
            gamma, delta = rng.fr(), rng.fr()
        gi, di = pow(gamma, -1, R), pow(delta, -1, R)
        for npubs in (0, 1, 3):
            for j in (0, npubs, npubs + 1, npubs + 7):
                shim.shim_combine(b"".join(mont(x) for x in (a, b, c, alpha, beta, gi, di)), j, npubs, out)
                want = (beta * a + alpha * b + c) * (gi if j <= npubs else di) % R
                assert unmont(out.raw) == want, (trial, npubs, j)


# ---- the .r1cs reader of tools/g16_files.hpp under sanitizers -----------------------------------------------------------
def _sections(blob):
    """[(id, offset of the length field, offset of the payload, length)] of a container file"""
    (nsec,) = struct.unpack_from("<I", blob, 8)
    pos, out = 12, []
    for _ in range(nsec):
        sid, ln = struct.unpack_from("<IQ", blob, pos)
        out.append((sid, pos + 4, pos + 12, ln))
        pos += 12 + ln
    return out


def test_r1cs_reader_under_sanitizers(tmp_path):
    from nim_groth16_amd.fake_setup import R1CS
    from nim_groth16_amd.files.r1cs import parseR1CS, writeR1CS
    exe = str(tmp_path / "r1cs_reader_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(HERE, "r1cs_reader_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="exitcode=86", UBSAN_OPTIONS="exitcode=86")

    def reader(path):
        return subprocess.run([exe, path], capture_output=True, text=True, timeout=120, env=env)

    def rejected(name, blob, why):
        path = str(tmp_path / name)
        open(path, "wb").write(blob)
        r = reader(path)
        assert r.returncode == 1 and why in r.stderr and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, \
            (name, r.returncode, r.stdout[-500:], r.stderr[-3000:])

    rng = o.SplitMix64(5)
    cons = list(o.toy_r1cs().constraints)
    cons.append(([(1, rng.fr()), (1, 2), (7, R - 1)], [], [(0, rng.fr())]))      # a repeated wire, an empty B
    good = str(tmp_path / "good.r1cs")
    writeR1CS(good, R1CS(8, 1, 1, 3, cons))
    r = reader(good)
    assert r.returncode == 0, (r.stdout, r.stderr[-3000:])
    nnz = [sum(len(c[k]) for c in cons) for k in range(3)]
    assert f"r1cs ok: wires 8 pubout 1 pubin 1 privin 3 constraints {len(cons)} nnz {nnz[0]} {nnz[1]} {nnz[2]} " in r.stdout
    assert parseR1CS(good).constraints == [tuple([(w, v % R) for (w, v) in lc] for lc in c) for c in cons]
    blob = open(good, "rb").read()
    secs = {sid: (lo, po, ln) for (sid, lo, po, ln) in _sections(blob)}
    h, s2 = secs[1][1], secs[2]

    def patched(off, fmt, value):
        b = bytearray(blob)
        struct.pack_into(fmt, b, off, value)
        return bytes(b)

    # truncated: in the container header, inside the header section, inside a term, after the last constraint
    for cut in (8, 20, h + 40, s2[1] + 4 + 17, s2[1] + s2[2] - 1, len(blob) - 1):
        rejected(f"cut{cut}.r1cs", blob[:cut], "")
    # oversized counts: constraints, terms of the first linear combination, a section length beyond the file
    rejected("ncons.r1cs", patched(h + 36 + 24, "<I", 0xffffffff), "constraint count exceeds")
    rejected("ncons1.r1cs", patched(h + 36 + 24, "<I", len(cons) + 1), "")
    rejected("nterms.r1cs", patched(s2[1] + 12 * 0 + 8 + 0, "<I", 0x7fffffff), "")
    first_terms = s2[1]                                      # constraint 0 has an empty A: its term count is 0 here
    rejected("nterms0.r1cs", patched(first_terms, "<I", 0xffffffff), "term count exceeds")
    rejected("seclen.r1cs", patched(s2[0], "<Q", 1 << 63), "truncated section")
    rejected("wire.r1cs", patched(s2[1] + 4 + 4 + 4, "<I", 8), "wire index out of range")
    # wrong sections: another file type, no constraint section, a header of the wrong length, a short label section
    rejected("magic.r1cs", b"zkey" + blob[4:], "not a `r1cs` file")
    rejected("nosec2.r1cs", patched(s2[0] - 4, "<I", 7), "missing section 2")
    rejected("hdrlen.r1cs", patched(secs[1][0], "<Q", 60), "")
    rejected("prime.r1cs", patched(h + 4, "<B", 2), "alt-bn128")
    rejected("labels.r1cs", patched(secs[3][0], "<Q", 8 * 8 - 8)[:-8], "unexpected label section length")
    rejected("fewer_cons.r1cs", patched(h + 36 + 24, "<I", len(cons) - 1), "unexpected constraint section length")
