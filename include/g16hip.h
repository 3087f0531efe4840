/*
 * g16hip -- C ABI of the MI355X-native MSM / NTT hot path of a Groth16 (BN254) prover.
 *
 * Drop-in boundary for codex-storage/nim-groth16 (reference paths relative to /root/reference):
 * every entry point names the reference proc it replaces.  The reference has no FFI layer of its
 * own (it is pure Nim calling constantine); INTEGRATION.md shows the `importc` shims that give
 * these functions the reference's Nim signatures.
 *
 * Data layouts (identical to the reference's in-memory types):
 *   Fr, Fp   : 32 bytes, 4 x u64 little-endian limbs, Montgomery form R = 2^256, canonical (< modulus)
 *              (groth16/bn128/fields.nim:23-25, io.nim:60-92)
 *   Fp2      : 64 bytes  = { c0, c1 }                       (fields.nim:27-32)
 *   G1 affine: 64 bytes  = { x, y : Fp  }, infinity = (0,0)  (curves.nim:33,49)
 *   G2 affine: 128 bytes = { x, y : Fp2 }, infinity = (0,0)  (curves.nim:34,50)
 *   "std" scalars: 32 bytes canonical little-endian, NOT Montgomery (the .wtns layout,
 *              files/witness.nim:14,57-60)
 *
 * Error convention: every function returns 0 on success or a negative G16_E* code; nothing
 * throws or aborts across the boundary (the reference uses `assert`, msm.nim:97, ntt.nim:56-57).
 * A g16_ctx is used by one host thread at a time (any thread: every call makes the context's device the calling
 * thread's current HIP device); distinct contexts are independent.
 * Registered point sets, proving keys and verification keys (g16_points / g16_pkey / g16_vkey) are immutable and
 * belong to the DEVICE of the context that created them: any context of that device may use them, concurrently
 * (the in-flight proofs of one GPU share one resident key), and they may be released before or after any context.
 * Inputs are read-only and not retained after return, except explicitly registered point sets.
 * G16_* environment knobs are read once per process, at the first g16_ctx_create.
 * There is NO CPU fallback: without a usable HIP device every call fails with G16_ENODEV.
 */
#ifndef G16HIP_H
#define G16HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define G16_OK 0
#define G16_EINVAL (-1)  /* bad argument (null pointer, size mismatch, log2n out of range ...) */
#define G16_ENODEV (-2)  /* no HIP device / device init failed */
#define G16_EHIP (-3)    /* a HIP runtime call or kernel failed; see g16_last_error */
#define G16_ENOMEM (-4)  /* device or host allocation failed */
#define G16_ESELFTEST (-5)
/* G16_EBUSY (-6): see the prover pool below */

typedef struct g16_ctx g16_ctx;
typedef struct g16_points g16_points; /* device-resident point set (ProverPoints member, zkey_types.nim:36-41) */

/* flags for the scalar argument of the MSM calls */
#define G16_SCALARS_MONT 1u /* Nim seq[Fr] limbs (Montgomery) -- what msm.nim:42-44 `toBig` consumes   */
#define G16_SCALARS_STD 0u  /* canonical little-endian (raw .wtns values)                              */
#define G16_SCALARS_DEVICE 2u /* g16_msm_points only: the scalar pointer is a device (HBM) pointer       */
#define G16_OUT_PARTIAL 4u    /* g16_msm_points only: write the 128/256-byte XYZZ partial, not the affine */
#define G16_OUT_DEVICE 8u     /* g16_prove_partials only: the output pointer is a device pointer           */
#define G16_NO_HOST_SYNC 32u  /* g16_prove_partials_begin/_end: do not block the host (see there)             */

/* ---- context ------------------------------------------------------------------------------------ */
int32_t g16_ctx_create(int32_t device, g16_ctx** out);
void g16_ctx_destroy(g16_ctx* ctx);
const char* g16_last_error(const g16_ctx* ctx);
/* run all work of this context on an existing HIP stream (e.g. torch's current stream); NULL = own stream */
int32_t g16_ctx_set_stream(g16_ctx* ctx, void* hip_stream);
int32_t g16_ctx_synchronize(g16_ctx* ctx);
/* waits for EVERYTHING the context has queued (its main stream and its MSM lanes) and forgets a pending
 * g16_prove_partials_begin (a later _end returns G16_EINVAL): what a caller does when its exchange between _begin and
 * _end failed, before it reuses or frees the buffers it handed in */
int32_t g16_ctx_cancel(g16_ctx* ctx);
/* layout / constant / arithmetic self-check on the device (sizeof, Montgomery one == frMontR io.nim:91,
 * gen1 on curve, small known-answer MSM and NTT).  The Nim shim calls it once at start-up. */
int32_t g16_selftest(g16_ctx* ctx);

/* ---- MSM: replaces msmMultiThreadedG1/G2 (groth16/bn128/msm.nim:89-158) and msmG1/msmG2 (:202-203),
 *      i.e. constantine's multiScalarMul_vartime + prj.affine (msm.nim:49-54, 76-81) ----------------- */
/* host pointers in, affine point out (64 / 128 bytes, host).  n == 0 -> infinity (0,0). */
int32_t g16_msm_g1(g16_ctx* ctx, const void* scalars, uint32_t scalar_flags, const void* points, size_t n,
                   void* out_affine);
int32_t g16_msm_g2(g16_ctx* ctx, const void* scalars, uint32_t scalar_flags, const void* points, size_t n,
                   void* out_affine);
/* same with scalars and points already resident in device memory (HBM); result to host memory */
int32_t g16_msm_g1_dev(g16_ctx* ctx, const void* d_scalars, uint32_t scalar_flags, const void* d_points, size_t n,
                       void* out_affine);
int32_t g16_msm_g2_dev(g16_ctx* ctx, const void* d_scalars, uint32_t scalar_flags, const void* d_points, size_t n,
                       void* out_affine);
/* partial result for multi-GPU sharding (msm.nim:105-119 chunks): 128 / 256 byte XYZZ accumulator
 * (X, Y, ZZ, ZZZ), Montgomery; combine with g16_g1_sum_partials / g16_g2_sum_partials. */
int32_t g16_msm_g1_partial_dev(g16_ctx* ctx, const void* d_scalars, uint32_t scalar_flags, const void* d_points,
                               size_t n, void* out_xyzz);
int32_t g16_msm_g2_partial_dev(g16_ctx* ctx, const void* d_scalars, uint32_t scalar_flags, const void* d_points,
                               size_t n, void* out_xyzz);
/* res = sum of `count` XYZZ partials (host memory, e.g. gathered over RCCL) -> affine; replaces the
 * `res += sync pending[k]` loop (msm.nim:117-119, 151-153) */
int32_t g16_g1_sum_partials(g16_ctx* ctx, const void* xyzz, size_t count, void* out_affine);
int32_t g16_g2_sum_partials(g16_ctx* ctx, const void* xyzz, size_t count, void* out_affine);

/* ---- registered point sets -------------------------------------------------------------------------
 * The five ProverPoints arrays (pointsA1/B1/B2/C1/H1, groth16/zkey_types.nim:36-41) are constant per
 * circuit and are loaded once (files/zkey.nim:201-224).  Registering a set copies it to HBM and
 * precomputes the window tables 2^(c w) * P_i, so that no MSM against it contains a doubling chain.
 * Because the factor lives in the table, all windows share one bucket set and the window size c is chosen
 * by a cost model (c = 20 for 2^20 points: 13 tables, 832 MiB per 2^20 G1 points, 1.6 GiB for G2). */
int32_t g16_points_register_g1(g16_ctx* ctx, const void* points, size_t n, g16_points** out);
int32_t g16_points_register_g2(g16_ctx* ctx, const void* points, size_t n, g16_points** out);
int32_t g16_points_register_g1_dev(g16_ctx* ctx, const void* d_points, size_t n, g16_points** out);
int32_t g16_points_register_g2_dev(g16_ctx* ctx, const void* d_points, size_t n, g16_points** out);
void g16_points_release(g16_points* pts);
size_t g16_points_count(const g16_points* pts);
/* points at infinity (0,0) in the set (legal inputs: curves.nim:95-107; snarkjs keys hold one for every wire absent
 * from a matrix).  A set with at least G16_INF_COMPACT percent of them (environment, default 10) gets bucket entry
 * lists that leave them out, instead of paying a loop trip per (0,0) entry. */
size_t g16_points_inf_count(const g16_points* pts);
/* window size c and number of tables chosen for this set: W = 254 / c + 1 windows x 1 or 2 multiplier tables
 * ([m][w][i] = 2^(c w + m) P_i).  An MSM against it performs count * W bucket additions + 2 reduction additions per
 * bucket: 2^(c-1) buckets with one table per window, 0.67 * 2^(c-1) with two (the class bucket set, msm.cuh) */
int32_t g16_points_info(const g16_points* pts, uint32_t* window_bits, uint32_t* ntables);

/* ---- lean point sets: window tables at a stride ------------------------------------------------------
 * The calls above store a table for EVERY window (two with the class bucket set): about 10 GB of HBM per 2^20
 * constraints of a proving key.  A set registered at table_stride s >= 2 stores a table for every s-th window only --
 * table j holds 2^(c s j) P_i -- and window w = s j + r gathers from table j into bucket set r:
 *     sum_w 2^(c w) D_w  =  sum_{r < s} 2^(c r) * ( sum_j 2^(c s j) D_{s j + r} ).
 * The trade, in the terms of the cost model that picks c (W = 254 / c + 1 windows):
 *     bucket additions     count * W, as before
 *     reduction additions  2 * s * 2^(c-1): s bucket sets of 2^(c-1) buckets instead of one (c <= 16, as for a
 *                          one-shot MSM), then a Horner fold of s sums with c doublings each
 *     tables               ceil(W / s) instead of W: the bytes shrink by about s
 * s above W is W: one table, the layout of a one-shot MSM with the points resident.  A lean set has one table per stored
 * window (never the class bucket set).  table_stride 0 or 1 is exactly g16_points_register_*: same tables, same
 * launches, same results.  Everything that takes a g16_points takes a lean one; results are the same canonical bytes. */
int32_t g16_points_register_g1_lean(g16_ctx* ctx, const void* points, size_t n, uint32_t table_stride, g16_points** out);
int32_t g16_points_register_g2_lean(g16_ctx* ctx, const void* points, size_t n, uint32_t table_stride, g16_points** out);
int32_t g16_points_register_g1_lean_dev(g16_ctx* ctx, const void* d_points, size_t n, uint32_t table_stride,
                                        g16_points** out);
int32_t g16_points_register_g2_lean_dev(g16_ctx* ctx, const void* d_points, size_t n, uint32_t table_stride,
                                        g16_points** out);
/* HBM held by the set's tables: ntables * count * 64 bytes (G1) or * 128 (G2), ntables as g16_points_info reports it
 * (ceil(W / s) for a lean set) */
int32_t g16_points_table_bytes(const g16_points* pts, size_t* bytes);
/* What registering n points of group 1 (G1) or 2 (G2) at table_stride would choose: window bits, tables, and the bytes
 * of HBM they take.  A pure function -- no device, no context: what a caller with a memory budget calls before
 * registering.  (With two tables per window, a set that finds no room in HBM falls back to one; g16_points_table_bytes
 * reports what a registered set holds.)  Any out pointer may be NULL. */
int32_t g16_points_plan(int group, size_t n, uint32_t table_stride, uint32_t* window_bits, uint32_t* ntables,
                        size_t* bytes);
/* sum_i scalars[i] * P_i over the whole registered set (scalars: g16_points_count elements);
 * flags = G16_SCALARS_MONT/STD | G16_SCALARS_DEVICE | G16_OUT_PARTIAL.  This is the call a prover makes
 * per proof for msmMultiThreadedG1/G2 (groth16/prover.nim:282,288,294,301,302). */
int32_t g16_msm_points(g16_ctx* ctx, const g16_points* pts, const void* scalars, uint32_t flags, void* out);

/* ---- curve membership of a point array: replaces the per-point asserts of mkG1 / mkG2 that the reference runs
 * while loading a .zkey (groth16/bn128/curves.nim:95-107 via io.nim:240-250).  *first_bad = index of the first
 * point that is neither (0,0) nor on y^2 = x^3 + b, or (size_t)-1 when all are fine.  Like the reference this is
 * NOT a subgroup check.  Host pointers. */
int32_t g16_points_check_g1(g16_ctx* ctx, const void* points, size_t n, size_t* first_bad);
int32_t g16_points_check_g2(g16_ctx* ctx, const void* points, size_t n, size_t* first_bad);

/* ---- fixed-base multiples of the generators: out[i] = scalars[i] * gen1 (resp. gen2) --------------------
 * replaces the `y ** gen1` / `y ** gen2` comprehensions of the fake trusted setup
 * (groth16/fake_setup.nim:258-261, 273-277, 290-302; generators: curves.nim:112-124).  Used to build
 * proving keys for the synthetic benchmark circuits on the GPU box.  Host pointers. */
int32_t g16_fixed_base_g1(g16_ctx* ctx, const void* scalars, uint32_t scalar_flags, size_t n, void* out_points);
int32_t g16_fixed_base_g2(g16_ctx* ctx, const void* scalars, uint32_t scalar_flags, size_t n, void* out_points);

/* ---- fake trusted setup: replaces fakeCircuitSetup (groth16/fake_setup.nim:201-326; `-u/--setup -r circuit.r1cs`,
 *      cli/cli_main.nim:184-193) ----------------------------------------------------------------------------------
 * One call from an R1CS and explicit toxic waste to every point of a ZKey.  The scalar side -- the Lagrange values at
 * tau (math/poly.nim:242-250), the sparse column sums (fake_setup.nim:159-187, 254-256), the combinations
 * beta*A + alpha*B + C over gamma / delta (:273-280) and the H scalars of the flavour (:290-304) -- is formed on the
 * device and stays in HBM between the stages; the points come from the fixed-base kernel of g16_fixed_base_g1/g2.
 * Field arithmetic is exact: the points are the bytes the reference computes.
 * ZKey.coeffs is a rearrangement of the input and stays with the caller (r1csToCoeffs, fake_setup.nim:46-65). */
typedef struct {
  uint32_t nvars, npubs, nconstraints; /* R1CS (files/r1cs.nim:62-80): nWires, nPubOut + nPubIn, constraints.len */
  uint32_t flavour;                    /* G16_FLAVOUR_* (below) */
  /* the R1CS as it is, as triplets; matrix k = 0, 1, 2 = A, B, C: entry i of matrix k is (constraint row[k][i], wire
   * col[k][i], value = 32 bytes at val[k] + 32 i); entries of one (constraint, wire) add up.  The library adds snarkjs's
   * dummy A entries (nconstraints + i, wire i, 1) for i <= npubs itself (fake_setup.nim:59-63, 182-185). */
  const uint32_t* row[3];
  const uint32_t* col[3];
  const void* val[3];
  size_t nnz[3];
  uint32_t flags;                                 /* G16_SCALARS_MONT or G16_SCALARS_STD: the values AND the toxic waste */
  const void *alpha, *beta, *gamma, *delta, *tau; /* ToxicWaste (fake_setup.nim:23-29), 32 bytes each */
} g16_setup_desc;
typedef struct {                                   /* host buffers the caller owns; sizes as in g16_pkey_desc */
  void *alpha1, *beta1, *delta1;                   /* SpecPoints G1 (zkey_types.nim:24-31), 64 B each */
  void *beta2, *gamma2, *delta2;                   /* SpecPoints G2, 128 B each */
  void* pointsIC;                                  /* npubs + 1 G1 points           (VKey, zkey_types.nim:62-73) */
  void *pointsA1, *pointsB1;                       /* nvars G1 points each          (zkey_types.nim:37-38) */
  void* pointsB2;                                  /* nvars G2 points               (:39) */
  void* pointsC1;                                  /* nvars - npubs - 1 G1 points   (:40) */
  void* pointsH1;                                  /* 2^log2_domain G1 points       (:41) */
} g16_setup_points;
/* logDomainSize of the key g16_fake_setup builds: ceilingLog2(nconstraints + npubs + 1) (fake_setup.nim:203-206).
 * A pure function -- no device, no context; only the three counts of desc are read. */
int32_t g16_setup_log2_domain(const g16_setup_desc* desc, uint32_t* log2_domain);
/* The whole setup on the context's stream, one wait at the end.  G16_EINVAL, checked on the host before anything is
 * queued: a null pointer, a matrix entry out of range, a value or toxic scalar that is not canonical (>= r), gamma or
 * delta zero, nvars <= npubs, a domain (doubled for the snarkjs flavour) above 2^28.  tau inside the domain that is
 * evaluated -- the reference's assert "point should be outside the domain" (poly.nim:245) -- is found by the kernel and
 * reported after the run: G16_EINVAL, g16_last_error names the index.  No output is promised after an error. */
int32_t g16_fake_setup(g16_ctx* ctx, const g16_setup_desc* desc, g16_setup_points* out);
/* The two scalar building blocks on their own; host pointers, Montgomery in and out; scale NULL = one.
 * g16_lagrange_fr: out[i] = scale * L_{first + step i}(tau), i < count, on the 2^log2n domain: replaces
 *   evalLagrangePolyAt (math/poly.nim:242-250) over a range of indices -- first 0, step 1 for fake_setup.nim:254-256,
 *   first 1, step 2 on the doubled domain for :301-304.  log2n <= 28; first + step (count - 1) < 2^log2n.
 *   tau = omega^j for a requested j: G16_EINVAL naming j.  tau elsewhere in the domain is legal: every value is zero.
 * g16_powers_fr: out[i] = scale * base^i, i < count <= 2^29: replaces the running product of fake_setup.nim:290-294. */
int32_t g16_lagrange_fr(g16_ctx* ctx, uint32_t log2n, uint32_t first, uint32_t step, size_t count, const void* tau,
                        const void* scale, void* out);
int32_t g16_powers_fr(g16_ctx* ctx, const void* base, const void* scale, size_t count, void* out);

/* ---- circuit setup: the key of `snarkjs zkey new circuit.r1cs pot.ptau` -- a proving key from an R1CS and the powers of
 *      tau of a ceremony, with no toxic waste -------------------------------------------------------------------------
 * g16_r1cs_desc / g16_ptau_desc: declared with the circuit audit, below. */
typedef struct g16_r1cs_desc_s g16_r1cs_desc;
typedef struct g16_ptau_desc_s g16_ptau_desc;
/* out[k] = sum_{j<n} (omega^(-jk) / n) * points[j], n = 2^log2n: the inverse NTT of g16_ntt_fr with curve points for
 * elements -- the Lagrange form of a run of powers of tau.  Host pointers, affine Montgomery in and out, (0,0) legal
 * anywhere; log2n <= 24.  Any points of the group, not only powers. */
int32_t g16_points_intt_g1(g16_ctx* ctx, const void* points, uint32_t log2n, void* out);
int32_t g16_points_intt_g2(g16_ctx* ctx, const void* points, uint32_t log2n, void* out);
/* The whole key; r1cs / ptau exactly the structs of g16_circuit_audit, out the struct of g16_fake_setup;
 * delta: NULL (= 1) or 32 bytes, canonical, non-zero, in the form r1cs->flags names.
 * Write n = 2^log2_domain, log2_domain = ceilingLog2(nconstraints + npubs + 1) as for g16_fake_setup, L_k for the Lagrange
 * polynomials of the n-point domain, and let A include snarkjs's dummy entries (nconstraints + i, wire i, 1), i <= npubs:
 *   LG1[k] = L_k(tau) gen1 = the inverse NTT (g16_points_intt_g1) of tauG1[0 .. n); LG2, LaG1, LbG1 the same of tauG2,
 *            alphaTauG1, betaTauG1
 *   pointsA1[w] = sum over the entries (row, w, v) of A of v LG1[row]; pointsB1 with B; pointsB2 with B over LG2
 *   comb[w]     = sum_A v LbG1[row] + sum_B v LaG1[row] + sum_C v LG1[row];  pointsIC = comb[0 .. npubs],
 *                 pointsC1[w - npubs - 1] = delta^-1 comb[w] for the private wires
 *   pointsH1[i] = delta^-1 L'_(2i+1)(tau) gen1 on the doubled domain (snarkjs flavour: the size-n transform of
 *                 (tauG1[j] - tauG1[j+n]) eta^-j / 2, eta = omega_2n), or delta^-1 (tauG1[i+n] - tauG1[i]) (JensGroth)
 *   alpha1 = alphaTauG1[0], beta1 = betaTauG1[0], beta2 = betaG2, gamma2 = gen2, delta1 = delta gen1, delta2 = delta gen2
 * By construction this is g16_fake_setup's key for the toxic waste (alpha, beta, gamma = 1, delta, tau) when the ptau is
 * the powers of that tau, byte for byte, and it passes g16_circuit_audit against the same r1cs and ptau.
 * SOUNDNESS: gamma = 1 always, and with delta == NULL delta = 1 as well -- exactly the key of `snarkjs zkey new`.  Such a
 * key is NOT fit for production: anyone can forge proofs for it.  It becomes sound only after a phase-2 contribution
 * (`snarkjs zkey contribute`: delta replaced by a secret, pointsC1 / pointsH1 rescaled): g16_key_contribute, below, and
 * g16_contributions_verify for whoever receives the key.  A caller-supplied delta is that step for a caller who may know
 * delta; it is toxic waste of the caller's.
 * Not part of this call: the contribution transcript of a .zkey (section 10 and its hashes) -- the contribution calls
 * below make and check its records, the hashes stay with the caller; the pre-computed Lagrange sections
 * 12-15 of a "prepared" .ptau are out of scope -- the call always works from the monomial sections 2-6.
 * Before any arithmetic the element passes of g16_circuit_audit run over the ptau elements the call reads (tauG1[0 .. 2n),
 * tauG2 / alphaTauG1 / betaTauG1 [0 .. n), betaG2): canonical and on the curve for every element, the order-r subgroup
 * for the G2 arrays.  An element that fails is G16_EINVAL; g16_last_error names section, index and check in the words
 * of the circuit-audit report ("ptau tauG2[3] is not in the order-r subgroup").
 * G16_EINVAL, checked on the host before anything is queued: a null pointer; an unknown flavour or flags; a matrix entry
 * out of range or not canonical; nvars <= npubs; a domain above 2^24; ptau->power < log2_domain + 1 (the audit's rule);
 * delta zero or >= r.  No output is promised after a failure.
 * The call changes no context state (a context proves the same bytes before and after), runs on the context's stream
 * with one wait after the element passes and one at the end; intermediates stay in HBM between the stages.  Outputs are
 * canonical affine bytes. */
int32_t g16_circuit_setup(g16_ctx* ctx, const g16_r1cs_desc* r1cs, const g16_ptau_desc* ptau, const void* delta,
                          g16_setup_points* out);

/* ---- NTT: replaces forwardNTT / inverseNTT (groth16/math/ntt.nim:55-77, 139-161) ------------------- */
/* natural order in and out; forward unscaled, inverse includes 1/n; omega = gen28^(2^(28-log2n))
 * (math/domain.nim:26-33).  src/dst: n = 2^log2n Fr elements (Montgomery), host memory. 0 <= log2n <= 28 */
int32_t g16_ntt_fr(g16_ctx* ctx, const void* src, void* dst, uint32_t log2n, int32_t inverse);
/* _dev: device pointers on the context's device, ordered on its stream; d_dst may equal d_src (in place). */
int32_t g16_ntt_fr_dev(g16_ctx* ctx, const void* d_src, void* d_dst, uint32_t log2n, int32_t inverse);

/* ---- quotient: replaces computeSnarkjsScalarCoeffs (flavour 1, groth16/prover.nim:158-181) and
 *      computeQuotientPointwise (flavour 0, prover.nim:118-148) -------------------------------------------
 * Az, Bz, Cz, out: n = 2^log2n Fr elements (Montgomery).  Snarkjs: out[j] = A1[j]*B1[j] - C1[j] on the coset
 * eta*H, eta = w_(2n); JensGroth: the n coefficients of (A*B - C)/Z.  log2n <= 27. */
#define G16_FLAVOUR_JENSGROTH 0u /* zkey_types.nim:11 */
#define G16_FLAVOUR_SNARKJS 1u   /* zkey_types.nim:12 */
int32_t g16_quotient(g16_ctx* ctx, const void* Az, const void* Bz, const void* Cz, uint32_t log2n, uint32_t flavour,
                     void* out);
int32_t g16_quotient_dev(g16_ctx* ctx, const void* d_Az, const void* d_Bz, const void* d_Cz, uint32_t log2n,
                         uint32_t flavour, void* d_out);

/* ---- proving key + proof: replaces generateProofWithMask (groth16/prover.nim:215-304) -----------------
 * g16_pkey_create uploads a ZKey (zkey_types.nim:54-59) once: the five ProverPoints arrays become
 * registered point sets, ZKey.coeffs becomes a device CSR for buildABC (prover.nim:56-73). */
typedef struct g16_pkey g16_pkey;
typedef struct {          /* one Coeff (zkey_types.nim:48-52) */
  uint32_t matrix;        /* 0 = MatrixA, 1 = MatrixB (MatrixC is rejected, as prover.nim:67 raises) */
  uint32_t row;           /* 0 .. domainSize-1 */
  uint32_t col;           /* 0 .. nvars-1 */
  uint32_t reserved;
  uint8_t value[32];      /* Fr, Montgomery */
} g16_coeff;
typedef struct {
  uint32_t nvars, npubs;  /* GrothHeader (zkey_types.nim:14-22) */
  uint32_t log2_domain;   /* logDomainSize */
  uint32_t flavour;       /* G16_FLAVOUR_* */
  const void *pointsA1, *pointsB1; /* nvars G1 points each          (zkey_types.nim:37-38) */
  const void* pointsB2;            /* nvars G2 points               (:39) */
  const void* pointsC1;            /* nvars - npubs - 1 G1 points   (:40) */
  const void* pointsH1;            /* domainSize G1 points          (:41) */
  const g16_coeff* coeffs;
  size_t ncoeffs;
  const void *alpha1, *beta1, *delta1; /* SpecPoints G1 (zkey_types.nim:24-31) */
  const void *beta2, *delta2;          /* SpecPoints G2 */
  /* multi-GPU: this key keeps only index range [N*i/count, N*(i+1)/count) of each point set -- the contiguous
   * chunks of msmMultiThreadedG1/G2 (msm.nim:105-115) with one chunk per GPU.  0/0 or 0/1 = whole key. */
  uint32_t shard_index, shard_count;
} g16_pkey_desc;
typedef struct { /* Proof (prover.nim:37-43) minus publicIO (= witness[0..npubs], which the caller already has) */
  uint8_t pi_a[64];
  uint8_t pi_b[128];
  uint8_t pi_c[64];
} g16_proof;
int32_t g16_pkey_create(g16_ctx* ctx, const g16_pkey_desc* desc, g16_pkey** out);
/* The same with ZKey.coeffs taken straight from the .zkey FILE: `section4` = section 4 as it lies on disk -- u32 count,
 * then count x { u32 matrix, u32 row, u32 col, 32-byte value in DOUBLE Montgomery form c R^2 } (files/zkey.nim:169-192;
 * the reference un-Montgomerys each value twice while loading, io.nim:134-139 unmarshalFrWTF) -- and desc->coeffs = NULL,
 * desc->ncoeffs = 0.  No host arithmetic and no 48-byte records: with the point sections of the file (plain Montgomery
 * bytes = the in-memory layout) and a raw .wtns witness (G16_SCALARS_STD) a memory-mapped .zkey / .wtns pair is proved
 * without being parsed.  c R^2 is also exactly what buildABC multiplies a raw .wtns value with: (c R^2) w / R = c w R. */
int32_t g16_pkey_create_zkey(g16_ctx* ctx, const g16_pkey_desc* desc, const void* section4, size_t section4_bytes,
                             g16_pkey** out);
/* The same two with all five point sets of the key registered at one table stride (g16_points_register_*_lean):
 * table_stride 0 or 1 is exactly g16_pkey_create / g16_pkey_create_zkey.  Proofs are the same bytes at every stride. */
int32_t g16_pkey_create_lean(g16_ctx* ctx, const g16_pkey_desc* desc, uint32_t table_stride, g16_pkey** out);
int32_t g16_pkey_create_zkey_lean(g16_ctx* ctx, const g16_pkey_desc* desc, const void* section4, size_t section4_bytes,
                                  uint32_t table_stride, g16_pkey** out);
void g16_pkey_destroy(g16_pkey* key);
/* points at infinity per ProverPoints array of this key (this shard): out[0..4] = A1, B1, B2, C1, H1; out[5] = wires
 * whose B1 AND B2 points are both (0,0); out[6] / out[7] = 1 if A1 / B1+B2 run on compacted entry lists (their own
 * arrangement of the witness without those wires; sets below the G16_INF_COMPACT threshold share one arrangement). */
int32_t g16_pkey_inf_counts(const g16_pkey* key, size_t out[8]);
/* pointsB1 folded into pointsA1.  Both sets meet the same scalars, so MSM(w, B1) = MSM(w, A1) + MSM(w, B1 - A1), and the
 * difference is the point at infinity for every wire whose columns of A and B coincide (squarings, boolean checks).  At
 * key creation the library counts, over the key's WHOLE wire range, live_b1 = pointsB1 entries that are not (0,0) and
 * live_delta = wires whose two points differ, and keeps in place of pointsB1
 *   1: nothing, if live_delta = 0;
 *   2: the differences, if live_delta * 100 <= live_b1 * (100 - G16_INF_COMPACT) -- and, where pointsB1 holds enough
 *      (0,0) entries to run on a compacted entry list, only if live_delta * 64 <= live_b1: the differences ride the entry
 *      list of all wires, where 64 neighbours at infinity are skipped together;
 *   0: pointsB1 as it is, otherwise and always under G16_B1_FOLD=0.
 * out[0] = that form, out[1] = live_b1, out[2] = live_delta.  Proofs are the same bytes in every form. */
int32_t g16_pkey_b1_fold(const g16_pkey* key, size_t out[3]);
/* How a key of form 2 runs its B1 job.  With at most out[2] (= 64) live differences over the key's WHOLE wire range it
 * also keeps the list of its live wires, and the job forms its bucket sums from those wires' witness values alone (the
 * sparse run) instead of reading the arrangement of all wires: out[0] = 1.  out[1] = the live differences inside THIS
 * key's wire range (a shard may hold none).  Keys of the other forms, and of form 2 with more live differences: out[0] =
 * out[1] = 0.  Proofs are the same bytes either way. */
int32_t g16_pkey_b1_sparse(const g16_pkey* key, size_t out[3]);
/* witness: nvars Fr values (flags: G16_SCALARS_MONT for Nim seq[Fr], G16_SCALARS_STD for raw .wtns,
 * | G16_SCALARS_DEVICE); mask_r / mask_s: Fr Montgomery (Mask, prover.nim:210-213), NULL = zero
 * (generateProofWithTrivialMask, prover.nim:308-310). */
int32_t g16_prove(g16_ctx* ctx, const g16_pkey* key, const void* witness, uint32_t flags, const void* mask_r,
                  const void* mask_s, g16_proof* out);
/* The two halves of g16_prove, for a proof sharded over several GPUs (one g16_ctx + one sharded key per GPU):
 *  g16_prove_partials: buildABC + quotient (replicated) and the five MSMs over this key's index ranges;
 *      writes G16_PARTIALS_BYTES = 768 bytes: XYZZ accumulators A1 | B1 | B2 (256 B) | H1 | C1.  The record is
 *      opaque: accumulators are not canonical (the addition order inside a bucket is not fixed), and when the C1 and
 *      H1 sets share their bucket set the H1 slot holds H1 + C1 and the C1 slot infinity (pi_c needs only the sum,
 *      prover.nim:301-302); for a key with pointsB1 folded into pointsA1 (g16_pkey_b1_fold) the B1 slot holds the
 *      MSM over the differences B1 - A1 and g16_prove_combine adds the A1 slots to it.  Only g16_prove_combine gives records a meaning; it accepts any mix of them.
 *      flags: G16_SCALARS_MONT/STD | G16_SCALARS_DEVICE (witness in HBM) | G16_OUT_DEVICE (output in HBM).
 *  g16_prove_combine: `count` gathered records (rank order; e.g. from an RCCL all-gather) are summed per MSM
 *      -- the `res += sync pending[k]` of msm.nim:117-119 across GPUs -- and the mask algebra of
 *      prover.nim:279-302 yields the proof.  flags: G16_SCALARS_DEVICE if `partials` is a device pointer. */
#define G16_PARTIALS_BYTES 768
int32_t g16_prove_partials(g16_ctx* ctx, const g16_pkey* key, const void* witness, uint32_t flags, void* out_partials);
int32_t g16_prove_combine(g16_ctx* ctx, const g16_pkey* key, const void* partials, size_t count, uint32_t flags,
                          const void* mask_r, const void* mask_s, g16_proof* out);
/* Sharded proof with a TASK-PARALLEL quotient (snarkjs-flavour keys): the three coset pipelines that
 * computeSnarkjsScalarCoeffs runs as three Taskpool tasks (prover.nim:167-169) live on three different ranks instead
 * of being replicated on all of them.
 *  g16_prove_partials_begin: uploads the witness, launches this key's four witness MSMs (they keep running after
 *      the call returns) and computes the coset vectors named by task_mask (bit 0: A, 1: B, 2: C) -- buildABC +
 *      shiftEvalDomain (prover.nim:56-73, 109-113) -- into d_task_out: domainSize Fr per set bit, in ascending bit
 *      order, device memory.  flags as for g16_prove_partials.  task_mask = 0: this rank owns no pipeline.
 *  (caller: every rank receives the [h_lo, h_hi) slices of the three coset vectors, h = domainSize * rank / count,
 *      from the ranks that own them -- three scatters; 32 * domainSize / count bytes per slice)
 *  g16_prove_partials_end: forms this rank's H scalars A1*B1 - C1 from the received slices (device pointers,
 *      h_hi - h_lo Fr each; prover.nim:175-176), runs the H MSM over them, joins the witness MSMs and writes the
 *      768-byte record exactly like g16_prove_partials.  Then g16_prove_combine as usual.
 *  Between _begin and _end the witness MSMs are in flight on this context's workspaces.  Only g16_ctx_synchronize
 *  and the g16_profile_* calls leave them alone; ANY other call on the context first waits for them and cancels
 *  the pending proof (a later _end returns G16_EINVAL) -- so a caller whose exchange failed may simply go on, and
 *  one that wants to overlap two sharded proofs uses two contexts (nim_groth16_amd/distributed.py does).
 *  flags for _begin additionally: G16_NO_HOST_SYNC -- return without waiting for the coset vectors; the caller
 *  orders its exchange behind them through the context's stream (g16_ctx_set_stream: e.g. torch's current stream,
 *  on which the collective is then enqueued).
 *  G16_NO_HOST_SYNC, the rules: (1) _begin honours it wherever the witness lives.  A HOST witness must then be in
 *  pinned memory (otherwise the copy blocks anyway) and must stay untouched until the context's stream has passed the
 *  copy -- e.g. until the matching _end or g16_prove_combine has returned, or an event recorded on that stream after
 *  _begin has completed; the library does not wait for it.  (2) g16_prove_partials and _end honour it only together
 *  with G16_OUT_DEVICE (a record written to host memory is not complete in stream order for the host); without
 *  G16_OUT_DEVICE the flag is ignored and the call waits as usual. */
int32_t g16_prove_partials_begin(g16_ctx* ctx, const g16_pkey* key, const void* witness, uint32_t flags,
                                 uint32_t task_mask, void* d_task_out);
int32_t g16_prove_partials_end(g16_ctx* ctx, const g16_pkey* key, const void* d_a1_slice, const void* d_b1_slice,
                               const void* d_c1_slice, uint32_t flags, void* out_partials);
/* buildABC alone (prover.nim:56-73): out_abc = Az | Bz | Cz, 3 * domainSize Fr (Montgomery), host memory */
int32_t g16_build_abc(g16_ctx* ctx, const g16_pkey* key, const void* witness, uint32_t flags, void* out_abc);
/* shape of the key's A / B matrices as buildABC sees them (ZKey.coeffs, zkey_types.nim:48-59; files/zkey.nim:169-192):
 * out[0] = ncoeffs; out[1] = distinct coefficient values if the key runs on a value dictionary (entries are then
 * 8 bytes: column + value index), else 0 (36 bytes: column + value); out[2 + b], b = 0..8 = rows of A or of B (2 per
 * domain row) by their number of terms L: L <= 1, L = 2, L <= 4 (one lane each), then L <= 8, 16, 32, 64, 128 and
 * longer: groups of 2, 4, 8, 16, 32, 64 lanes with four terms per lane */
int32_t g16_pkey_abc_info(const g16_pkey* key, size_t out[11]);
/* y = M x over Fr (Montgomery in and out) for a sparse M given as nnz triplets (row[i], col[i], val[i] = 32 bytes);
 * entries of one row add up.  The same row-balanced kernel as buildABC.  Replaces the sparse column dot products of
 * the fake setup -- `for each coefficient: taus[wire] += value * L_row(tau)` (fake_setup.nim:159-187, 254-256): pass
 * row = wire, col = constraint, x = the Lagrange values.  Host pointers; x: ncols elements, y: nrows elements. */
int32_t g16_spmv_fr(g16_ctx* ctx, const uint32_t* row, const uint32_t* col, const void* val, size_t nnz, const void* x,
                    size_t ncols, size_t nrows, void* y);

/* ---- device group: one proof over several GPUs from ONE host process -------------------------------------------------
 * The reference is one process whose MSMs run as Taskpool tasks over contiguous index ranges, partial sums added in task
 * order (groth16/bn128/msm.nim:96-122), and whose three coset pipelines are three tasks (prover.nim:165-173).  A group is
 * that shape with GPUs in place of threads: member g = a context on devices[g] + shard g of ndev of the key, one host
 * thread per member INSIDE the library; per proof the members exchange 3 x 32 n / ndev bytes of coset slices (peer copies
 * between their HBMs) and member 0 adds the ndev 768-byte records in member order.  The caller needs no Python, no
 * torch.distributed and no RCCL; it calls g16_group_prove where it called generateProofWithMask.
 *   devices: HIP device ordinals, one per member (a device may repeat: several members then share it)
 *   g16_group_pkey_create: desc = the WHOLE key (shard_count 0 or 1); member g keeps index range g of every point set
 *   g16_group_prove: witness = nvars Fr in HOST memory (flags: G16_SCALARS_MONT or G16_SCALARS_STD), masks as g16_prove;
 *       the proof is bit-identical to g16_prove's on the unsharded key
 * A group is used by one host thread at a time; its keys may be destroyed before or after it.  (Python ranks over RCCL: nim_groth16_amd/distributed.py does the same
 * exchange with one process per GPU.) */
typedef struct g16_group g16_group;
typedef struct g16_group_pkey g16_group_pkey;
int32_t g16_group_create(const int32_t* devices, int32_t ndev, g16_group** out);
void g16_group_destroy(g16_group* group);
int32_t g16_group_size(const g16_group* group);
const char* g16_group_last_error(const g16_group* group);
int32_t g16_group_pkey_create(g16_group* group, const g16_pkey_desc* desc, g16_group_pkey** out);
/* ... with every member's point sets at one table stride (g16_pkey_create_lean) */
int32_t g16_group_pkey_create_lean(g16_group* group, const g16_pkey_desc* desc, uint32_t table_stride,
                                   g16_group_pkey** out);
void g16_group_pkey_destroy(g16_group_pkey* key);
int32_t g16_group_prove(g16_group* group, const g16_group_pkey* key, const void* witness, uint32_t flags,
                        const void* mask_r, const void* mask_s, g16_proof* out);

/* ---- prover pool: proofs in flight from ONE host thread -------------------------------------------------------------
 * generateProofWithMask (prover.nim:215-304) is one blocking call; g16_prove keeps that shape, so one caller gets one
 * proof at a time.  A pool runs `depth` proofs on one GPU at once behind a submit / poll / collect interface, with no
 * host thread inside the library: every step is taken inside the caller's own calls.
 *   g16_prover_create: depth (1..8) = proofs running on the GPU at once; the pool owns `depth` contexts on `device`,
 *       all proving against the one resident `key`, which must outlive the pool.  G16_EINVAL for a sharded key
 *       (shard_count != 1), a key of another device, or depth 0 or > 8.
 *   g16_prover_submit: never waits for the GPU.  Accepts up to depth + 1 outstanding (uncollected) proofs; the extra one
 *       is PREFETCHED: its witness starts uploading at once (a copy stream and a device witness buffer owned by the pool)
 *       and its kernels are enqueued as soon as any pool call (submit, poll, collect) sees a running proof finished.
 *       With depth + 1 outstanding it returns G16_EBUSY, enqueues nothing and leaves the ticket counter unchanged.
 *       flags: G16_SCALARS_MONT or G16_SCALARS_STD, | G16_SCALARS_DEVICE, as for g16_prove.  The masks (NULL = zero)
 *       are copied before it returns; the witness must stay valid and unmodified until g16_prover_poll has returned 1
 *       for its ticket or g16_prover_collect has returned.  A pageable host witness is accepted, but submit then returns
 *       only once HIP has taken the copy: memory from g16_host_alloc avoids that.  Tickets count up from 1.
 *   g16_prover_poll: never blocks; 1 = done, 0 = pending.  g16_prover_collect: waits for that ticket's proof and
 *       writes exactly the bytes g16_prove(ctx, key, witness, flags, mask_r, mask_s, out) writes.  Both take tickets in
 *       any order; an unknown ticket, and one already collected, give G16_EINVAL.
 *   Failure: after the first HIP or allocation failure the pool is FAILED: every later submit / poll / collect returns
 *       that code and g16_prover_last_error gives the first message.  Only g16_prover_destroy stays valid.
 *   g16_prover_destroy: waits for every outstanding proof, discards them and releases what the pool owns; the key and
 *       other contexts stay usable.
 * A pool is used by one host thread at a time (any thread), like a g16_ctx; other contexts may prove against the same
 * key concurrently.
 *   g16_host_alloc / g16_host_free: pinned (page-locked) host memory for witnesses; G16_ENODEV without a device. */
#define G16_EBUSY (-6) /* g16_prover_submit: depth + 1 proofs are already outstanding; nothing was enqueued */
typedef struct g16_prover g16_prover;
int32_t g16_prover_create(int32_t device, const g16_pkey* key, uint32_t depth, g16_prover** out);
void g16_prover_destroy(g16_prover* p);
const char* g16_prover_last_error(const g16_prover* p);
int32_t g16_prover_submit(g16_prover* p, const void* witness, uint32_t flags, const void* mask_r, const void* mask_s,
                          uint64_t* ticket);
int32_t g16_prover_poll(g16_prover* p, uint64_t ticket); /* 1 done, 0 pending, <0 error */
int32_t g16_prover_collect(g16_prover* p, uint64_t ticket, g16_proof* out);
int32_t g16_host_alloc(int32_t device, size_t bytes, void** out); /* pinned host memory */
void g16_host_free(void* p);

/* ---- verifier ------------------------------------------------------------------------
 * Replaces verifyProof (groth16/verifier.nim:31-52), extractVKey / VKey (groth16/zkey_types.nim:62-73) and the
 * `pairing` of bn128/curves.nim:218-221, on the device, batched over proofs.
 *
 * g16_vkey_desc: npubs = number of public inputs; pointsIC holds npubs + 1 G1 points (the first one belongs to
 * the constant 1).  alpha1: 64 B; beta2, gamma2, delta2: 128 B each (Montgomery affine, as everywhere).
 * g16_verify: `public_io` = count x (npubs + 1) scalars, each row starting with the constant 1 exactly like
 * Proof.publicIO (prover.nim:238-240); flags: G16_SCALARS_MONT / G16_SCALARS_STD for the scalars, and
 * G16_VERIFY_SUBGROUP to also require [r]pi_b = infinity (the reference only asserts the curve equations).
 * status[j]: 1 = proof j verifies, 0 = pairing equation fails, -1 / -2 / -3 = pi_a / pi_b / pi_c is not on its
 * curve (the reference's three asserts), -4 = pi_b is not in the order-r subgroup, -5 = a proof coordinate is not
 * the canonical residue (limbs >= p), -6 = a public input is not canonical (>= r): each proof / input has exactly
 * one accepted byte encoding.  (The smallest code wins when several apply.)
 * g16_pairing: out_gt[i] = e(P_i, Q_i) as 6 x Fp2 = 384 bytes, coefficient k of w^k in
 * Fp12 = Fp2[w]/(w^6 - (9+u)) (the tower of files/export_sage.nim:84-97 flattened), Montgomery form;
 * e is the ate pairing f_{t-1,Q}(P)^((p^12-1)/r).  NOT byte-compatible with the GT values of the reference's
 * `pairing` (constantine's optimal ate, curves.nim:218-221): the two differ by a fixed exponent, so products /
 * equality-to-one tests (all verifyProof needs) agree, the 384 bytes do not. */
typedef struct g16_vkey g16_vkey;
typedef struct {
  uint32_t npubs;
  const void* alpha1;
  const void* beta2;
  const void* gamma2;
  const void* delta2;
  const void* pointsIC;
} g16_vkey_desc;
#define G16_VERIFY_SUBGROUP 16u
#define G16_GT_BYTES 384
int32_t g16_vkey_create(g16_ctx* ctx, const g16_vkey_desc* desc, g16_vkey** out);
void g16_vkey_destroy(g16_vkey* key);
int32_t g16_verify(g16_ctx* ctx, const g16_vkey* key, const g16_proof* proofs, const void* public_io, uint32_t flags,
                   size_t count, int32_t* status);
int32_t g16_pairing(g16_ctx* ctx, const void* g1_points, const void* g2_points, size_t n, void* out_gt);
/* One pairing-product check for the whole batch ("do they all verify?"), the random-linear-combination check:
 *   prod_j e(-z_j A_j, B_j) * e(sum_j z_j C_j, delta2) * e(sum_i s_i IC_i, gamma2) * e((sum_j z_j) alpha1, beta2) == 1,
 *   s_i = sum_j z_j pub_{j,i} (mod r):  count + 3 Miller loops and ONE final exponentiation per batch.
 * proofs, public_io, key, count (< 2^22) and G16_SCALARS_MONT / G16_SCALARS_STD: as for g16_verify.
 * multipliers: count x 16 bytes, little-endian 128-bit integers z_j, host memory, every one non-zero, drawn by the
 * CALLER from a CSPRNG after the proofs are fixed.  The library draws no randomness itself.
 * *result = 1: no proof has a structural defect (the negative codes of g16_verify) and the combined equation holds;
 * 0 otherwise.  count == 0 gives 1.
 * The order-r check on pi_b is ALWAYS applied (G16_VERIFY_SUBGROUP is implied: the combination is only sound on G2).
 * Soundness: if at least one proof would not get status 1 from g16_verify with G16_VERIFY_SUBGROUP, then
 * *result == 1 with probability at most 1/(2^128 - 1), for multipliers uniform over the non-zero 128-bit values and
 * independent of the proofs: the proofs' defects form a non-zero linear form in the z_j over Fr, and r > 2^128.
 * Multipliers that the prover can predict (or equal ones) void the bound.
 * status: NULL, or count entries.  result 1 -> all 1.  result 0 -> exactly what
 * g16_verify(ctx, key, proofs, public_io, flags | G16_VERIFY_SUBGROUP, count, status) writes (the per-proof kernels
 * run on the data already uploaded; NULL skips them).
 * G16_EINVAL: NULL result, NULL multipliers with count > 0, any z_j == 0 (checked on the host before anything is
 * queued; g16_last_error names the index). */
int32_t g16_verify_batch(g16_ctx* ctx, const g16_vkey* key, const g16_proof* proofs, const void* public_io,
                         uint32_t flags, size_t count, const void* multipliers, int32_t* result, int32_t* status);

/* ---- key audit: is an UNTRUSTED proving key fit to prove with? ------------------------------------------------------
 * g16_pkey_create* take a key as it is, and g16_points_check_* are the reference's curve asserts only (mkG1 / mkG2,
 * curves.nim:95-107).  The calls below are for a service that is handed .zkey files by third parties.  None of them
 * changes any state: a context proves the same bytes before and after.  Host pointers throughout.
 *
 * g16_points_audit_g1/g2: three checks per element, in this precedence:
 *   [0] canonical: every Fp limb pattern is < p
 *   [1] on the curve y^2 = x^3 + b; (0,0) is infinity and passes
 *   [2] in the order-r subgroup, [r]Q == infinity by the definition (G2 only: G1 has cofactor 1, its [2] is always
 *       "none")
 * An element that fails a check is counted under that check ONLY and is not examined by the later ones: the field
 * arithmetic would silently reduce a non-canonical pattern, so an alias of a valid point would pass [1] and [2].
 * first_bad[k] = index of the first element failing check k, (size_t)-1 when none does; bad_count[k] = how many.
 * n < 2^31. */
int32_t g16_points_audit_g1(g16_ctx* ctx, const void* points, size_t n, size_t first_bad[3], size_t bad_count[3]);
int32_t g16_points_audit_g2(g16_ctx* ctx, const void* points, size_t n, size_t first_bad[3], size_t bad_count[3]);
/* Do P_i (G1) and Q_i (G2) have the same logarithm, P_i = k_i gen1 and Q_i = k_i gen2, for every i?  One
 * random-linear-combination pairing equation:
 *   *result = 1 exactly when  e(sum_i z_i P_i, gen2) * e(-gen1, sum_i z_i Q_i) == 1,  0 otherwise  (n == 0 gives 1):
 * two one-shot MSMs, two Miller loops, one final exponentiation.
 * PRECONDITION: both arrays pass g16_points_audit_* (no element fails any check).  The call does not repeat those
 * checks, and its arithmetic is only defined on canonical points of the curve and subgroup.
 * multipliers: n x 16 bytes, little-endian 128-bit z_i, every one non-zero, drawn by the CALLER from a CSPRNG after the
 * arrays are fixed, exactly as for g16_verify_batch; the library draws no randomness.  A zero multiplier: G16_EINVAL,
 * g16_last_error names the index.  n < 2^27.
 * Soundness, as for g16_verify_batch: with P_i = a_i gen1 and Q_i = b_i gen2 the equation says sum_i z_i (a_i - b_i) = 0
 * (mod r); if any a_i != b_i that is a non-zero linear form in the z_i over Fr, so *result == 1 with probability at most
 * 1/(2^128 - 1) over multipliers uniform in the non-zero 128-bit values and independent of the arrays. */
int32_t g16_points_pairs_check(g16_ctx* ctx, const void* g1_points, const void* g2_points, size_t n,
                               const void* multipliers, int32_t* result);
/* The whole key.  Sections, in the order of the report: */
#define G16_AUDIT_SECTIONS 13
enum {
  G16_SEC_ALPHA1 = 0, G16_SEC_BETA1, G16_SEC_DELTA1, G16_SEC_BETA2, G16_SEC_GAMMA2, G16_SEC_DELTA2, G16_SEC_POINTS_IC,
  G16_SEC_POINTS_A1, G16_SEC_POINTS_B1, G16_SEC_POINTS_B2, G16_SEC_POINTS_C1, G16_SEC_POINTS_H1, G16_SEC_COEFFS
};
#define G16_AUDIT_CANONICAL 1u     /* some element fails check [0] */
#define G16_AUDIT_CURVE 2u         /* ... check [1] */
#define G16_AUDIT_SUBGROUP 4u      /* ... check [2] */
#define G16_AUDIT_RELATION 8u      /* a relation that was run does not hold */
#define G16_AUDIT_SPEC_INFINITY 16u /* a spec point is (0,0): on the curve, but no key of a real setup holds one */
typedef struct {
  uint32_t failed;        /* OR of G16_AUDIT_*; 0 = fit to prove with */
  uint32_t spec_infinity; /* bit s set: spec point s (G16_SEC_ALPHA1 .. G16_SEC_DELTA2) is (0,0) */
  /* [0] pointsB1 ~ pointsB2 (g16_points_pairs_check with the multipliers), [1] beta1 ~ beta2, [2] delta1 ~ delta2 (the
   * last two exact: two Miller loops each, no multipliers).  1 = holds, 0 = fails, -1 = not run: a section it reads
   * failed an element check, or (for [0]) multipliers == NULL */
  int32_t relation[3];
  uint32_t reserved;
  size_t first_bad[G16_AUDIT_SECTIONS][3]; /* per section and check, as g16_points_audit_* */
  size_t bad_count[G16_AUDIT_SECTIONS][3];
} g16_key_report;
/* desc: the key as for g16_pkey_create* (a sharded one, shard_count > 1, is G16_EINVAL: audit the whole key).
 * vk: NULL, or the key's verification half -- only gamma2 and pointsIC (npubs + 1 points; vk->npubs == desc->npubs) are
 *   read from it; with NULL those two sections are reported as empty.
 * coefficients: desc->coeffs / ncoeffs, or section 4 of the .zkey as for g16_pkey_create_zkey (then desc->coeffs = NULL,
 *   desc->ncoeffs = 0); section4 == NULL and no desc->coeffs: none.  Only check [0] applies to them: the value is < r
 *   (the Montgomery limbs of a g16_coeff; for section 4 the 32-byte integer on file) -- buildABC's products are only
 *   correct for operands < r.  A matrix selector, row or column out of range is G16_EINVAL, as for g16_pkey_create*.
 * multipliers: desc->nvars x 16 bytes as for g16_points_pairs_check, or NULL to skip the pointsB1 ~ pointsB2 relation.
 * Every array is uploaded whole, one at a time, into the context's staging buffer; all work runs on the context's
 * stream with one wait after the element passes (the relations run only on sections whose every element passed)
 * and one at the end.
 * What the audit CANNOT establish: that the key belongs to any circuit.  Nothing in the key alone ties pointsA1 /
 * pointsC1 / pointsH1 / pointsIC (or the values of alpha, beta, gamma, delta) to an R1CS; a key can pass every check
 * here and still prove nothing about the statement its user has in mind.  A caller who also holds the circuit's .r1cs
 * and the ceremony's .ptau can establish that tie: g16_circuit_audit, below. */
int32_t g16_key_audit(g16_ctx* ctx, const g16_pkey_desc* desc, const g16_vkey_desc* vk, const void* section4,
                      size_t section4_bytes, const void* multipliers, g16_key_report* out);

/* ---- circuit audit: does an UNTRUSTED proving key belong to THIS circuit and THIS powers of tau? --------------------
 * What `snarkjs zkey verify circuit.r1cs pot.ptau circuit.zkey` checks before it walks the contribution chain; the
 * reference lists a piece of it as open ("compare .r1cs to the 'coeffs' section of .zkey").  The caller's multipliers
 * z (one per wire) are treated as a witness: buildABC over the key's coefficients and the same products over the R1CS
 * must agree, and every point array of the key, combined with z, must equal the matching combination of the powers of
 * tau.  Like the key audit the call changes no state: a context proves the same bytes before and after.  Host pointers.
 *
 * g16_r1cs_desc: the R1CS as triplets, the first members of g16_setup_desc under the same rules (entries of one
 *   (constraint, wire) add up; the library adds snarkjs's dummy A entries (nconstraints + i, wire i, 1), i <= npubs).
 * g16_ptau_desc: sections 2..6 of a .ptau, Montgomery affine like every point here. */
struct g16_r1cs_desc_s {
  uint32_t nvars, npubs, nconstraints;
  uint32_t flavour;         /* must equal the key's */
  const uint32_t* row[3];
  const uint32_t* col[3];
  const void* val[3];
  size_t nnz[3];
  uint32_t flags;           /* G16_SCALARS_MONT or G16_SCALARS_STD for val */
};
struct g16_ptau_desc_s {
  uint32_t power;           /* tauG1: 2^(power+1) - 1 points; tauG2, alphaTauG1, betaTauG1: 2^power; betaG2: 1 */
  const void *tauG1, *tauG2, *alphaTauG1, *betaTauG1, *betaG2;
};
#define G16_PTAU_SECTIONS 5
#define G16_CIRCUIT_RELATIONS 9
enum {
  G16_PTAU_TAU_G1 = 0, G16_PTAU_TAU_G2, G16_PTAU_ALPHA_TAU_G1, G16_PTAU_BETA_TAU_G1, G16_PTAU_BETA_G2
};
enum {
  G16_REL_COEFFS_A = 0, G16_REL_COEFFS_B, G16_REL_SPEC, G16_REL_A1, G16_REL_B1, G16_REL_B2, G16_REL_C1, G16_REL_IC,
  G16_REL_H1
};
#define G16_CIRCUIT_KEY 1u     /* the key's own report has failed != 0 */
#define G16_CIRCUIT_PTAU 2u    /* an element of a ptau array fails a check of g16_points_audit_* */
#define G16_CIRCUIT_COEFFS 4u  /* COEFFS_A or COEFFS_B fails */
#define G16_CIRCUIT_SPEC 8u    /* SPEC fails */
#define G16_CIRCUIT_POINTS 16u /* A1, B1, B2, C1, IC or H1 fails */
typedef struct {
  g16_key_report key;       /* exactly what g16_key_audit(ctx, desc, vk, section4, section4_bytes, wire_multipliers) reports */
  /* the five ptau arrays (G16_PTAU_*), only the elements the call reads -- tauG1[0 .. 2n), tauG2 / alphaTauG1 /
   * betaTauG1 [0 .. n), betaG2 -- per check as g16_points_audit_*; check [2] applies to tauG2 and betaG2 */
  size_t ptau_first_bad[G16_PTAU_SECTIONS][3];
  size_t ptau_bad_count[G16_PTAU_SECTIONS][3];
  int32_t relation[G16_CIRCUIT_RELATIONS]; /* G16_REL_*: 1 = holds, 0 = fails, -1 = not run */
  uint32_t failed;          /* OR of G16_CIRCUIT_*; 0 = the key belongs to the circuit and the powers of tau */
  size_t first_row[2];      /* COEFFS_A / COEFFS_B: the first row of the domain where the two products differ, (size_t)-1: none */
} g16_circuit_report;
/* Write n = 2^log2_domain, coef_m(v) = the inverse NTT of v on the m-point domain, z|pub = z with the wires above npubs
 * zeroed, z|priv = z - z|pub.  Every matrix-vector product includes the dummy A entries.  The relations:
 *   COEFFS_A, COEFFS_B  A_key z == A_r1cs z as vectors of n Fr values, for z|pub and for z|priv (B likewise): a comparison
 *             of linear maps -- entry order, duplicates that add up and explicit zeros in either description do not matter
 *   SPEC      alpha1 == alphaTauG1[0], beta1 == betaTauG1[0], beta2 == betaG2 byte for byte; tauG1[0], tauG2[0] = gen1, gen2
 *   A1        MSM(z, pointsA1) == MSM(coef_n(A z), tauG1[0..n))                     (A, B, C below: the R1CS's matrices)
 *   B1, B2    the same with B, against tauG1 and tauG2
 *   C1        e(MSM(z|priv, pointsC1), delta2) == e(R, gen2),  R = MSM(coef_n(A z|priv), betaTauG1)
 *             + MSM(coef_n(B z|priv), alphaTauG1) + MSM(coef_n(C z|priv), tauG1); no private wire: holds trivially (1)
 *   IC        the same over z|pub with gamma2 and pointsIC; -1 when vk == NULL
 *   H1        e(MSM(y, pointsH1), delta2) == e(MSM(c, tauG1[0..2n)), gen2), y = h_multipliers; snarkjs flavour:
 *             c = coef_2n(v), v[2i+1] = y_i, v[even] = 0; JensGroth: c[i] = -y_i, c[n+i] = +y_i
 * A relation is -1 if a section it reads failed an element check (SPEC reads alpha1, beta1, beta2 and all five ptau
 * arrays; COEFFS_* the key's coefficients): nothing is evaluated on points that are not canonical members of their group.
 * wire_multipliers: nvars x 16 bytes, h_multipliers: n x 16 bytes, under the rules of g16_verify_batch: little-endian
 * 128-bit integers, every one non-zero, drawn by the CALLER from a CSPRNG after every input is fixed; the library draws
 * nothing.  A zero multiplier is G16_EINVAL and g16_last_error names its index.
 * Soundness, as for g16_verify_batch: write every point of the key as its logarithm times the generator.  If the
 * logarithm of any point differs from the value its circuit and the powers of tau give it (or any entry of A_key - A_r1cs,
 * B_key - B_r1cs is non-zero), the relation that covers it is a non-zero linear form in the multipliers over Fr, and
 * r > 2^128: it reports 1 with probability at most 1/(2^128 - 1) over multipliers uniform in the non-zero 128-bit values
 * and independent of the inputs.
 * G16_EINVAL, checked on the host before anything is queued: a null pointer; r1cs->nvars or npubs different from the
 * key's; ceilingLog2(nconstraints + npubs + 1) != log2_domain; a flavour mismatch; an R1CS entry out of range or not
 * canonical; ptau->power < log2_domain + 1 (the rule of `snarkjs zkey new`: tau^(2n-1) is needed and tauG1 holds
 * 2^(power+1) - 1 powers); a sharded key description; everything g16_key_audit rejects.
 * What the call does NOT cover:
 *   - the ptau is the trusted anchor here: its self-consistency (`snarkjs powersoftau verify`) is g16_ptau_verify's, below;
 *   - the phase-2 contribution chain (section 10 of a .zkey) is not walked here: g16_contributions_verify, below, checks
 *     its records against an initial key that this call has tied to the circuit; the hashes stay with the caller;
 *   - gamma and delta are taken from the key: a legitimately contributed key (delta changed, pointsC1 and pointsH1
 *     rescaled) passes, as it should. */
int32_t g16_circuit_audit(g16_ctx* ctx, const g16_pkey_desc* desc, const g16_vkey_desc* vk, const void* section4,
                          size_t section4_bytes, const g16_r1cs_desc* r1cs, const g16_ptau_desc* ptau,
                          const void* wire_multipliers, const void* h_multipliers, g16_circuit_report* out);

/* ---- witness check: which constraints does an UNTRUSTED witness break? -------------------------------------------------
 * What `snarkjs wtns check circuit.r1cs witness.wtns` answers.  The proving calls take a witness as it is: a value >= r
 * is multiplied as if it were a residue, and a witness that breaks a constraint gives a proof that does not verify with
 * nothing that says why (the prover forms Cz := Az * Bz and never sees the real C z).  A service creates the constraint
 * system once, checks every witness against it, and proves only when the report has failed == 0.
 *
 * g16_r1cs: a constraint system resident in HBM; immutable, belongs to the device of the creating context like a
 *   g16_pkey; any context of that device may check against it, several at once, and it may be destroyed before or after
 *   any context.
 * desc: the struct of the circuit audit under its rules -- entries of one (constraint, wire) add up, explicit zeros are
 *   legal, values in the form desc->flags names.  snarkjs's dummy A entries are NOT added (they belong to a key's
 *   domain, not to the circuit) and rows >= nconstraints do not exist.  npubs (< nvars) and flavour are validated as
 *   elsewhere and otherwise unused.  nconstraints == 0 is legal: every check then reports constraints = 1.
 * G16_EINVAL from g16_r1cs_create, on the host, before anything is queued: a null pointer; an entry out of range; a value
 *   >= r; unknown flags or flavour.  g16_last_error names matrix and entry in the circuit audit's words
 *   ("r1cs matrix 2 entry 5 out of range"). */
typedef struct g16_r1cs g16_r1cs;
int32_t g16_r1cs_create(g16_ctx* ctx, const g16_r1cs_desc* desc, g16_r1cs** out);
void g16_r1cs_destroy(g16_r1cs* r);
/* out: nvars, nconstraints, nnz(A) + nnz(B) + nnz(C), distinct values (0: no value dictionary) */
int32_t g16_r1cs_info(const g16_r1cs* r, size_t out[4]);

#define G16_WITNESS_CANONICAL 1u   /* some value is >= r */
#define G16_WITNESS_ONE 2u         /* witness[0] is not the canonical encoding of 1 in the form named by flags */
#define G16_WITNESS_CONSTRAINTS 4u /* some constraint fails */
#define G16_WITNESS_LIST 16
typedef struct {
  uint32_t failed;                      /* OR of G16_WITNESS_*; 0 = fit to prove with */
  int32_t constraints;                  /* 1 = all hold, 0 = some fail, -1 = not run (a value is not canonical) */
  size_t noncanonical_count, first_noncanonical; /* first = (size_t)-1 when none */
  size_t bad_count;                     /* constraints i with (A z)_i (B z)_i != (C z)_i */
  size_t first_bad[G16_WITNESS_LIST];   /* the min(bad_count, 16) SMALLEST failing indices, ascending; rest (size_t)-1 */
  uint8_t az[32], bz[32], cz[32];       /* the three sums at first_bad[0]: canonical little-endian, standard form; zero
                                           when no constraint fails or the pass did not run */
} g16_witness_report;
/* witness: nvars x 32 bytes; flags: G16_SCALARS_MONT or G16_SCALARS_STD, optionally | G16_SCALARS_DEVICE (the pointer
 * is then a device pointer of the context's device).  Precedence, as in the audits:
 *   1. the canonical pass over every value: the limb pattern (MONT) / the integer (STD) must be < r.  If any value fails,
 *      constraints = -1, the counts and the list stay empty and the sums zero: the field arithmetic would silently reduce
 *      or mis-multiply such a value, so nothing is reported about values that are not residues;
 *   2. ONE: a byte comparison of witness[0] with the canonical encoding of 1 in the named form.  Reported on its own; it
 *      does not stop the constraint pass;
 *   3. the constraint pass: A z, B z and C z over the nconstraints rows as one row-balanced sparse product, then one lane
 *      per constraint compares (A z)_i (B z)_i with (C z)_i.
 * The list is deterministic: the same witness gives the same report, byte for byte, on every call.
 * The call changes no context state (a context proves the same bytes before and after), runs on the context's stream
 * with one wait at the end, and keeps the sums in the calling context's workspace: what crosses back to the host is the
 * report.  G16_EINVAL: a null pointer, unknown flags, a system of another device. */
int32_t g16_witness_check(g16_ctx* ctx, const g16_r1cs* r, const void* witness, uint32_t flags, g16_witness_report* out);

/* ---- scaling an array of points: by ONE scalar, or by a scalar per point ------------------------------------------------
 * out[i] = k * points[i]; host pointers, affine Montgomery in and out, (0,0) legal anywhere; k: 32 bytes, canonical,
 * flags = G16_SCALARS_MONT or G16_SCALARS_STD; k == 0 is legal (all infinity); n < 2^31.  out may be points.
 * The points must be on the curve (g16_points_audit_*): the G1 path multiplies through the endomorphism
 * (x, y) -> (beta x, y), which is only the multiplication by lambda on the curve itself.  G1: the scalar is split as
 * k = k1 + k2 lambda with halves below 2^128 on the host and every lane walks the same joint-sparse-form schedule (~127
 * doublings, ~64 mixed additions); G2: the plain 254-bit ladder.  Both share one field inversion among the four points of
 * a lane for the affine output.  Outputs are canonical affine bytes.  The call changes no context state. */
int32_t g16_points_scale_g1(g16_ctx* ctx, const void* points, size_t n, const void* k, uint32_t flags, void* out);
int32_t g16_points_scale_g2(g16_ctx* ctx, const void* points, size_t n, const void* k, uint32_t flags, void* out);
/* A scalar PER POINT: out[i] = scalars[i] * points[i] (what a powers-of-tau contribution does to tauG1: point i times
 * t^i).  scalars: n x 32 bytes, every one canonical, all in the form `flags` names (G16_SCALARS_MONT or G16_SCALARS_STD);
 * a zero scalar is legal (that output is (0,0)); n < 2^31; out may be points.  Points, outputs and context state: as for
 * g16_points_scale_g1/g2 above (on the curve, (0,0) legal anywhere, canonical affine bytes out, no state changed).
 * G1: every lane splits its own scalar as k = k1 + k2 lambda on the device, halves below 2^128, and walks the columns of
 * (k1, k2) from its own top bit down: one doubling per column and one mixed addition of +-P, +-phi P or +-(P +- phi P)
 * where the column is not empty -- at most 128 doublings and 128 additions against the 254 and 254 of the plain ladder;
 * G2: the plain ladder over the lane's scalar.  One field inversion per four points, as above.
 * G16_EINVAL, checked on the host before anything is queued: a null pointer, flags other than the two, n >= 2^31, a
 * scalar >= r (g16_last_error names its index: "scalar 17 is not canonical (>= r)"). */
int32_t g16_points_scale_each_g1(g16_ctx* ctx, const void* points, size_t n, const void* scalars, uint32_t flags,
                                 void* out);
int32_t g16_points_scale_each_g2(g16_ctx* ctx, const void* points, size_t n, const void* scalars, uint32_t flags,
                                 void* out);

/* ---- phase-2 contribution: what makes the key of g16_circuit_setup(delta = NULL) sound ------------------------------
 * `snarkjs zkey contribute` and the walk of `snarkjs zkey verify` over the contribution chain, as arithmetic: the library
 * hashes nothing and draws nothing.  The secret d, the proof-of-knowledge secret s and the challenge point of a
 * contribution are the CALLER's, like every multiplier in this ABI (Python: nim_groth16_amd/phase2.py derives the
 * challenges from a BLAKE2b transcript -- the project's own rule, NOT snarkjs's: see there).  Host pointers, affine
 * Montgomery points throughout. */
typedef struct {                      /* the part of a key a contribution touches */
  const void *delta1, *delta2;        /* 64 B, 128 B */
  const void *pointsC1, *pointsH1;    /* nc1 and nh1 G1 points (nc1 == 0: pointsC1 may be NULL) */
  size_t nc1, nh1;
} g16_phase2_key;
typedef struct {                      /* one record of the chain: 320 bytes */
  uint8_t delta_after[64];            /* delta1 after this contribution */
  uint8_t g1_s[64], g1_sx[64];        /* s gen1, d s gen1 */
  uint8_t g2_spx[128];                /* d * challenge */
} g16_contribution;
typedef struct {                      /* host buffers the caller owns, sized as the input key's; may not overlap it */
  void *delta1, *delta2, *pointsC1, *pointsH1;
  g16_contribution* record;
} g16_phase2_out;
/* delta1' = d delta1, delta2' = d delta2, pointsC1' = d^-1 pointsC1, pointsH1' = d^-1 pointsH1 (the two arrays through the
 * kernel of g16_points_scale_g1), record = { delta1', s gen1, d s gen1, d challenge_g2 }.
 * d, s: 32 bytes each, canonical, non-zero, in the form `flags` names (G16_SCALARS_MONT or G16_SCALARS_STD).
 * Before any arithmetic the key's elements go through the element passes of g16_points_audit_*: canonical and on the
 * curve for delta1, pointsC1, pointsH1; also the order-r subgroup for delta2 and the challenge.  An element that fails
 * is G16_EINVAL; g16_last_error names section, index and check in the audit's words ("pointsH1[3] is not on the curve").
 * G16_EINVAL also: a null pointer; flags other than the two; d or s zero or >= r; delta1, delta2 or the challenge (0,0).
 * No output is promised after a failure.  The call changes no context state (a context proves the same bytes before and
 * after) and runs on the context's stream with one wait after the element passes and one at the end. */
int32_t g16_key_contribute(g16_ctx* ctx, const g16_phase2_key* key, const void* d, const void* s, uint32_t flags,
                           const void* challenge_g2, g16_phase2_out* out);

/* The chain.  `initial` is the ANCHOR: the key before any contribution, which the caller built with g16_circuit_setup or
 * established with g16_circuit_audit -- it is trusted here and not examined.  `final_` is the key under test, `records`
 * the `count` contributions between them in order, challenges_g2[j] the G2 challenge point sp_j of record j (128 B each;
 * the caller re-derives them from its transcript).  The arrays of a report, in order: */
#define G16_CHAIN_ARRAYS 9
enum {
  G16_CHAIN_DELTA_AFTER = 0, G16_CHAIN_G1_S, G16_CHAIN_G1_SX, G16_CHAIN_G2_SPX, G16_CHAIN_CHALLENGES,   /* count elements */
  G16_CHAIN_FINAL_DELTA1, G16_CHAIN_FINAL_DELTA2, G16_CHAIN_FINAL_POINTS_C1, G16_CHAIN_FINAL_POINTS_H1
};
#define G16_CHAIN_RELATIONS 7
enum {
  G16_CHAIN_ELEMENTS = 0, G16_CHAIN_POK, G16_CHAIN_STEP, G16_CHAIN_LAST, G16_CHAIN_DELTA, G16_CHAIN_C1, G16_CHAIN_H1
};
typedef struct {
  uint32_t failed;                          /* bit k set: relation k (G16_CHAIN_*) is 0; 0 = the chain leads from initial to final */
  int32_t relation[G16_CHAIN_RELATIONS];    /* 1 = holds, 0 = fails, -1 = not run */
  size_t first_record[2];                   /* the first record whose POK / STEP fails, (size_t)-1: none */
  size_t first_bad[G16_CHAIN_ARRAYS][3];    /* per array and check, as g16_points_audit_* */
  size_t bad_count[G16_CHAIN_ARRAYS][3];
  size_t first_infinity[G16_CHAIN_ARRAYS];  /* first (0,0) element of the five record arrays and of final delta1 / delta2, (size_t)-1: none */
} g16_chain_report;
/*   ELEMENTS  every point of the nine arrays is canonical and on its curve, the G2 ones (g2_spx, challenges, final delta2)
 *             in the order-r subgroup, and no delta_after, g1_s, g1_sx, g2_spx, challenge, final delta1 or delta2 is (0,0)
 *   POK       for every record j: e(g1_s, g2_spx) == e(g1_sx, sp_j)             (the contributor knew d: g2_spx = d sp_j)
 *   STEP      for every record j: e(delta_(j-1), g2_spx) == e(delta_after_j, sp_j), delta_0 = initial->delta1
 *   LAST      final->delta1 == records[count-1].delta_after byte for byte; count == 0: == initial->delta1
 *   DELTA     e(final.delta1, gen2) == e(gen1, final.delta2)
 *   C1        e(MSM(z, C1_initial), delta2_initial) == e(MSM(z, C1_final), delta2_final); nc1 == 0: holds trivially
 *   H1        the same with y over pointsH1
 * A relation is -1 when an array it reads failed ELEMENTS (POK: g1_s, g1_sx, g2_spx, challenges; STEP: delta_after,
 * g2_spx, challenges; LAST: delta_after, final delta1; DELTA: final delta1, delta2; C1 / H1: final delta2 and the
 * array).  Every pairing equation is one product of two Miller loops and one final exponentiation in the kernel of the
 * circuit audit's point relations, all of them side by side in ONE launch (a record costs two such products: four Miller
 * loops, two final exponentiations); the four sums are the one-shot MSM; no new arithmetic.
 * c1_multipliers: nc1 x 16 bytes, h1_multipliers: nh1 x 16 bytes, under the rules of g16_verify_batch: little-endian
 * 128-bit integers, every one non-zero, drawn by the CALLER from a CSPRNG after every input is fixed.  A zero multiplier
 * is G16_EINVAL and g16_last_error names its index.  Soundness of C1 / H1 as there: if the final array is not one
 * multiple (delta_initial / delta_final) of the initial one, the relation is a non-zero linear form in the multipliers
 * and holds with probability at most 1/(2^128 - 1).  POK, STEP, LAST and DELTA are exact.
 * G16_EINVAL also: a null pointer; initial->nc1 != final_->nc1 or nh1 likewise; count >= 2^20; nc1 or nh1 >= 2^27 (the
 * limit of the one-shot MSM, as for g16_points_pairs_check).
 * The call changes no context state; one wait after the element passes and one at the end. */
int32_t g16_contributions_verify(g16_ctx* ctx, const g16_phase2_key* initial, const g16_phase2_key* final_,
                                 const g16_contribution* records, const void* challenges_g2, size_t count,
                                 const void* c1_multipliers, const void* h1_multipliers, g16_chain_report* out);

/* ---- phase-1 contribution: powers of tau nobody knows ------------------------------------------------------------------
 * `snarkjs powersoftau contribute` as arithmetic: from the powers of (tau, alpha, beta) to those of (t tau, a alpha,
 * b beta), starting from a file of generators (tau = alpha = beta = 1).  As in phase 2 the library hashes nothing and
 * draws nothing: t, a, b, the three proof-of-knowledge secrets and the three challenge points are the CALLER's (Python:
 * nim_groth16_amd/phase1.py derives the challenges from a BLAKE2b transcript -- the project's own rule, NOT snarkjs's).
 * Host pointers, affine Montgomery points throughout.  g16_ptau_verify, below, checks a .ptau and a chain of these records
 * (`snarkjs powersoftau verify`): the check that g16_circuit_audit and g16_circuit_setup presuppose of their ptau. */
typedef struct {                      /* host buffers the caller owns, sized as the input's arrays; may not overlap them */
  void *tauG1, *tauG2, *alphaTauG1, *betaTauG1, *betaG2;
} g16_ptau_out;
typedef struct {                      /* a proof of knowledge of x: 256 bytes */
  uint8_t g1_s[64], g1_sx[64], g2_spx[128];     /* s gen1, x s gen1, x * challenge */
} g16_ptau_pok;
typedef struct {                      /* one phase-1 record: 1216 bytes */
  uint8_t tauG1[64], alphaG1[64], betaG1[64];   /* after this contribution: tauG1[1], alphaTauG1[0], betaTauG1[0] */
  uint8_t tauG2[128], betaG2[128];              /* tauG2[1], betaG2 */
  g16_ptau_pok pok[3];                          /* x = t, a, b in this order */
} g16_ptau_contribution;
/* tauG1[i] *= t^i (i < 2^(power+1) - 1), tauG2[i] *= t^i, alphaTauG1[i] *= a t^i, betaTauG1[i] *= b t^i (i < 2^power),
 * betaG2 *= b.  The scalars c t^i are made in HBM by the geometric-sequence kernel of the setup and never visit the host;
 * every point meets its own scalar in the kernel of g16_points_scale_each_g1/g2.
 * t, a, b: 32 bytes each; s3: the three proof-of-knowledge secrets for t, a, b (3 x 32 B); all canonical and non-zero, in
 * the form `flags` names (G16_SCALARS_MONT or G16_SCALARS_STD).  challenges_g2: three G2 points (3 x 128 B), for t, a, b.
 * Before any arithmetic all five arrays and the three challenges go through the element passes of g16_points_audit_*:
 * canonical and on the curve, the G2 ones also in the order-r subgroup.  An element that fails is G16_EINVAL and
 * g16_last_error names array, index and check in the audit's words ("ptau tauG2[3] is not in the order-r subgroup",
 * "challenges[1] is not on the curve"); so is a (0,0) element anywhere ("ptau alphaTauG1[7] is the point at infinity").
 * G16_EINVAL also: a null pointer; flags other than the two; a scalar zero or >= r; power == 0 or power > 25.
 * No output is promised after a failure.  The call changes no context state (a context proves the same bytes before and
 * after) and runs on the context's stream with one wait after the element passes and one at the end.
 * HBM: the element passes stage one whole array at a time in the context's staging buffer, which grows to the longest
 * (tauG1: 2^(power+1) x 64 bytes, 4 GiB at power 25) and stays with the context; the arithmetic then takes the long arrays
 * through the device in chunks of at most 2^22 points, one chunk at a time: 2^22 x (128 + 32) bytes = 640 MiB at the peak
 * (a G2 chunk and its scalars), whatever the power. */
int32_t g16_ptau_contribute(g16_ctx* ctx, const g16_ptau_desc* ptau, const void* t, const void* a, const void* b,
                            const void* s3, uint32_t flags, const void* challenges_g2, g16_ptau_out* out,
                            g16_ptau_contribution* record);

/* The check of a .ptau (`snarkjs powersoftau verify` as arithmetic): is this the powers of SOME tau, alpha, beta, and, when
 * records are given, did this chain of contributions lead to it from the generators?  records: `count` records in order,
 * or NULL (no chain to check); challenges_g2: 3 challenge points per record (t, a, b), re-derived by the caller.  The
 * arrays of a report, in order: the file's five (G16_PTAU_*), then per record the five after-values and, three per record,
 * g1_s, g1_sx, g2_spx and the challenges: */
#define G16_PTAU_REPORT_ARRAYS 14
enum {
  G16_PTAUV_REC_TAU_G1 = 5, G16_PTAUV_REC_ALPHA_G1, G16_PTAUV_REC_BETA_G1, G16_PTAUV_REC_TAU_G2, G16_PTAUV_REC_BETA_G2, /* count */
  G16_PTAUV_G1_S, G16_PTAUV_G1_SX, G16_PTAUV_G2_SPX, G16_PTAUV_CHALLENGES                                          /* 3 count */
};
#define G16_PTAU_RELATIONS 10
enum {
  G16_PTAUV_ELEMENTS = 0, G16_PTAUV_FIRST, G16_PTAUV_TAU_G1, G16_PTAUV_TAU_G2, G16_PTAUV_ALPHA, G16_PTAUV_BETA,
  G16_PTAUV_BETA_G2, G16_PTAUV_POK, G16_PTAUV_STEP, G16_PTAUV_LAST
};
typedef struct {
  uint32_t failed;                                /* bit k set: relation k is 0; 0 = nothing fails */
  int32_t relation[G16_PTAU_RELATIONS];           /* 1 = holds, 0 = fails, -1 = not run */
  size_t first_record[2];                         /* the first record whose POK / STEP fails, (size_t)-1: none */
  size_t first_bad[G16_PTAU_REPORT_ARRAYS][3];    /* per array and check, as g16_points_audit_* */
  size_t bad_count[G16_PTAU_REPORT_ARRAYS][3];
  size_t first_infinity[G16_PTAU_REPORT_ARRAYS];  /* first (0,0) element, (size_t)-1: none */
} g16_ptau_report;
/* Write m = 2^(power+1) - 2, n = 2^power, z_i the multipliers.
 *   ELEMENTS  every element of the fourteen arrays is canonical and on its curve, the G2 ones in the order-r subgroup, none (0,0)
 *   FIRST     tauG1[0] == gen1, tauG2[0] == gen2, byte for byte
 *   TAU_G1    e(sum_{i<m} z_i tauG1[i], tauG2[1]) == e(sum_{i<m} z_i tauG1[i+1], gen2)
 *   TAU_G2    e(tauG1[1], sum_{i<n-1} z_i tauG2[i]) == e(gen1, sum_{i<n-1} z_i tauG2[i+1])
 *   ALPHA, BETA  the form of TAU_G1 over alphaTauG1 / betaTauG1, i < n - 1
 *   BETA_G2   e(betaTauG1[0], gen2) == e(gen1, betaG2)
 *   POK       per record and x in (t, a, b): e(g1_s, g2_spx) == e(g1_sx, challenge)
 *   STEP      per record: e(before, g2_spx_x) == e(after, challenge_x) for tauG1 (x = t), alphaG1 (a), betaG1 (b);
 *             e(g1_sx_x, before) == e(g1_s_x, after) for tauG2 (x = t) and betaG2 (b); record 0 steps from the generators
 *   LAST      the last record's five values are the file's tauG1[1], alphaTauG1[0], betaTauG1[0], tauG2[1], betaG2 byte for
 *             byte; count == 0: the file's five are generators
 * POK, STEP, LAST are -1 when records == NULL.  A relation is -1 when an array it reads failed ELEMENTS (FIRST, TAU_G1,
 * TAU_G2: tauG1, tauG2; ALPHA / BETA: the array and tauG2; BETA_G2: betaTauG1, betaG2; POK: g1_s, g1_sx, g2_spx, challenges;
 * STEP: those and the five record arrays; LAST: the five record arrays and the file's five).  Each sum is the one-shot MSM,
 * twice per relation over the same widened multipliers with the point pointer at offsets 0 and 1; the multipliers of the
 * three shorter arrays are the prefix of the one array; every pairing equation goes into ONE launch of the circuit audit's
 * four-pair product.  No new arithmetic.
 * multipliers: m x 16 bytes under the rules of g16_verify_batch: little-endian 128-bit integers, every one non-zero, drawn by
 * the CALLER from a CSPRNG after every input is fixed.  A zero one is G16_EINVAL and g16_last_error names its index.
 * Soundness: write tauG1[i] = a_i gen1 and tauG2[1] = T gen2.  TAU_G1 says sum z_i (T a_i - a_(i+1)) = 0: if any step
 * a_(i+1) != T a_i, a non-zero linear form in the z_i over Fr (r > 2^128), which vanishes with probability at most
 * 1/(2^128 - 1) over multipliers uniform in the non-zero 128-bit values and independent of the inputs; with FIRST (a_0 = 1)
 * tauG1[i] = T^i gen1.  TAU_G2 likewise forces tauG2[i+1] = a_1 tauG2[i] with a_1 the logarithm of tauG1[1]; its i = 0 term
 * with FIRST gives tauG2[1] = a_1 gen2, i.e. T = a_1: the two relations tie tauG1[1] and tauG2[1] to each other, so ONE tau
 * runs through both arrays.  ALPHA and BETA force alphaTauG1[i] = T^i alphaTauG1[0] and the same for beta; BETA_G2, POK,
 * STEP, LAST, FIRST are exact.  Bound 1/(2^128 - 1) per relation.
 * G16_EINVAL also: a null pointer (records may be NULL; then count must be 0); power == 0 or > 25 (the limit of
 * g16_ptau_contribute: what one writes the other can check); count >= 2^16.
 * The call changes no context state; one wait after the element passes and one at the end.  HBM: the context's staging
 * buffers grow to tauG1 (2^(power+1) x 64 B) and the widened multipliers (2^(power+1) x 32 B). */
int32_t g16_ptau_verify(g16_ctx* ctx, const g16_ptau_desc* ptau, const g16_ptau_contribution* records,
                        const void* challenges_g2, size_t count, const void* multipliers, g16_ptau_report* out);

/* ---- profiling ---------------------------------------------------------------------------------- */
/* on = 1: every kernel launch is bracketed by HIP events on the stream it is launched on; on = 2: only the
 * bucket-accumulation kernels (cheap enough to leave on inside a timed region); on = 0: off */
int32_t g16_profile_enable(g16_ctx* ctx, int32_t on);
int32_t g16_profile_reset(g16_ctx* ctx);
/* writes a JSON object {"kernel": {"calls": k, "total_ms": t}, ...} into buf (NUL-terminated) */
int32_t g16_profile_report(g16_ctx* ctx, char* buf, size_t buflen);
/* The shader clock (GHz) the chip sustained while the bucket-accumulation kernels launched since the last call ran
 * (profiling on): sum of s_memtime deltas / sum of s_memrealtime deltas over thread 0 of every workgroup.  0 if none
 * ran.  Waits for the context's work; resets the sums. */
int32_t g16_profile_clock(g16_ctx* ctx, double* ghz);

#ifdef __cplusplus
}
#endif
#endif /* G16HIP_H */
