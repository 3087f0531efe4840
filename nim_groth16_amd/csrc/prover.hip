// The per-proof launch sequence: the GPU counterpart of generateProofWithMask (reference groth16/prover.nim:215-304),
// run against a resident proving key (g16_pkey, pkey.hpp; created by pkey.hip).
//   buildABC                      prover.nim:56-73     -> spmv_binned kernel (spmv.hip; rows binned once per key)
//   computeSnarkjsScalarCoeffs /  prover.nim:158-181   -> g16_quotient_device (ntt.hip)
//   computeQuotientPointwise      prover.nim:118-148
//   5 x msmMultiThreaded          prover.nim:282-302   -> msm_device on the registered point tables
//   mask algebra (`**`, `+=`)     prover.nim:279-302   -> O(1) curve operations on the host, as in the
//                                                         reference (curves.nim:136-214); not a hot loop
// Which launches a proof makes, and in which order, is proof_plan.hpp's; run_plan below walks that list.  The one kernel
// defined here is the combine of the shards' partials.
#include "pkey.hpp"
#include "host_curve.hpp"   // the host-side O(1) curve algebra of the combine step (ec.cuh, host_ff64.hpp)

using namespace g16;

// Az | Bz | Cz for a witness (device buffers); exposed for tests of the buildABC kernel
// need_cz = false: only Az | Bz (Montgomery); the quotient forms Cz = Az * Bz while its first pass loads (ntt.cuh)
static int32_t build_abc_device(g16_ctx* ctx, const g16_pkey* k, const u256* d_wit, uint32_t wit_mont, u256* d_abc,
                                bool need_cz = true) {
  return g16_spmat_apply(ctx, k->abc, d_wit, wit_mont, d_abc, need_cz);
}

extern "C" int32_t g16_build_abc(g16_ctx* ctx, const g16_pkey* k, const void* witness, uint32_t flags, void* out_abc) {
  if (!ctx) return G16_EINVAL;
  if (!k || !witness || !out_abc || k->device != ctx->device) {
    ctx->err = "bad argument";
    return G16_EINVAL;
  }
  CTX_ENTER(ctx);
  const size_t n = size_t(1) << k->log2n;
  int32_t rc;
  if ((rc = ensure(ctx, ctx->prove, ((size_t)k->nvars + 4 * n) * 32))) return rc;
  u256* d_w = (u256*)ctx->prove.p();
  u256* d_abc = d_w + k->nvars;
  HIPCHK(ctx, hipMemcpyAsync(d_w, witness, (size_t)k->nvars * 32, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = build_abc_device(ctx, k, d_w, (flags & G16_SCALARS_MONT) ? 1u : 0u, d_abc))) return rc;
  HIPCHK(ctx, hipMemcpyAsync(out_abc, d_abc, 3 * n * 32, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return G16_OK;
}

// record of the five MSM partials of one rank: XYZZ accumulators (Montgomery), fixed order
//   [0,128) A1 | [128,256) B1 | [256,512) B2 (G2) | [512,640) H1 | [640,768) C1
static constexpr size_t PART_A = 0, PART_B1 = 128, PART_B2 = 256, PART_H = 512, PART_C = 640, PART_BYTES = G16_PARTIALS_BYTES;
static_assert(PART_C + sizeof(g1_acc) == PART_BYTES && PART_BYTES <= STAGE_O_RESULT_BYTES, "record layout");

// ---- a proof's launch sequence: the plan (proof_plan.hpp) decides, run_plan issues ------------------------------
static ProofShape proof_shape(const g16_pkey* k) {
  return ProofShape{k->w.size(), k->h.size(), k->log2n, k->liveA != nullptr, (bool)k->liveB,
                    k->C1->cfg() == k->H1->cfg(), k->b1_form};
}

// what the steps of one entry point work on
struct ProofArgs {
  const void* witness = nullptr;   // (whole proof, _begin)
  uint32_t flags = 0;
  u256* task_out = nullptr;        // _begin: the coset vectors, n Fr each
  const void *d_a1 = nullptr, *d_b1 = nullptr, *d_c1 = nullptr;   // _end: this key's slices of them
  bool qs_is_slice = false;        // _end: the H scalars lie at the start of the qs buffer, not at h_lo
  void* out_partials = nullptr;
};

static int32_t run_plan(g16_ctx* ctx, const g16_pkey* k, ProofEntry entry, uint32_t task_mask, bool host_sync,
                        const ProofArgs& a) {
  ProofPlan plan;
  if (!proof_plan_build(plan, g16_env(), entry, task_mask, host_sync, proof_shape(k))) {
    ctx->err = "proof launch plan exceeds its capacity";
    return G16_EINVAL;
  }
  const size_t n = size_t(1) << k->log2n, nw = k->w.size(), nh = k->h.size();
  int32_t rc;
  if ((rc = ensure(ctx, ctx->prove, ((size_t)k->nvars + 4 * n) * 32))) return rc;
  if ((rc = ensure_stage_o(ctx))) return rc;
  u256* const d_w = (u256*)ctx->prove.p();   // per-proof scalars: witness | Az | Bz | Cz | qs
  u256* const d_abc = d_w + k->nvars;
  u256* const d_qs = d_abc + 3 * n;
  char* const slots = stage_o_at(ctx, STAGE_O_RESULT);
  const u256* const d_wr = d_w + k->w.lo;
  const u256* const d_qs_slice = a.qs_is_slice ? d_qs : d_qs + k->h.lo;   // the H scalars of [h_lo, h_hi), Montgomery
  const uint32_t wit_mont = (a.flags & G16_SCALARS_MONT) ? 1u : 0u;
  g16_ctx::MsmLane* L = ctx->lane;
  // the five MSMs (ProofRun order): arrangement, workspace, tables, slot of the record
  const g16_points* const sets[RUN_COUNT] = {k->A1, k->B1, k->C1, k->B2, k->H1};
  g16_msm_run runs[RUN_COUNT] = {
      {&ctx->sort[plan.sort_a], &L[0].acc, k->A1->d_tables.get(), nullptr, slots + PART_A, nullptr},
      // (B1_EMPTY: no table -- msm_accum leaves infinity in every bucket and the tail kernels take their early-outs)
      {&ctx->sort[plan.sort_b1], &L[2].acc, k->b1_form == B1_EMPTY ? nullptr : k->B1->d_tables.get(), nullptr,
       slots + PART_B1, nullptr},
      {&ctx->sort[SORT_W], &L[3].acc, k->C1->d_tables.get(), nullptr, slots + PART_C, nullptr},
      {&ctx->sort[plan.sort_b], &L[1].acc, k->B2->d_tables.get(), nullptr, slots + PART_B2, nullptr},
      {&ctx->sort[SORT_H], &L[4].acc, k->H1->d_tables.get(), nullptr, slots + PART_H, nullptr}};
  // A DELTA key with a handful of live differences (b1_sparse_run, decided when the key was made): the B1 job forms its
  // bucket sums from the witness values of those wires alone.  It keeps its place in the plan -- same step, same stream,
  // same waits -- and takes from the witness arrangement only the launch parameters, which every job of the witness shares.
  g16_msm_sparse b1_sparse{d_wr, nullptr, k->b1_nlive, k->b1_sparse.get()};
  if (k->b1_sparse) {
    b1_sparse.d_wires = k->b1_sparse.get() + g16_pkey::B1_VIEW_WORDS;
    runs[RUN_B1].sparse = &b1_sparse;
  }
  auto event = [&](int e) { return e == EV_NONE ? nullptr : e < EV_COUNT ? ctx->ev[e].get() : L[e - EV_DONE0].done.get(); };
  for (int i = 0; i < plan.count; ++i) {
    const ProofStep& s = plan.steps[i];
    rc = G16_OK;
    hipStream_t st = s.stream == PS_MAIN ? ctx->stream : L[s.stream].stream.get();
    switch (s.op) {
      case OP_UPLOAD:
        HIPCHK(ctx, hipMemcpyAsync(d_w, a.witness, (size_t)k->nvars * 32,
                                   (a.flags & G16_SCALARS_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipMemsetAsync(slots, 0, PART_BYTES, st));   // empty range -> XYZZ infinity (all zero)
        break;
      case OP_WAIT: HIPCHK(ctx, hipStreamWaitEvent(st, event(s.a), 0)); break;
      case OP_RECORD: HIPCHK(ctx, hipEventRecord(event(s.a), st)); break;
      case OP_SORT_W:
        ctx->sort[s.a].narrow_tail = plan.narrow_tail;
        rc = g16_msm_sort(ctx, st, d_wr, wit_mont ? G16_SCALARS_MONT : 0u, nw, sets[s.c]->cfg(), ctx->sort[s.a],
                          s.b == 0 ? nullptr : s.b == 1 ? k->liveA : k->liveB.get());
        break;
      case OP_SORT_H:
        ctx->sort[SORT_H].narrow_tail = plan.narrow_tail;
        rc = g16_msm_sort(ctx, st, d_qs_slice, G16_SCALARS_MONT, nh, k->H1->cfg(), ctx->sort[SORT_H]);
        break;
      case OP_BUILD_ABC: rc = build_abc_device(ctx, k, d_w, wit_mont, d_abc, s.a != 0); break;
      case OP_QUOTIENT:
        rc = g16_quotient_device(ctx, d_abc, d_abc + n, d_abc + 2 * n, k->log2n, (int)k->flavour, d_qs, s.a);
        break;
      case OP_COSET: {   // (the outputs of the set bits of task_mask lie one after the other)
        const int at = __builtin_popcount(task_mask & ((1u << s.a) - 1));
        rc = g16_coset_pipeline_device(ctx, d_abc + s.a * n, k->log2n, a.task_out + at * n);
        break;
      }
      case OP_POINTWISE: rc = g16_abc_pointwise_device(ctx, a.d_a1, a.d_b1, a.d_c1, nh, d_qs); break;
      case OP_MSM:
        runs[RUN_H].init_partial = s.e ? g16_msm_partial_ptr(L[3].acc) : nullptr;   // (read by H's step alone)
        rc = g16_msm_batch(ctx, st, s.a == RUN_B2 ? 2 : 1, &runs[s.a], s.b, s.c, event(s.d));
        break;
      case OP_COPY_OUT:
        HIPCHK(ctx, hipMemcpyAsync(a.out_partials, slots, PART_BYTES,
                                   (a.flags & G16_OUT_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
        break;
      case OP_HOST_SYNC: HIPCHK(ctx, hipStreamSynchronize(st)); break;
    }
    if (rc) return rc;
  }
  return G16_OK;
}

extern "C" int32_t g16_prove_partials(g16_ctx* ctx, const g16_pkey* k, const void* witness, uint32_t flags,
                                      void* out_partials) {
  if (!ctx) return G16_EINVAL;
  if (!k || !witness || !out_partials || k->device != ctx->device) {
    ctx->err = "bad argument";
    return G16_EINVAL;
  }
  CTX_ENTER(ctx);
  ProofArgs a;
  a.witness = witness, a.flags = flags, a.out_partials = out_partials;
  // G16_NO_HOST_SYNC (device output only): the record is complete in stream order; the caller's next operation on
  // the context's stream (an all-gather enqueued on it, g16_prove_combine) is ordered behind it without a host wait
  const bool host_sync = !((flags & G16_NO_HOST_SYNC) && (flags & G16_OUT_DEVICE));
  const int32_t rc = run_plan(ctx, k, PROOF_WHOLE, 0, host_sync, a);
  // an error exit may leave work queued on the lane streams (e.g. a failed allocation after the witness MSMs were
  // launched): drain all of them before returning, so that the caller -- or the next call's ensure() -- can never
  // free a buffer a lane kernel is still reading
  if (rc != G16_OK) ctx_quiesce(ctx);
  return rc;
}

// ---- sharded proof with a task-parallel quotient ------------------------------------------------------------
// The reference runs the three coset pipelines of computeSnarkjsScalarCoeffs as three tasks (prover.nim:167-169).
// Across GPUs each pipeline lives on ONE rank: _begin launches this rank's witness MSMs and computes the pipelines
// named by task_mask (bit 0: A, bit 1: B, bit 2: C) into d_task_out (n Fr per set bit, ascending); the caller
// scatters the [h_lo, h_hi) slices of the three coset vectors to their ranks (nim_groth16_amd/distributed.py: three
// scatters of 32 n / G bytes per destination) while the MSM lanes keep computing; _end forms this rank's H scalars
// A1*B1 - C1 from the received slices (prover.nim:175-176), runs the H MSM over them and hands out the partials.
extern "C" int32_t g16_prove_partials_begin(g16_ctx* ctx, const g16_pkey* k, const void* witness, uint32_t flags,
                                            uint32_t task_mask, void* d_task_out) {
  if (!ctx) return G16_EINVAL;
  if (!k || !witness || k->device != ctx->device || task_mask > 7 || (task_mask && !d_task_out)) {
    ctx->err = "bad argument";
    return G16_EINVAL;
  }
  if (k->flavour != G16_FLAVOUR_SNARKJS) {
    ctx->err = "the task-parallel quotient serves snarkjs-flavour keys (JensGroth needs a 7th transform of the whole "
               "vector: use g16_prove_partials)";
    return G16_EINVAL;
  }
  CTX_ENTER(ctx);
  ProofArgs a;
  a.witness = witness, a.flags = flags, a.task_out = (u256*)d_task_out;
  const int32_t rc = run_plan(ctx, k, PROOF_BEGIN, task_mask, !(flags & G16_NO_HOST_SYNC), a);
  if (rc != G16_OK) {
    ctx_quiesce(ctx);
    return rc;
  }
  ctx->shard_begun = k;
  return G16_OK;
}

extern "C" int32_t g16_prove_partials_end(g16_ctx* ctx, const g16_pkey* k, const void* d_a1, const void* d_b1,
                                          const void* d_c1, uint32_t flags, void* out_partials) {
  if (!ctx) return G16_EINVAL;
  const size_t nh = k ? k->h.size() : 0;
  if (!k || !out_partials || k->device != ctx->device || (nh && (!d_a1 || !d_b1 || !d_c1))) {
    ctx->err = "bad argument";
    return G16_EINVAL;
  }
  if (ctx->shard_begun != k) {
    ctx->err = "g16_prove_partials_end without a matching g16_prove_partials_begin on this context";
    return G16_EINVAL;
  }
  CTX_ENTER_KEEP(ctx);
  ctx->shard_begun = nullptr;
  ProofArgs a;
  a.flags = flags, a.d_a1 = d_a1, a.d_b1 = d_b1, a.d_c1 = d_c1, a.qs_is_slice = true, a.out_partials = out_partials;
  const int32_t rc = run_plan(ctx, k, PROOF_END, 0, !((flags & G16_NO_HOST_SYNC) && (flags & G16_OUT_DEVICE)), a);
  if (rc != G16_OK) ctx_quiesce(ctx);
  return rc;
}

// one workgroup per MSM: res = sum over ranks of that MSM's partial, then canonical affine
// (`res += sync pending[k]`, msm.nim:117-119, across GPUs instead of threads)
// fold_b1: the B1 slots hold MSM(w, B1 - A1) (a key with pointsB1 folded into pointsA1): B1 = the A1 slots + the B1 slots
static __global__ void prove_combine_kernel(const unsigned char* __restrict__ gathered, uint32_t count, uint32_t fold_b1,
                                            unsigned char* __restrict__ out) {
  if (threadIdx.x != 0) return;
  const uint32_t b = blockIdx.x;
  if (b == 2) {
    g2_acc r = G2::acc_inf();
    for (uint32_t i = 0; i < count; ++i) G2::add(r, *(const g2_acc*)(gathered + (size_t)i * PART_BYTES + PART_B2));
    *(g2_aff*)(out + 128) = G2::to_affine(r);
  } else {
    const size_t src = b == 0 ? PART_A : b == 1 ? PART_B1 : b == 3 ? PART_H : PART_C;
    const size_t dst = b == 0 ? 0 : b == 1 ? 64 : b == 3 ? 256 : 320;
    g1_acc r = G1::acc_inf();
    for (uint32_t i = 0; i < count; ++i) G1::add(r, *(const g1_acc*)(gathered + (size_t)i * PART_BYTES + src));
    if (b == 1 && fold_b1)
      for (uint32_t i = 0; i < count; ++i) G1::add(r, *(const g1_acc*)(gathered + (size_t)i * PART_BYTES + PART_A));
    *(g1_aff*)(out + dst) = G1::to_affine(r);
  }
}

// g16_prove_combine in two halves, shared with the prover pool (pool.hip).
// Enqueue half: stage copy + prove_combine_kernel on the context's main stream, the host algebra that needs only the
// mask and the key, then the copy of the five affine MSM sums (384 bytes) into `res_host` and, if `done` is given, an
// event behind it.  Into pageable memory the copy makes the host wait for the stream; into pinned memory it does not.
static_assert(sizeof(CombineRes) == G16_COMBINE_RES_BYTES, "slot layout");
static_assert(sizeof(CombinePre) == sizeof(g16_combine_pre), "g16_combine_pre layout");

int32_t g16_combine_enqueue(g16_ctx* ctx, const g16_pkey* k, const void* partials, size_t count, uint32_t flags,
                            const void* mask_r, const void* mask_s, void* res_host, hipEvent_t done,
                            g16_combine_pre* pre_out) {
  int32_t rc;
  if ((rc = ensure(ctx, ctx->stage_p, count * PART_BYTES))) return rc;
  if ((rc = ensure_stage_o(ctx))) return rc;
  HIPCHK(ctx, hipMemcpyAsync(ctx->stage_p.p(), partials, count * PART_BYTES,
                             (flags & G16_SCALARS_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                             ctx->stream));
  unsigned char* d_res = (unsigned char*)stage_o_at(ctx, STAGE_O_COMBINE);
  KLAUNCH(ctx, "prove_combine", prove_combine_kernel, 5, 64, 0, (const unsigned char*)ctx->stage_p.p(), (uint32_t)count,
          k->b1_form != B1_PLAIN ? 1u : 0u, d_res);

  // Everything that depends on the mask and the key alone is computed while the GPU works -- in g16_prove that is the
  // whole proof, which is enqueued without a host wait (host_curve.hpp: host_combine_pre)
  u256 r = Fr::zero(), s = Fr::zero();
  if (mask_r) memcpy(&r, mask_r, 32);
  if (mask_s) memcpy(&s, mask_s, 32);
  const CombinePre pre = host_combine_pre(k->alpha1, k->beta1, k->delta1, k->beta2, k->delta2, r, s);
  memcpy(pre_out, &pre, sizeof pre);
  // (a copy into pageable host memory makes the host wait for the stream: it comes AFTER the host arithmetic above)
  HIPCHK(ctx, hipMemcpyAsync(res_host, d_res, sizeof(CombineRes), hipMemcpyDeviceToHost, ctx->stream));
  if (done) HIPCHK(ctx, hipEventRecord(done, ctx->stream));
  return G16_OK;
}

// Finish half: what needs the MSM results -- three additions and ONE joint double-scalar multiplication.  `res_host`
// must be complete (the stream or the enqueue half's event has passed the copy).
void g16_combine_finish(const g16_combine_pre* pre_in, const void* res_host, g16_proof* out) {
  CombinePre pre;
  CombineRes res;
  memcpy(&pre, pre_in, sizeof pre);
  memcpy(&res, res_host, sizeof res);
  g1_aff pi_a, pi_c;
  g2_aff pi_b;
  host_combine_finish(pre, res, pi_a, pi_b, pi_c);
  memcpy(out->pi_a, &pi_a, 64);
  memcpy(out->pi_b, &pi_b, 128);
  memcpy(out->pi_c, &pi_c, 64);
}

extern "C" int32_t g16_prove_combine(g16_ctx* ctx, const g16_pkey* k, const void* partials, size_t count,
                                     uint32_t flags, const void* mask_r, const void* mask_s, g16_proof* out) {
  if (!ctx) return G16_EINVAL;
  if (!k || !partials || !out || k->device != ctx->device || count == 0 || count > 1024) {
    ctx->err = "bad argument";
    return G16_EINVAL;
  }
  CTX_ENTER(ctx);
  int32_t rc;
  CombineRes res;
  g16_combine_pre pre;
  if ((rc = g16_combine_enqueue(ctx, k, partials, count, flags, mask_r, mask_s, &res, nullptr, &pre))) return rc;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  g16_combine_finish(&pre, &res, out);
  return G16_OK;
}

extern "C" int32_t g16_prove(g16_ctx* ctx, const g16_pkey* k, const void* witness, uint32_t flags, const void* mask_r,
                             const void* mask_s, g16_proof* out) {
  if (!ctx) return G16_EINVAL;
  if (!k || !witness || !out || k->device != ctx->device) {
    ctx->err = "bad argument";
    return G16_EINVAL;
  }
  if (k->shard_count != 1) {
    ctx->err = "g16_prove needs an unsharded key; use g16_prove_partials + g16_prove_combine";
    return G16_EINVAL;
  }
  CTX_ENTER(ctx);   // before the first allocation: a fresh host thread's current device is 0, not the context's
  int32_t rc;
  if ((rc = ensure_stage_o(ctx))) return rc;
  if ((rc = ensure(ctx, ctx->stage_s, PART_BYTES))) return rc;
  // partials stay in HBM (stage_s is free again once the witness has been copied into the prove buffer)
  unsigned char* d_part = (unsigned char*)ctx->stage_s.p();
  // no host wait here: the combine's copy and kernel are ordered behind the record on the main stream, and its
  // mask-only host arithmetic (~0.3 ms) then overlaps the whole proof instead of following it
  if ((rc = g16_prove_partials(ctx, k, witness, flags | G16_OUT_DEVICE | G16_NO_HOST_SYNC, d_part))) return rc;
  rc = g16_prove_combine(ctx, k, d_part, 1, G16_SCALARS_DEVICE, mask_r, mask_s, out);
  if (rc != G16_OK) ctx_quiesce(ctx);   // a failed combine may leave the lanes running
  return rc;
}

// quotient alone, host pointers (replaces computeSnarkjsScalarCoeffs / computeQuotientPointwise)
extern "C" int32_t g16_quotient(g16_ctx* ctx, const void* Az, const void* Bz, const void* Cz, uint32_t log2n,
                                uint32_t flavour, void* out) {
  if (!ctx) return G16_EINVAL;
  if (!Az || !Bz || !Cz || !out || log2n > 27 || flavour > 1) {
    ctx->err = "bad argument";
    return G16_EINVAL;
  }
  CTX_ENTER(ctx);
  const size_t n = size_t(1) << log2n;
  int32_t rc;
  if ((rc = ensure(ctx, ctx->prove, 4 * n * 32))) return rc;
  u256* d = (u256*)ctx->prove.p();
  HIPCHK(ctx, hipMemcpyAsync(d, Az, n * 32, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(d + n, Bz, n * 32, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(d + 2 * n, Cz, n * 32, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = g16_quotient_device(ctx, d, d + n, d + 2 * n, log2n, (int)flavour, d + 3 * n))) return rc;
  HIPCHK(ctx, hipMemcpyAsync(out, d + 3 * n, n * 32, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return G16_OK;
}
extern "C" int32_t g16_quotient_dev(g16_ctx* ctx, const void* d_Az, const void* d_Bz, const void* d_Cz, uint32_t log2n,
                                    uint32_t flavour, void* d_out) {
  if (!ctx) return G16_EINVAL;
  if (!d_Az || !d_Bz || !d_Cz || !d_out || log2n > 27 || flavour > 1) {
    ctx->err = "bad argument";
    return G16_EINVAL;
  }
  CTX_ENTER(ctx);
  return g16_quotient_device(ctx, d_Az, d_Bz, d_Cz, log2n, (int)flavour, d_out);
}
