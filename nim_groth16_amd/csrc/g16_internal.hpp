// Internal declarations shared by the translation units of libg16hip.so (not part of the C ABI).
#pragma once
#include "../../include/g16hip.h"

#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>


#include "g16_env.hpp"
#include "hip_owners.hpp"
#include "msm_params.hpp"
#include "circuit_setup_plan.hpp"
#include "msm_plan.hpp"
#include "proof_plan.hpp"

const G16Env& g16_env();   // g16hip.hip: the knobs of this process

struct ProfEntry {
  const char* name;
  Event e0, e1;
};

// Members release themselves when g16_ctx_destroy deletes the context, in reverse order of declaration; the order
// among them does not matter because g16_ctx_destroy has made the device current and drained every stream first.
struct g16_ctx {
  int device = 0;
  hipStream_t stream = nullptr;   // the main stream: own_stream's, or the caller's (g16_ctx_set_stream; never destroyed here)
  Stream own_stream;              // empty while the caller's stream is in use
  std::string err;
  // growable device buffers (ensure())
  struct Buf {
    DevMem<> mem;
    size_t bytes = 0;
    void* p() const { return mem.get(); }
  };
  // MSM workspaces.  A "sort" is the bucket arrangement of ONE scalar vector (shared by every MSM that
  // uses those scalars: the witness feeds A1, B1, B2 and C1, prover.nim:282-302); a "lane" is one
  // accumulate/reduce pipeline with its own stream so that independent MSMs overlap.
  struct MsmSort {
    Buf buf;
    g16::MsmParams P;
    bool narrow_tail = false;   // reduce2 geometry: an input of msm_tail_plan, msm_plan.hpp (set by the prover's lanes: throughput)
    uint32_t *count = nullptr, *cursor = nullptr, *offset = nullptr, *xoff = nullptr, *heavy = nullptr,
             *info = nullptr, *entries = nullptr, *perm = nullptr, *ghist = nullptr, *blk_base = nullptr, *tile_hist = nullptr;
    uint2* tmp = nullptr;
    uint32_t* slice_hist = nullptr;
    uint2* tiles2 = nullptr;
    uint2* tiles = nullptr;
    uint2* xseg = nullptr;
  };
  struct MsmLane {
    Stream stream;
    Event done;
    Buf acc;
  };
  MsmSort sort[4];   // 0: witness (all pairs)  1: H scalars  2: witness, A1's live pairs  3: witness, B1/B2's live pairs
  MsmLane lane[5];
  Event ev[g16::EV_COUNT];   // the cross-stream edges of a proof (ProofEvent, proof_plan.hpp)
  Buf stage_s;   // staged scalars (host-pointer API)
  Buf stage_p;   // staged points
  Buf stage_p29; // the same points as reduced-radix entries (one-shot MSMs; registered sets keep their own tables)
  Buf stage_o;   // result slot (STAGE_O_*, below)
  Buf ntt_tw;    // twiddle table
  Buf ntt_tmp;   // ping-pong buffers
  Buf coset[2];  // eta^(+-i)/n tables (ntt_make_coset_table)
  Buf quot;      // 6n work area of the quotient pipeline
  Buf prove;     // per-proof scalars: witness, Az|Bz|Cz, qs
  Buf fb_table[2];  // fixed-base tables of gen1 / gen2
  bool fb_ready[2] = {false, false};
  DevMem<unsigned long long> clk_buf;   // {sum d_memtime, sum d_memrealtime} of the accumulate kernels (g16_profile_clock)
  const void* shard_begun = nullptr;   // key of a g16_prove_partials_begin that still awaits its _end
  uint32_t tw_log2n = 0xffffffffu;
  uint32_t coset_log2n[2] = {0xffffffffu, 0xffffffffu};
  // profiling
  bool profiling = false;
  bool prof_accum_only = false;   // g16_profile_enable(ctx, 2): only the bucket-accumulation kernels
  std::vector<ProfEntry> prof;
  std::vector<Event> free_events;
};

// The one way a HIP call fails in the host layer: "<call>: <reason>" goes to the error slot the caller will ask
// (g16_last_error, or through it g16_group_last_error / g16_prover_last_error), out-of-memory maps to G16_ENOMEM and
// everything else to G16_EHIP, and HIP's sticky last error is cleared so that it does not surface in the caller's next,
// unrelated call.
inline int32_t g16_hip_check(std::string& err, const char* call, hipError_t e) {
  if (e == hipSuccess) return G16_OK;
  err = std::string(call) + ": " + hipGetErrorString(e);
  (void)hipGetLastError();
  return e == hipErrorOutOfMemory ? G16_ENOMEM : G16_EHIP;
}
#define HIPCHK(ctx, call)                                                          \
  do {                                                                             \
    if (int32_t hiprc__ = g16_hip_check((ctx)->err, #call, (call))) return hiprc__; \
  } while (0)

// waits for everything this context has queued: the main stream AND the five MSM lane streams.  Called before a
// workspace buffer is freed or regrown, on every error exit of a multi-stream launch sequence and at teardown, so
// that no lane kernel can still be reading a buffer that is about to go away.
inline void ctx_quiesce(g16_ctx* ctx) {
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  for (auto& l : ctx->lane)
    if (l.stream) (void)hipStreamSynchronize(l.stream.get());
}
// for the temporaries of one call: declared AFTER the owners of the call's scratch buffers, it drains the stream that
// uses them on every exit, before they are freed
struct SyncOnExit {
  hipStream_t stream;
  ~SyncOnExit() { (void)hipStreamSynchronize(stream); }
};

// Entry protocol of every context-taking C-ABI function.
//  * The calling thread's current HIP device becomes the context's: allocations, event creation and launches bind to
//    the CURRENT device, and a host thread starts on device 0 -- a context of GPU 3 used from a fresh worker thread
//    would otherwise allocate its workspaces on GPU 0.
//  * A g16_prove_partials_begin whose _end never came (the caller's exchange failed, or it simply moved on) still has
//    four witness lanes reading the sort and per-proof buffers: any other compute call on the context first drains
//    them and cancels the pending proof (its _end then returns G16_EINVAL).  `keep_shard`: calls that do not touch
//    the workspaces (_end itself, synchronize, the profiling getters).
inline int32_t ctx_enter(g16_ctx* ctx, bool keep_shard = false) {
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (ctx->shard_begun && !keep_shard) {
    ctx_quiesce(ctx);
    ctx->shard_begun = nullptr;
  }
  return G16_OK;
}
#define CTX_ENTER(ctx)                              \
  do {                                              \
    if (int32_t rc__ = ctx_enter(ctx)) return rc__; \
  } while (0)
#define CTX_ENTER_KEEP(ctx)                               \
  do {                                                    \
    if (int32_t rc__ = ctx_enter(ctx, true)) return rc__; \
  } while (0)

inline int32_t ensure(g16_ctx* ctx, g16_ctx::Buf& b, size_t bytes) {
  if (b.bytes >= bytes) return G16_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));   // hipMalloc binds to the calling thread's current device
  if (b.mem) {
    ctx_quiesce(ctx);
    b.mem.reset();
    b.bytes = 0;
  }
  size_t want = bytes + bytes / 8 + 4096;
  HIPCHK(ctx, dev_alloc(b.mem, want));
  b.bytes = want;
  return G16_OK;
}

// ---- stage_o: the result slot of a context ------------------------------------------------------------------------------
// One small buffer, laid out once.  [0, RESULT_BYTES): the result of the call in progress -- a proof's partials record
// (G16_PARTIALS_BYTES), the sum of a one-shot MSM, the counts of an audit; then the counter words of counted_launch;
// then the five affine sums the combine kernel writes, which a proof's next record must not overwrite before they
// have been copied out.
#define G16_COMBINE_RES_BYTES 384   // the five affine MSM sums A1 | B1 | B2 | H1 | C1 the combine kernel writes
constexpr size_t STAGE_O_RESULT = 0, STAGE_O_RESULT_BYTES = G16_PARTIALS_BYTES;
constexpr size_t STAGE_O_COUNTERS = STAGE_O_RESULT + STAGE_O_RESULT_BYTES, STAGE_O_COUNTER_WORDS = 2;
constexpr size_t STAGE_O_COMBINE = 1024;
constexpr size_t STAGE_O_BYTES = 2048;
static_assert(STAGE_O_COUNTERS % 4 == 0 && STAGE_O_COUNTERS + 4 * STAGE_O_COUNTER_WORDS <= STAGE_O_COMBINE &&
                  STAGE_O_COMBINE % 128 == 0 && STAGE_O_COMBINE + G16_COMBINE_RES_BYTES <= STAGE_O_BYTES,
              "the pieces of stage_o overlap or do not fit");
inline int32_t ensure_stage_o(g16_ctx* ctx) { return ensure(ctx, ctx->stage_o, STAGE_O_BYTES); }
inline char* stage_o_at(g16_ctx* ctx, size_t offset) { return (char*)ctx->stage_o.p() + offset; }

// The one way the host reads a count back from a kernel: `nwords` (<= STAGE_O_COUNTER_WORDS) device words are filled
// with the byte `fill`, `launch(d_words)` queues on the main stream whatever updates them (an int32_t code: nonzero
// ends the call), then the words are copied into `words` and the stream is drained.
template <class Launch>
inline int32_t counted_launch(g16_ctx* ctx, int fill, uint32_t* words, size_t nwords, Launch&& launch) {
  if (int32_t rc = ensure_stage_o(ctx)) return rc;
  uint32_t* d_words = (uint32_t*)stage_o_at(ctx, STAGE_O_COUNTERS);
  HIPCHK(ctx, hipMemsetAsync(d_words, fill, 4 * nwords, ctx->stream));
  if (int32_t rc = launch(d_words)) return rc;
  HIPCHK(ctx, hipMemcpyAsync(words, d_words, 4 * nwords, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return G16_OK;
}

// ---- profiling helpers ----------------------------------------------------------------------------
struct ProfScope {
  g16_ctx* ctx;
  bool on;
  ProfEntry e;
  hipStream_t st;
  ProfScope(g16_ctx* c, const char* name, hipStream_t stream = nullptr)
      : ctx(c), on(c->profiling && (!c->prof_accum_only || strncmp(name, "msm_accum", 9) == 0)),
        st(stream ? stream : c->stream) {
    if (!on) return;
    e.name = name;
    auto get = [&](Event& ev) {
      if (!ctx->free_events.empty()) {
        ev = std::move(ctx->free_events.back());
        ctx->free_events.pop_back();
      } else {
        (void)event_create(ev, hipEventDefault);
      }
    };
    get(e.e0);
    get(e.e1);
    (void)hipEventRecord(e.e0.get(), st);
  }
  ~ProfScope() {
    if (!on) return;
    (void)hipEventRecord(e.e1.get(), st);
    ctx->prof.push_back(std::move(e));
  }
};
#define KLAUNCH_ON(ctx, stream_, name, kernel, grid, block, shmem, ...)                        \
  do {                                                                                         \
    ProfScope ps__(ctx, name, stream_);                                                        \
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), shmem, stream_, __VA_ARGS__);          \
  } while (0)
#define KLAUNCH(ctx, name, kernel, grid, block, shmem, ...) \
  KLAUNCH_ON(ctx, (ctx)->stream, name, kernel, grid, block, shmem, __VA_ARGS__)


// ---- MSM: the group-agnostic surface (msm_sort.hip unless noted) -------------------------------------
// device-resident point set with precomputed window tables.  Immutable after registration and tied to a DEVICE,
// not to the context that created it: every context of that device may run MSMs against it concurrently (the
// in-flight proofs of one GPU share one key), and it may be released before or after any context.
struct g16_points {
  int device = 0;
  int group = 1;          // 1: G1 (64-byte points), 2: G2 (128-byte points)
  size_t n = 0;
  uint32_t c = 0, nwin = 0;
  uint32_t mtab = 1;         // multiplier tables per window: 1, or 2 = {1, 2} with the class bucket set (msm.cuh)
  uint32_t stride = 1;       // a table for every stride-th window: 1, or >= 2 for a lean set (msm_plan.hpp; mtab == 1)
  uint32_t ntables() const { return mtab * ((nwin + stride - 1) / stride); }
  uint32_t cfg() const { return g16::msm_table_cfg(c, mtab, stride); }   // the `table_cfg` of g16_msm_sort / msm_device
  DevMem<> d_tables;         // ntables() * n affine points: [m][j][i] = 2^(c stride j + m) P_i
  DevMem<uint32_t> d_live;      // bitmap: bit i set <=> point i is not (0,0); ceil(n/32) words
  size_t n_inf = 0;             // points at infinity in the set
};
// the live bitmap of a registered set if it holds enough (0,0) points for its own entry lists to pay (points_sparse,
// key_plan.hpp; g16hip.hip)
const uint32_t* g16_points_live_if_sparse(const g16_points* p);
// the two halves of an MSM: (1) arrange one scalar vector into buckets, (2) accumulate + reduce a point set
// against that arrangement.  Several point sets may share one sort (same scalars, same n, same c).
// table_c == 0: plain point arrays; else g16_points::cfg() of the registered sets that will run against the sort
// d_live (optional): bitmap over the n pairs; pairs with a cleared bit get no entries (point sets with (0,0) points)
int32_t g16_msm_sort(g16_ctx* ctx, hipStream_t stream, const void* d_scalars, uint32_t flags, size_t n,
                     uint32_t table_c, g16_ctx::MsmSort& sort, const uint32_t* d_live = nullptr);
// Several MSMs of one group as ONE launch sequence on one stream (every stage kernel takes blockIdx.y = job): the jobs
// must share the launch parameters (same n, same window: e.g. the G1 MSMs of a proof that consume the witness).
//   n_accum jobs are accumulated (+ split buckets combined); the first n_tail <= n_accum of them are reduced and folded
//   init_partial: the bucket sums (after `after_heavy`) of another job over the same bucket set, to continue from
//   after_heavy (optional): recorded on the stream once every job's bucket sums are final
// What a sparse run reads in place of an arrangement (msm_sparse_accum, msm.cuh; G1 only): the set holds live points at
// the `nlive` ascending pair indices d_wires alone, and its bucket sums are formed from those pairs' scalars.
struct g16_msm_sparse {
  const void* d_scalars;     // the scalars the run's `sort` arranged (same n, same form: the sort's MsmParams hold both)
  const uint32_t* d_wires;   // device; never null
  uint32_t nlive;
  const uint32_t* d_info;    // >= 3 zero words on the device: the job's view of the arrangement's counters (MsmJob::info)
};
struct g16_msm_run {
  const g16_ctx::MsmSort* sort;   // (a sparse run takes its launch parameters from it and nothing else)
  g16_ctx::Buf* acc;            // workspace of this job (bucket sums first: see g16_msm_partial_ptr)
  const void* d_points;         // the tables of a registered set, or reduced-radix entries (to29_device); null = a set
                                // that is infinity throughout: msm_accum (msm.cuh) then writes infinity to every bucket
                                // sum and reads no entry.  It does NOT carry `init_partial` over in that case, so a run
                                // with a null table must have a null init_partial (g16_msm_batch refuses the pair)
  void* d_out_aff;              // either may be null
  void* d_out_acc;
  const void* init_partial;
  const g16_msm_sparse* sparse = nullptr;   // the accumulation is the sparse run (needs a table, takes no init_partial)
};
// `group` (1 / 2) is data to the prover, which walks its MSMs in a table: the one run-time choice of the curve below the C ABI
int32_t g16_msm_batch(g16_ctx* ctx, hipStream_t stream, int group, const g16_msm_run* runs, int n_accum, int n_tail,
                      hipEvent_t after_heavy);
inline const void* g16_msm_partial_ptr(const g16_ctx::Buf& acc) { return acc.p(); }
int32_t g16_lanes_init(g16_ctx* ctx);   // g16hip.hip
// d_out = d_a | d_b over bitmaps of n bits; *d_n_dead (device u32, zeroed by the caller) += bits clear in
// the union (msm_g1_misc.hip)
int32_t g16_bitmap_or_device(g16_ctx* ctx, uint32_t* d_out, const uint32_t* d_a, const uint32_t* d_b, size_t n,
                             uint32_t* d_n_dead);

// ---- MSM: per curve, C = g16::G1 / g16::G2 (ec.cuh) ---------------------------------------------------
// Declarations only.  msm_device is defined in msm_sort.hip; the bodies of the others are in msm_stage.cuh and are
// explicitly instantiated, with their kernels, in msm_g{1,2}_{accum,reduce1,reduce2,misc}.hip.  A translation unit
// that includes only this header can call them and instantiates no kernel of its own.
namespace g16 {
template <class C>
struct MsmBatch;   // msm.cuh: up to MSM_BATCH_MAX jobs that share the launch parameters P
}
// one complete MSM on the context's main stream
// table_c == 0: d_points = n affine points; else g16_points::cfg() and d_points = the tables of that registered set
template <class C>
int32_t msm_device(g16_ctx* ctx, const void* d_scalars, uint32_t flags, const void* d_points, size_t n, void* d_out_aff,
                   void* d_out_acc, uint32_t table_c, const uint32_t* d_live = nullptr);
// the stages of phase 2 over the first `ny` jobs of a batch
template <class C>
int32_t stage_accum(g16_ctx* ctx, hipStream_t st, const g16::MsmParams& P, const g16::MsmBatch<C>& B, uint32_t ny);
// the sparse run of one job (G1; msm_g1_misc.hip).  `own_entry`: the launch is the accumulate stage of its batch and goes
// into the profile under that stage's name; otherwise it rides behind the stage's msm_accum launch, unlisted
template <class C>
int32_t stage_accum_sparse(g16_ctx* ctx, hipStream_t st, const g16::MsmParams& P, const g16_msm_sparse& sp,
                           const void* d_points, void* d_partial, bool own_entry);
// T: the tail plan of the batch (msm_plan.hpp), built once by msm_batch
template <class C>
int32_t stage_heavy(g16_ctx* ctx, hipStream_t st, const g16::MsmParams& P, const g16::MsmTailPlan& T,
                    const g16::MsmBatch<C>& B, uint32_t ny);
template <class C>
int32_t stage_reduce1(g16_ctx* ctx, hipStream_t st, const g16::MsmParams& P, const g16::MsmTailPlan& T,
                      const g16::MsmBatch<C>& B, uint32_t ny);
template <class C>
int32_t stage_reduce2_fold(g16_ctx* ctx, hipStream_t st, const g16::MsmParams& P, const g16::MsmTailPlan& T,
                           const g16::MsmBatch<C>& B, uint32_t ny);
// reference-layout points -> reduced-radix entries (one-shot MSMs) / window tables (registered sets)
template <class C>
int32_t to29_device(g16_ctx* ctx, hipStream_t st, const void* d_points, size_t n, void* d_out);
template <class C>
int32_t precompute_device(g16_ctx* ctx, const void* d_points, size_t n, uint32_t c, uint32_t mtab, uint32_t stride,
                          void* d_tables);
// d_out[i] = d_scalars[i] * generator; d_table: 32*255 points, built first unless table_ready
template <class C>
int32_t fixed_base_device(g16_ctx* ctx, void* d_table, bool table_ready, const void* d_scalars, uint32_t mont, size_t n,
                          void* d_out);
// *d_first_bad (device u32, 0xffffffff on entry) = index of the first point off the curve
template <class C>
int32_t on_curve_device(g16_ctx* ctx, const void* d_points, size_t n, uint32_t* d_first_bad);
// *d_n_inf (device u32, zeroed by the caller) += number of (0,0) points; bitmap: ceil(n/32) words
template <class C>
int32_t live_bitmap_device(g16_ctx* ctx, const void* d_points, size_t n, uint32_t* d_bitmap, uint32_t* d_n_inf);
// sum of `count` XYZZ partials -> affine
template <class C>
int32_t sum_partials_device(g16_ctx* ctx, const void* d_parts, uint32_t count, void* d_out_aff);

// row-binned sparse matrices over Fr (spmv.hip): nmat = 2 -> the A and B matrices of a key, apply = buildABC
struct g16_spmat;
int32_t g16_spmat_create(g16_ctx* ctx, uint32_t nmat, uint32_t nrows, size_t nnz, const uint32_t* vrow,
                         size_t vrow_stride, const uint32_t* col, size_t col_stride, const void* val_base,
                         size_t val_stride, g16_spmat** out, bool values_r2 = false);
void g16_spmat_destroy(g16_spmat* m);
void g16_spmat_info(const g16_spmat* m, size_t out[10]);   // dictionary size (0: plain values), virtual rows per bin
// nmat == 2: d_out = Az | Bz | Cz; need_cz = false: Cz may be left unwritten (the quotient forms it on the fly)
// nmat == 3 (A, B and C of a circuit, witness_check.hip): d_out = A z | B z | C z, nrows each.  x_mont = 0 and no
// dictionary: the sums are in standard form and stay so; every other case gives Montgomery sums
int32_t g16_spmat_apply(g16_ctx* ctx, const g16_spmat* m, const void* d_x, uint32_t x_mont, void* d_out,
                        bool need_cz = true);
int32_t g16_ntt_device(g16_ctx* ctx, const void* d_src, void* d_dst, uint32_t log2n, int inverse);
// computeSnarkjsScalarCoeffs (flavour 1, prover.nim:158-181) / computeQuotientPointwise (flavour 0, :118-148)
// d_a, d_b, d_c, d_out: n elements each (device); inputs are not modified
int32_t g16_quotient_device(g16_ctx* ctx, const void* d_a, const void* d_b, const void* d_c, uint32_t log2n,
                            int flavour, void* d_out, int c_from_ab = 0);
// one coset pipeline (shiftEvalDomain, prover.nim:109-113) and the pointwise step on separately held slices: the
// pieces of the task-parallel quotient of a sharded proof
int32_t g16_coset_pipeline_device(g16_ctx* ctx, const void* d_in, uint32_t log2n, void* d_out);
int32_t g16_abc_pointwise_device(g16_ctx* ctx, const void* d_a, const void* d_b, const void* d_c, size_t count,
                                 void* d_out);

// ---- key audit (audit.hip), shared with the circuit audit (circuit_audit.hip) ------------------------------------------
// 16-byte multipliers -> 32-byte standard scalars; a zero one: G16_EINVAL, "<who>: multiplier <i> is zero"
int32_t g16_widen_multipliers(g16_ctx* ctx, const char* who, const void* multipliers, size_t n, std::vector<uint64_t>& out);
// the body of g16_key_audit
int32_t g16_key_audit_body(g16_ctx* ctx, const g16_pkey_desc* d, const g16_vkey_desc* vk, const void* section4,
                           size_t section4_bytes, const void* multipliers, g16_key_report* out);
// the element passes (audit_points) over `nsec` host arrays, group 1 = G1, 2 = G2 (with the order-r check); results as
// g16_points_audit_*.  `coeffs` (the key audit): then the pass over the values of `count` coefficient records, `stride`
// bytes apart with the value `value_offset` bytes in; its results are row `nsec`.  One wait, at the end, on every path.
// The caller has entered the context.  Callers go through ElementPass (checker.hpp).
struct g16_audit_section {
  int group;
  const void* p;
  size_t n;
};
struct g16_audit_coeffs {
  const void* base;
  size_t count, stride, value_offset;
};
int32_t g16_audit_sections(g16_ctx* ctx, const g16_audit_section* sec, int nsec, size_t (*first_bad)[3],
                           size_t (*bad_count)[3], const g16_audit_coeffs* coeffs = nullptr);

// d_result[j] = ( prod_{k<4} e(+-d_P[4j+k], d_Q[4j+k]) == 1 ), j < count; bit k of neg_mask negates pair k; a pair with (0,0)
// on either side contributes one (circuit_audit.hip: the kernel of the circuit audit's point relations)
int32_t g16_pairing_products4(g16_ctx* ctx, const void* d_P, const void* d_Q, uint32_t count, uint32_t neg_mask,
                              int32_t* d_result);

// ---- circuit setup (circuit_setup.hip); kernels and launcher bodies in circuit_setup.cuh, instantiated per curve in
// circuit_setup_g1.hip / circuit_setup_g2.hip.  Device pointers, the context's stream, nothing waits. ----------------------
namespace g16 {
struct u256;   // ff.cuh
}
// d_out[i] = c * w0 * s^i (setup.hip: the geometric-sequence kernel of the fake setup; `lagrange`: c x_i / (tau - x_i))
int32_t g16_setup_geometric(g16_ctx* ctx, bool lagrange, const g16::u256& w0, const g16::u256& s, const g16::u256& c,
                            const g16::u256& tau, size_t count, g16::u256* d_out, uint32_t* d_first_zero);
namespace g16 {
// out_acc[rev(e)] = val[vstride * ord[e]] * pts[src[e]], e < count (cs_term, circuit_setup.cuh)
template <class C>
int32_t cs_term_device(g16_ctx* ctx, const void* d_pts, const uint32_t* d_src, const void* d_val, const uint32_t* d_ord,
                       uint32_t vstride, uint32_t mont, uint32_t log2rev, size_t count, void* d_out_acc);
// the log2n stages of the inverse NTT over 2^log2n XYZZ points in bit-reversed order, in place
template <class C>
int32_t cs_butterflies_device(g16_ctx* ctx, void* d_v, const void* d_tw, uint32_t log2n);
template <class C>
int32_t cs_segsum_device(g16_ctx* ctx, const void* d_terms, const uint32_t* d_off, const uint32_t* d_wires,
                         const CsSumPlan& plan, void* d_out_aff);
template <class C>
int32_t cs_to_affine_device(g16_ctx* ctx, const void* d_acc, size_t count, void* d_out_aff);
template <class C>
int32_t cs_diff_device(g16_ctx* ctx, const void* d_p, const void* d_q, size_t count, void* d_out_aff);
}  // namespace g16

// ---- one scalar times an array of points (scale.hip); kernel and launcher body in scale.cuh, instantiated per curve in
// scale_g1.hip / scale_g2.hip.  Device pointers, the context's stream, nothing waits. --------------------------------------
namespace g16 {
struct ScalePlan;   // scale_plan.hpp
struct ScaleJob;
// d_out_aff[i] = k * d_pts[i], canonical affine; d_out_aff may be d_pts
template <class C>
int32_t scale_uniform_device(g16_ctx* ctx, const void* d_pts, size_t n, const ScaleJob& job, void* d_out_aff);
// d_out_aff[i] = d_scalars[i] * d_pts[i] (scale_each.cuh, instantiated in scale_each_g1.hip / scale_each_g2.hip); d_scalars:
// n x 32 bytes in HBM, canonical, Montgomery form if `mont`; d_out_aff may be d_pts
template <class C>
int32_t scale_each_device(g16_ctx* ctx, const void* d_pts, size_t n, const void* d_scalars, uint32_t mont, void* d_out_aff);
}  // namespace g16
// the job of k (standard form, < r): its plan into `plan` (the host copy the upload reads: it must outlive the stream's
// work) and into d_steps (ScalePlan::MAX_STEPS words of device memory)
int32_t g16_scale_job(g16_ctx* ctx, const g16::u256& k_std, g16::ScalePlan& plan, uint32_t* d_steps, g16::ScaleJob& job);

// ---- the two halves of g16_prove_combine (prover.hip), shared with the prover pool (pool.hip) ----------------------
// What the finish half needs from the enqueue half: the mask in standard form and the mask-only parts of the proof
// (r, s; alpha1 + r delta1; beta2 + s delta2; s alpha1 + r beta1 + rs delta1), as bytes.
struct g16_combine_pre {
  unsigned char r_std[32], s_std[32];
  unsigned char a_pre[64], b_pre[128], c_pre[64];
};
// stage copy + combine kernel on ctx->stream, host algebra, then the 384-byte D2H into res_host (+ event `done`)
int32_t g16_combine_enqueue(g16_ctx* ctx, const g16_pkey* k, const void* partials, size_t count, uint32_t flags,
                            const void* mask_r, const void* mask_s, void* res_host, hipEvent_t done,
                            g16_combine_pre* pre);
// the additions and the one joint multiplication on the MSM sums; res_host must be complete
void g16_combine_finish(const g16_combine_pre* pre, const void* res_host, g16_proof* out);
