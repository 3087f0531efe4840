// Prover pool: `depth` proofs in flight on one GPU behind submit / poll / collect, driven by ONE host thread
// (include/g16hip.h, "prover pool").  The reference proves with one blocking call (groth16/prover.nim:215-304); a
// caller of g16_prove that wants several proofs on the GPU at once needs a thread per context.  The pool is that
// arrangement without threads: every step is taken inside the caller's calls, and no kernel is new -- each proof is
// g16_prove_partials + the enqueue half of g16_prove_combine on one of the pool's contexts, and collect runs the finish
// half (prover.hip), exactly what g16_prove runs.
//
// Per proof (one of depth + 1 records):
//   submit   witness -> the record's device buffer `d_w` on the pool's copy stream, the record's event `up` behind it
//   launch   (a free slot) the slot context's main stream waits for `up`; g16_prove_partials copies d_w into the
//            context's own prove buffer and enqueues the proof; the combine's enqueue half adds the 384-byte result
//            copy into the record's pinned slot and the record's event `done`
//   done     `done` has completed: the slot is free again, the result waits in pinned memory
//   collect  finish half on the host; the record is free again
// With all slots busy one more proof may be submitted: its witness uploads while the others run (the prefetch), and
// the first pool call that sees a slot free launches it.  A record's d_w is written again only after its proof has
// been collected, i.e. after `done`: the copy stream never waits for a slot's stream.
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "pkey.hpp"

namespace {
enum RecState { REC_FREE, REC_PENDING, REC_RUNNING, REC_DONE };
struct PoolRec {
  uint64_t ticket = 0;
  RecState state = REC_FREE;
  int slot = -1;
  uint32_t flags = 0;
  unsigned char r[32], s[32];   // mask, Montgomery (zero when the caller passed NULL)
  g16_combine_pre pre;          // written by the enqueue half at launch
  DevMem<> d_w;                 // device witness buffer (nvars * 32 bytes)
  Event up;                     // the upload into d_w has completed
  Event done;                   // the result copy into the pinned slot has completed
};
}  // namespace

// The contexts are destroyed by g16_prover_destroy, which also drains the copy stream; the other members release
// themselves when it deletes the pool (no work is left on the device by then, so their order does not matter).
struct g16_prover {
  int device = 0;
  const g16_pkey* key = nullptr;
  uint32_t depth = 0;
  size_t wbytes = 0;                   // nvars * 32
  std::vector<g16_ctx*> ctx;           // one per slot
  std::vector<int> slot_rec;           // record running on each slot, -1 = free
  std::vector<PoolRec> rec;            // depth + 1 records: one per outstanding proof
  Stream copy;                         // witness uploads (non-blocking; not a lane of any context)
  DevMem<unsigned char> d_part;        // depth x G16_PARTIALS_BYTES: the partial record of each slot (HBM)
  PinnedMem<unsigned char> h_res;      // (depth + 1) x G16_COMBINE_RES_BYTES, pinned: the MSM sums of each record
  uint64_t next_ticket = 1;
  int32_t failed = G16_OK;
  std::string err;
};

static int32_t pool_fail(g16_prover* p, int32_t rc, const std::string& msg) {
  if (p->failed == G16_OK) {
    p->failed = rc;
    p->err = msg;
  }
  return p->failed;
}
static int32_t pool_einval(g16_prover* p, const char* msg) {
  if (p->failed == G16_OK) p->err = msg;
  return G16_EINVAL;
}
// a failed HIP call of the pool itself: g16_hip_check's message and code, through pool_fail
static int32_t pool_hip(g16_prover* p, const char* call, hipError_t e) {
  std::string msg;
  const int32_t rc = g16_hip_check(msg, call, e);
  return rc ? pool_fail(p, rc, msg) : G16_OK;
}
#define POOLCHK(p, call)                                          \
  do {                                                            \
    if (int32_t rc__ = pool_hip(p, #call, (call))) return rc__;   \
  } while (0)

// enqueue record i on free slot `slot` (never waits for the GPU)
static int32_t pool_launch(g16_prover* p, int i, int slot) {
  PoolRec& r = p->rec[i];
  g16_ctx* c = p->ctx[slot];
  unsigned char* part = p->d_part.get() + (size_t)slot * G16_PARTIALS_BYTES;
  POOLCHK(p, hipStreamWaitEvent(c->stream, r.up.get(), 0));
  const uint32_t flags = (r.flags & G16_SCALARS_MONT) | G16_SCALARS_DEVICE | G16_OUT_DEVICE | G16_NO_HOST_SYNC;
  int32_t rc = g16_prove_partials(c, p->key, r.d_w.get(), flags, part);
  if (rc) return pool_fail(p, rc, c->err);
  rc = g16_combine_enqueue(c, p->key, part, 1, G16_SCALARS_DEVICE, r.r, r.s,
                           p->h_res.get() + (size_t)i * G16_COMBINE_RES_BYTES, r.done.get(), &r.pre);
  if (rc) return pool_fail(p, rc, c->err);
  r.state = REC_RUNNING;
  r.slot = slot;
  p->slot_rec[slot] = i;
  return G16_OK;
}

// the progress step of every pool call: running proofs whose event has completed free their slot, and a prefetched
// proof takes a free slot
static int32_t pool_advance(g16_prover* p) {
  for (size_t i = 0; i < p->rec.size(); ++i) {
    PoolRec& r = p->rec[i];
    if (r.state != REC_RUNNING) continue;
    const hipError_t q = hipEventQuery(r.done.get());
    if (q == hipErrorNotReady) continue;
    if (q != hipSuccess) return pool_fail(p, G16_EHIP, std::string("proof failed on the GPU: ") + hipGetErrorString(q));
    r.state = REC_DONE;
    p->slot_rec[r.slot] = -1;
    r.slot = -1;
  }
  for (size_t i = 0; i < p->rec.size(); ++i) {
    if (p->rec[i].state != REC_PENDING) continue;
    for (uint32_t s = 0; s < p->depth; ++s)
      if (p->slot_rec[s] < 0) return pool_launch(p, (int)i, (int)s);
    break;   // (at most one proof is pending)
  }
  return G16_OK;
}

// common entry of submit / poll / collect
static int32_t pool_enter(g16_prover* p) {
  if (p->failed) return p->failed;
  POOLCHK(p, hipSetDevice(p->device));
  return pool_advance(p);
}

static int pool_find(const g16_prover* p, uint64_t ticket) {
  for (size_t i = 0; i < p->rec.size(); ++i)
    if (p->rec[i].state != REC_FREE && p->rec[i].ticket == ticket) return (int)i;
  return -1;
}

extern "C" void g16_prover_destroy(g16_prover* p) {
  if (!p) return;
  (void)hipSetDevice(p->device);
  for (g16_ctx* c : p->ctx) g16_ctx_destroy(c);   // waits for its streams: every launched proof
  if (p->copy) (void)hipStreamSynchronize(p->copy.get());   // a prefetched upload
  delete p;
}

extern "C" int32_t g16_prover_create(int32_t device, const g16_pkey* key, uint32_t depth, g16_prover** out) {
  if (!out) return G16_EINVAL;
  *out = nullptr;
  if (!key || depth < 1 || depth > 8) return G16_EINVAL;
  if (key->shard_count != 1 || key->device != device) return G16_EINVAL;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return G16_ENODEV;
  if (device < 0 || device >= ndev) return G16_EINVAL;
  if (hipSetDevice(device) != hipSuccess) return G16_ENODEV;
  Building<g16_prover, g16_prover_destroy> p(new (std::nothrow) g16_prover());
  if (!p) return G16_ENOMEM;
  try {
    p->device = device;
    p->key = key;
    p->depth = depth;
    p->wbytes = (size_t)key->nvars * 32;
    p->ctx.assign(depth, nullptr);
    p->slot_rec.assign(depth, -1);
    p->rec.resize(depth + 1);
  } catch (const std::bad_alloc&) {
    return G16_ENOMEM;
  }
  for (uint32_t s = 0; s < depth; ++s)
    if (int32_t rc = g16_ctx_create(device, &p->ctx[s])) return rc;
  POOLCHK(p.get(), stream_create(p->copy));
  for (PoolRec& r : p->rec) {
    POOLCHK(p.get(), event_create(r.done));
    POOLCHK(p.get(), event_create(r.up));
    POOLCHK(p.get(), dev_alloc(r.d_w, p->wbytes));
  }
  POOLCHK(p.get(), dev_alloc(p->d_part, (size_t)depth * G16_PARTIALS_BYTES));
  POOLCHK(p.get(), pinned_alloc(p->h_res, (size_t)(depth + 1) * G16_COMBINE_RES_BYTES));
  *out = p.release();
  return G16_OK;
}

extern "C" const char* g16_prover_last_error(const g16_prover* p) { return p ? p->err.c_str() : "null prover"; }

extern "C" int32_t g16_prover_submit(g16_prover* p, const void* witness, uint32_t flags, const void* mask_r,
                                     const void* mask_s, uint64_t* ticket) {
  if (!p) return G16_EINVAL;
  if (p->failed) return p->failed;
  if (!witness || !ticket || (flags & ~(G16_SCALARS_MONT | G16_SCALARS_DEVICE)))
    return pool_einval(p, "bad argument (flags: G16_SCALARS_MONT / G16_SCALARS_STD | G16_SCALARS_DEVICE)");
  if (int32_t rc = pool_enter(p)) return rc;
  int i = -1;
  for (size_t j = 0; j < p->rec.size(); ++j)
    if (p->rec[j].state == REC_FREE) {
      i = (int)j;
      break;
    }
  if (i < 0) return G16_EBUSY;   // depth + 1 outstanding
  PoolRec& r = p->rec[i];
  // (a free record's d_w is no longer read: its last proof was collected, after its `done` event)
  POOLCHK(p, hipMemcpyAsync(r.d_w.get(), witness, p->wbytes,
                            (flags & G16_SCALARS_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                            p->copy.get()));
  POOLCHK(p, hipEventRecord(r.up.get(), p->copy.get()));
  r.flags = flags;
  memset(r.r, 0, 32);
  memset(r.s, 0, 32);
  if (mask_r) memcpy(r.r, mask_r, 32);
  if (mask_s) memcpy(r.s, mask_s, 32);
  r.ticket = p->next_ticket++;
  r.state = REC_PENDING;
  *ticket = r.ticket;
  return pool_advance(p);   // straight to a free slot, if there is one
}

extern "C" int32_t g16_prover_poll(g16_prover* p, uint64_t ticket) {
  if (!p) return G16_EINVAL;
  if (int32_t rc = pool_enter(p)) return rc;
  const int i = pool_find(p, ticket);
  if (i < 0) return pool_einval(p, "unknown or already collected ticket");
  return p->rec[i].state == REC_DONE ? 1 : 0;
}

extern "C" int32_t g16_prover_collect(g16_prover* p, uint64_t ticket, g16_proof* out) {
  if (!p) return G16_EINVAL;
  if (!out) return pool_einval(p, "null output");
  if (int32_t rc = pool_enter(p)) return rc;
  const int i = pool_find(p, ticket);
  if (i < 0) return pool_einval(p, "unknown or already collected ticket");
  PoolRec& r = p->rec[i];
  while (r.state != REC_DONE) {
    // While a proof waits for a slot it must take the FIRST slot that frees, whichever that is: query every running
    // proof.  Otherwise block on this one.
    bool pending = false;
    for (const PoolRec& q : p->rec) pending |= q.state == REC_PENDING;
    if (r.state == REC_RUNNING && !pending) POOLCHK(p, hipEventSynchronize(r.done.get()));
    else std::this_thread::yield();
    if (int32_t rc = pool_advance(p)) return rc;
  }
  g16_combine_finish(&r.pre, p->h_res.get() + (size_t)i * G16_COMBINE_RES_BYTES, out);
  r.state = REC_FREE;
  r.ticket = 0;
  return G16_OK;
}

extern "C" int32_t g16_host_alloc(int32_t device, size_t bytes, void** out) {
  if (!out) return G16_EINVAL;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return G16_ENODEV;
  if (device < 0 || device >= ndev || bytes == 0) return G16_EINVAL;
  if (hipSetDevice(device) != hipSuccess) return G16_ENODEV;
  PinnedMem<> mem;   // handed to the caller, who returns it to g16_host_free
  if (pinned_alloc(mem, bytes) != hipSuccess) return G16_ENOMEM;
  *out = mem.release();
  return G16_OK;
}

extern "C" void g16_host_free(void* p) {
  if (p) HostFree{}(p);
}
