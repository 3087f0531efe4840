// ab_prove -- throughput of ONE build of libg16hip.so on a .zkey / .wtns pair, for paired same-box A/B runs of
// several builds (tools/ab_rounds.sh).  The library is dlopen()ed from the path given with -l, so the very same
// binary, key file, witness and protocol measure every build; only entry points that exist since round 1 are used
// (g16_ctx_create, g16_pkey_create, g16_prove, g16_pkey_destroy, g16_ctx_destroy).
//
//   g++ -O2 -std=c++17 -Iinclude tools/ab_prove.cpp -ldl -lpthread -o ab_prove
//   ./ab_prove -l path/to/libg16hip.so -z circuit.zkey -w witness.wtns [-k steps] [-f inflight] [-K] [-r reps] [-s S]
//
// -s S: the key as a lean key at table stride S (g16_pkey_create_lean; builds without it are refused), its table bytes
// printed beside the batches.
//
// Protocol = bench.py's replica mode: `inflight` host threads, one context each, prove `steps` proofs in total from
// the (host, .wtns-layout) witness; wall time over the whole batch; `reps` batches, each printed.  -K: one key per
// context (round 1's ownership rule: a key belonged to the context that created it) instead of one shared key.
// -P depth: ONE host thread proves the `steps` proofs through a prover pool of that depth (g16_prover_*: submit until
// G16_EBUSY, then collect the oldest ticket and submit one more), the witness in pinned memory from g16_host_alloc.
// Builds without the pool (no g16_prover_create symbol) are refused with a message.
#define G16_TOOL_NAME "ab_prove"
#include <dlfcn.h>

#include <atomic>
#include <deque>
#include <thread>

#include "g16_files.hpp"

// fixed mask (Montgomery limbs of two arbitrary residues): the same proof from every build
static void fixed_mask(uint8_t rmask[32], uint8_t smask[32]) {
  for (int i = 0; i < 32; ++i) rmask[i] = (uint8_t)(17 * i + 3), smask[i] = (uint8_t)(29 * i + 5);
  rmask[31] = smask[31] = 0x10;
}

// -P depth: one host thread, one pool
static int run_pool(void* lib, const char* lpath, const ZkeyFile& zf, const WtnsFile& wf, const g16_pkey_desc& d,
                    int depth, int steps, int reps) {
  auto opt = [&](const char* name) {
    void* p = dlsym(lib, name);
    if (!p) die(std::string(lpath) + " has no prover pool (" + name + " is missing): -P needs a build with g16_prover_*");
    return p;
  };
  auto prover_create = (int32_t(*)(int32_t, const g16_pkey*, uint32_t, g16_prover**))opt("g16_prover_create");
  auto prover_destroy = (void (*)(g16_prover*))opt("g16_prover_destroy");
  auto prover_error = (const char* (*)(const g16_prover*))opt("g16_prover_last_error");
  auto submit = (int32_t(*)(g16_prover*, const void*, uint32_t, const void*, const void*, uint64_t*))opt("g16_prover_submit");
  auto collect = (int32_t(*)(g16_prover*, uint64_t, g16_proof*))opt("g16_prover_collect");
  auto host_alloc = (int32_t(*)(int32_t, size_t, void**))opt("g16_host_alloc");
  auto host_free = (void (*)(void*))opt("g16_host_free");
  auto ctx_create = (int32_t(*)(int32_t, g16_ctx**))opt("g16_ctx_create");
  auto ctx_destroy = (void (*)(g16_ctx*))opt("g16_ctx_destroy");
  auto last_error = (const char* (*)(const g16_ctx*))opt("g16_last_error");
  auto pkey_create = (int32_t(*)(g16_ctx*, const g16_pkey_desc*, g16_pkey**))opt("g16_pkey_create");
  auto pkey_destroy = (void (*)(g16_pkey*))opt("g16_pkey_destroy");
  auto prove = (int32_t(*)(g16_ctx*, const g16_pkey*, const void*, uint32_t, const void*, const void*, g16_proof*))opt("g16_prove");

  g16_ctx* ctx = nullptr;
  g16_pkey* key = nullptr;
  g16_prover* pool = nullptr;
  if (ctx_create(0, &ctx) != G16_OK) die("no usable GPU");
  if (pkey_create(ctx, &d, &key) != G16_OK) die(std::string("g16_pkey_create: ") + last_error(ctx));
  const size_t wbytes = (size_t)zf.nvars * 32;
  void* wpin = nullptr;
  if (host_alloc(0, wbytes, &wpin) != G16_OK) die("g16_host_alloc failed");
  memcpy(wpin, wf.values, wbytes);
  uint8_t rmask[32], smask[32];
  fixed_mask(rmask, smask);
  g16_proof ref;
  if (prove(ctx, key, wf.values, G16_SCALARS_STD, rmask, smask, &ref) != G16_OK)
    die(std::string("g16_prove: ") + last_error(ctx));
  if (prover_create(0, key, (uint32_t)depth, &pool) != G16_OK) die("g16_prover_create failed");
  int bad = 0;
  auto batch = [&](int count) {
    std::deque<uint64_t> open;
    int submitted = 0;
    g16_proof p;
    while (submitted < count || !open.empty()) {
      while (submitted < count) {   // submit until G16_EBUSY
        uint64_t t = 0;
        const int32_t rc = submit(pool, wpin, G16_SCALARS_STD, rmask, smask, &t);
        if (rc == G16_EBUSY) break;
        if (rc != G16_OK) die(std::string("g16_prover_submit: ") + prover_error(pool));
        open.push_back(t);
        ++submitted;
      }
      if (collect(pool, open.front(), &p) != G16_OK) die(std::string("g16_prover_collect: ") + prover_error(pool));
      open.pop_front();
      if (memcmp(&p, &ref, sizeof p)) ++bad;
    }
  };
  batch(4 * depth);   // warm-up: workspaces, clocks
  uint64_t fp = 1469598103934665603ull;
  for (size_t i = 0; i < sizeof ref; ++i) fp = (fp ^ ((const uint8_t*)&ref)[i]) * 1099511628211ull;
  for (int r = 0; r < reps; ++r) {
    const double t0 = now();
    batch(steps);
    const double dt = now() - t0;
    printf("%s proofs_per_s %.2f ms_per_proof %.3f steps %d pool_depth %d threads 1 proof_fnv %016llx\n", lpath,
           steps / dt, dt / steps * 1e3, steps, depth, (unsigned long long)fp);
    fflush(stdout);
  }
  prover_destroy(pool);
  host_free(wpin);
  pkey_destroy(key);
  ctx_destroy(ctx);
  if (bad) die("a pool proof differed from g16_prove's");
  return 0;
}

int main(int argc, char** argv) {
  const char *lpath = nullptr, *zpath = nullptr, *wpath = nullptr;
  int steps = 96, inflight = 3, reps = 3;
  if (const char* v = getenv("AB_INFLIGHT")) inflight = atoi(v);   // (tools/ab_rounds.sh: per-entry "@AB_INFLIGHT=4")
  bool key_per_ctx = false;
  int pool_depth = 0, table_stride = 0;
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i];
    auto next = [&]() -> const char* {
      if (i + 1 >= argc) die("missing value after " + a);
      return argv[++i];
    };
    if (a == "-l") lpath = next();
    else if (a == "-z") zpath = next();
    else if (a == "-w") wpath = next();
    else if (a == "-k") steps = atoi(next());
    else if (a == "-f") inflight = atoi(next());
    else if (a == "-r") reps = atoi(next());
    else if (a == "-K") key_per_ctx = true;
    else if (a == "-P") pool_depth = atoi(next());
    else if (a == "-s") table_stride = atoi(next());
    else die("unknown option " + a);
  }
  if (!lpath || !zpath || !wpath || steps < 1 || inflight < 1 || inflight > 16 || pool_depth < 0 || pool_depth > 8 ||
      table_stride < 0 || table_stride > 255 || (table_stride && pool_depth))
    die("usage: ab_prove -l libg16hip.so -z circuit.zkey -w witness.wtns [-k steps] [-f inflight | -P depth] [-K] "
        "[-r reps] [-s table_stride]");
  void* lib = dlopen(lpath, RTLD_NOW | RTLD_LOCAL);
  if (!lib) die(std::string("dlopen: ") + dlerror());
  auto sym = [&](const char* name) {
    void* p = dlsym(lib, name);
    if (!p) die(std::string("missing symbol ") + name);
    return p;
  };
  auto ctx_create = (int32_t(*)(int32_t, g16_ctx**))sym("g16_ctx_create");
  auto ctx_destroy = (void (*)(g16_ctx*))sym("g16_ctx_destroy");
  auto last_error = (const char* (*)(const g16_ctx*))sym("g16_last_error");
  auto pkey_create = (int32_t(*)(g16_ctx*, const g16_pkey_desc*, g16_pkey**))sym("g16_pkey_create");
  auto pkey_destroy = (void (*)(g16_pkey*))sym("g16_pkey_destroy");
  auto prove = (int32_t(*)(g16_ctx*, const g16_pkey*, const void*, uint32_t, const void*, const void*, g16_proof*))sym("g16_prove");

  // -s: the lean entry points, which only builds with table strides have
  int32_t (*pkey_create_lean)(g16_ctx*, const g16_pkey_desc*, uint32_t, g16_pkey**) = nullptr;
  int32_t (*points_plan)(int, size_t, uint32_t, uint32_t*, uint32_t*, size_t*) = nullptr;
  if (table_stride) {
    pkey_create_lean = (decltype(pkey_create_lean))sym("g16_pkey_create_lean");
    points_plan = (decltype(points_plan))sym("g16_points_plan");
  }

  ZkeyFile zf(zpath);
  WtnsFile wf(wpath, zf.nvars);
  const g16_pkey_desc d = zf.desc();
  if (points_plan) {   // bytes of the five point sets' tables at this stride (A1, B1, C1 padded to nvars; B2; H1)
    size_t g1w = 0, g2w = 0, g1h = 0;
    uint32_t c = 0, nt = 0;
    points_plan(1, zf.nvars, (uint32_t)table_stride, &c, &nt, &g1w);
    points_plan(2, zf.nvars, (uint32_t)table_stride, nullptr, nullptr, &g2w);
    points_plan(1, size_t(1) << d.log2_domain, (uint32_t)table_stride, nullptr, nullptr, &g1h);
    printf("%s table_stride %d window_bits %u tables %u table_bytes %zu\n", lpath, table_stride, c, nt,
           3 * g1w + g2w + g1h);
  }
  if (pool_depth) return run_pool(lib, lpath, zf, wf, d, pool_depth, steps, reps);
  std::vector<g16_ctx*> ctx(inflight, nullptr);
  std::vector<g16_pkey*> key(inflight, nullptr);
  for (int j = 0; j < inflight; ++j) {
    if (ctx_create(0, &ctx[j]) != G16_OK) die("no usable GPU");
    if (j == 0 || key_per_ctx) {
      const int32_t rc = pkey_create_lean ? pkey_create_lean(ctx[j], &d, (uint32_t)table_stride, &key[j])
                                          : pkey_create(ctx[j], &d, &key[j]);
      if (rc != G16_OK) die(std::string("g16_pkey_create: ") + last_error(ctx[j]));
    } else {
      key[j] = key[0];
    }
  }
  // fixed mask (Montgomery limbs of two arbitrary residues): the same proof from every build
  uint8_t rmask[32], smask[32];
  for (int i = 0; i < 32; ++i) rmask[i] = (uint8_t)(17 * i + 3), smask[i] = (uint8_t)(29 * i + 5);
  rmask[31] = smask[31] = 0x10;
  g16_proof ref;
  if (prove(ctx[0], key[0], wf.values, G16_SCALARS_STD, rmask, smask, &ref) != G16_OK)
    die(std::string("g16_prove: ") + last_error(ctx[0]));
  std::atomic<int> bad{0};
  auto batch = [&](int count) {
    std::vector<std::thread> th;
    for (int j = 0; j < inflight; ++j)
      th.emplace_back([&, j]() {
        g16_proof p;
        for (int i = j; i < count; i += inflight) {
          if (prove(ctx[j], key[j], wf.values, G16_SCALARS_STD, rmask, smask, &p) != G16_OK) ++bad;
          else if (memcmp(&p, &ref, sizeof p)) ++bad;
        }
      });
    for (auto& t : th) t.join();
  };
  batch(4 * inflight);   // warm-up: workspaces, clocks
  // proof bytes as a short fingerprint, so that the A/B script can require identical proofs from every build
  uint64_t fp = 1469598103934665603ull;
  for (size_t i = 0; i < sizeof ref; ++i) fp = (fp ^ ((const uint8_t*)&ref)[i]) * 1099511628211ull;
  for (int r = 0; r < reps; ++r) {
    const double t0 = now();
    batch(steps);
    const double dt = now() - t0;
    printf("%s proofs_per_s %.2f ms_per_proof %.3f steps %d inflight %d keys %d proof_fnv %016llx\n", lpath,
           steps / dt, dt / steps * 1e3, steps, inflight, key_per_ctx ? inflight : 1, (unsigned long long)fp);
    fflush(stdout);
  }
  // single-proof latency
  {
    const double t0 = now();
    g16_proof p;
    for (int i = 0; i < 5; ++i) prove(ctx[0], key[0], wf.values, G16_SCALARS_STD, rmask, smask, &p);
    printf("%s latency_ms %.3f\n", lpath, (now() - t0) / 5 * 1e3);
  }
  if (bad) die("a proof failed or differed from the first one");
  for (int j = 0; j < inflight; ++j)
    if (j == 0 || key_per_ctx) pkey_destroy(key[j]);
  for (int j = 0; j < inflight; ++j) ctx_destroy(ctx[j]);
  return 0;
}
