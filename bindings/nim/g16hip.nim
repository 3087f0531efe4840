## groth16/gpu/g16hip.nim -- Nim binding of libg16hip.so (include/g16hip.h) for codex-storage/nim-groth16.
##
## Keeps the reference's proc names and signatures (groth16/bn128/msm.nim:89,128,202-203; groth16/math/ntt.nim:55,139;
## groth16/prover.nim:215; groth16/verifier.nim:31) so that prover.nim compiles against it unchanged.
## Assembled from INTEGRATION.md sections 2, 3 and "Verifier".  NOT compile-tested: this image has no `nim` / `nimble`
## and constantine is not vendored (SURVEY.md section 8c); the same boundary is exercised through ctypes
## (nim_groth16_amd/_lib.py), plain C (examples/c_abi_demo.c) and C++ (tools/g16prove.cpp) by the GPU tests.
##
## Build: nim c --passC:-I<repo>/include --passL:-L<repo>/nim_groth16_amd/csrc --passL:-lg16hip ...

# groth16/gpu/g16hip.nim -- binds libg16hip.so; keeps the signatures of bn128/msm.nim and math/ntt.nim
import groth16/bn128
import groth16/math/domain
import groth16/zkey_types
import groth16/files/witness
import std/tables
import std/sysrand

{.passL: "-lg16hip".}
type
  G16Ctx   {.importc: "g16_ctx",    header: "g16hip.h", incompleteStruct.} = object
  G16PKey  {.importc: "g16_pkey",   header: "g16hip.h", incompleteStruct.} = object
  G16Coeff {.importc: "g16_coeff",  header: "g16hip.h".} = object
    matrix, row, col, reserved: uint32
    value: array[32, byte]
  G16PKeyDesc {.importc: "g16_pkey_desc", header: "g16hip.h".} = object
    nvars, npubs, log2_domain, flavour: uint32
    pointsA1, pointsB1, pointsB2, pointsC1, pointsH1: pointer
    coeffs: ptr G16Coeff
    ncoeffs: csize_t
    alpha1, beta1, delta1, beta2, delta2: pointer
    shard_index, shard_count: uint32
  G16Proof {.importc: "g16_proof", header: "g16hip.h".} = object
    pi_a: array[64, byte]; pi_b: array[128, byte]; pi_c: array[64, byte]

const G16_SCALARS_MONT = 1'u32

proc g16_ctx_create(device: int32, ctx: ptr ptr G16Ctx): int32 {.importc, header: "g16hip.h".}
proc g16_selftest(ctx: ptr G16Ctx): int32 {.importc, header: "g16hip.h".}
proc g16_last_error(ctx: ptr G16Ctx): cstring {.importc, header: "g16hip.h".}
proc g16_msm_g1(ctx: ptr G16Ctx, scalars: pointer, flags: uint32, points: pointer, n: csize_t, res: pointer): int32 {.importc, header: "g16hip.h".}
proc g16_msm_g2(ctx: ptr G16Ctx, scalars: pointer, flags: uint32, points: pointer, n: csize_t, res: pointer): int32 {.importc, header: "g16hip.h".}
proc g16_ntt_fr(ctx: ptr G16Ctx, src, dst: pointer, log2n: uint32, inverse: int32): int32 {.importc, header: "g16hip.h".}
proc g16_quotient(ctx: ptr G16Ctx, az, bz, cz: pointer, log2n, flavour: uint32, res: pointer): int32 {.importc, header: "g16hip.h".}
proc g16_pkey_create(ctx: ptr G16Ctx, desc: ptr G16PKeyDesc, key: ptr ptr G16PKey): int32 {.importc, header: "g16hip.h".}
proc g16_pkey_create_lean(ctx: ptr G16Ctx, desc: ptr G16PKeyDesc, tableStride: uint32, key: ptr ptr G16PKey): int32 {.importc, header: "g16hip.h".}
proc g16_prove(ctx: ptr G16Ctx, key: ptr G16PKey, witness: pointer, flags: uint32, r, s: pointer, res: ptr G16Proof): int32 {.importc, header: "g16hip.h".}
# points at infinity per ProverPoints array (A1, B1, B2, C1, H1, B1-and-B2) and whether A1 / B1+B2 run on compacted
# entry lists: snarkjs keys hold (0,0) for every wire absent from a matrix (curves.nim:95-107 accepts them)
proc g16_pkey_inf_counts(key: ptr G16PKey, res: ptr array[8, csize_t]): int32 {.importc, header: "g16hip.h".}
proc g16_pkey_b1_fold(key: ptr G16PKey, res: ptr array[3, csize_t]): int32 {.importc, header: "g16hip.h".}
proc g16_pkey_b1_sparse(key: ptr G16PKey, res: ptr array[3, csize_t]): int32 {.importc, header: "g16hip.h".}

var gctx: ptr G16Ctx

proc check(rc: int32) =
  if rc != 0: raise newException(AssertionDefect, "g16hip: " & $g16_last_error(gctx))

proc initG16Hip*(device = 0) =
  doAssert sizeof(Fr) == 32 and sizeof(G1) == 64 and sizeof(G2) == 128, "constantine layout changed"
  check g16_ctx_create(int32(device), addr gctx)
  check g16_selftest(gctx)

# --- drop-ins for groth16/bn128/msm.nim:89,128,202-203 ---------------------------------------------------
proc msmMultiThreadedG1*(nthreads_hint: int, coeffs: seq[Fr], points: seq[G1]): G1 =
  assert coeffs.len == points.len, "incompatible sequence lengths"          # msm.nim:97
  if coeffs.len == 0: return infG1                                            # msm.nim:117
  check g16_msm_g1(gctx, unsafeAddr coeffs[0], G16_SCALARS_MONT, unsafeAddr points[0], csize_t(coeffs.len), addr result)

proc msmMultiThreadedG2*(nthreads_hint: int, coeffs: seq[Fr], points: seq[G2]): G2 =
  assert coeffs.len == points.len, "incompatible sequence lengths"          # msm.nim:131
  if coeffs.len == 0: return infG2
  check g16_msm_g2(gctx, unsafeAddr coeffs[0], G16_SCALARS_MONT, unsafeAddr points[0], csize_t(coeffs.len), addr result)

proc msmG1*(coeffs: seq[Fr], points: seq[G1]): G1 = msmMultiThreadedG1(0, coeffs, points)
proc msmG2*(coeffs: seq[Fr], points: seq[G2]): G2 = msmMultiThreadedG2(0, coeffs, points)

# --- drop-ins for groth16/math/ntt.nim:55,139 ---------------------------------------------------------------
proc forwardNTT*(src: seq[Fr], D: Domain): seq[Fr] =
  assert D.domainSize == (1 shl D.logDomainSize) and D.domainSize == src.len   # ntt.nim:56-57
  result = newSeq[Fr](src.len)
  check g16_ntt_fr(gctx, unsafeAddr src[0], addr result[0], uint32(D.logDomainSize), 0)

proc inverseNTT*(src: seq[Fr], D: Domain): seq[Fr] =
  assert D.domainSize == (1 shl D.logDomainSize) and D.domainSize == src.len   # ntt.nim:140-141
  result = newSeq[Fr](src.len)
  check g16_ntt_fr(gctx, unsafeAddr src[0], addr result[0], uint32(D.logDomainSize), 1)

# --- drop-in for computeSnarkjsScalarCoeffs / computeQuotientPointwise (prover.nim:118-181) ------------------
proc computeQuotientGpu*(valuesAz, valuesBz, valuesCz: seq[Fr], flavour: Flavour): seq[Fr] =
  let n = valuesAz.len
  result = newSeq[Fr](n)
  check g16_quotient(gctx, unsafeAddr valuesAz[0], unsafeAddr valuesBz[0], unsafeAddr valuesCz[0],
                     uint32(createDomain(n).logDomainSize), uint32(ord(flavour)), addr result[0])

var gkey: ptr G16PKey
proc loadKeyGpu*(zkey: ZKey, tableStride = 0) =
  ## tableStride >= 2: a lean key -- every ProverPoints array keeps window tables for every tableStride-th window only:
  ## about 1 / tableStride of the HBM, more bucket reduction per proof, the same proof bytes (include/g16hip.h "lean")
  var cs = newSeq[G16Coeff](zkey.coeffs.len)
  for i, c in zkey.coeffs:                                  # zkey_types.nim:48-52
    cs[i] = G16Coeff(matrix: uint32(ord(c.matrix)), row: uint32(c.row), col: uint32(c.col))
    copyMem(addr cs[i].value, unsafeAddr c.coeff, 32)
  var d = G16PKeyDesc(nvars: uint32(zkey.header.nvars), npubs: uint32(zkey.header.npubs),
    log2_domain: uint32(zkey.header.logDomainSize), flavour: uint32(ord(zkey.header.flavour)),
    pointsA1: unsafeAddr zkey.pPoints.pointsA1[0], pointsB1: unsafeAddr zkey.pPoints.pointsB1[0],
    pointsB2: unsafeAddr zkey.pPoints.pointsB2[0], pointsC1: unsafeAddr zkey.pPoints.pointsC1[0],
    pointsH1: unsafeAddr zkey.pPoints.pointsH1[0], coeffs: addr cs[0], ncoeffs: csize_t(cs.len),
    alpha1: unsafeAddr zkey.specPoints.alpha1, beta1: unsafeAddr zkey.specPoints.beta1,
    delta1: unsafeAddr zkey.specPoints.delta1, beta2: unsafeAddr zkey.specPoints.beta2,
    delta2: unsafeAddr zkey.specPoints.delta2, shard_index: 0, shard_count: 1)
  check g16_pkey_create_lean(gctx, addr d, uint32(tableStride), addr gkey)

proc generateProofWithMask*(nthreads: int, printTimings: bool, zkey: ZKey, wtns: Witness, mask: Mask): Proof =
  assert zkey.header.curve == wtns.curve and zkey.header.nvars == wtns.values.len   # prover.nim:224,236
  var p: G16Proof
  check g16_prove(gctx, gkey, unsafeAddr wtns.values[0], G16_SCALARS_MONT, unsafeAddr mask.r, unsafeAddr mask.s, addr p)
  result = Proof(curve: "bn128", publicIO: wtns.values[0..zkey.header.npubs])        # prover.nim:238-240
  copyMem(addr result.pi_a, addr p.pi_a, 64); copyMem(addr result.pi_b, addr p.pi_b, 128); copyMem(addr result.pi_c, addr p.pi_c, 64)

# --- proofs in flight from ONE thread: the prover pool (include/g16hip.h "prover pool") --------------------------------
# generateProofWithMask above blocks for one proof; the multi-proof rate used to need three host threads with a context
# each (INTEGRATION.md section 3).  A pool reaches it from the calling thread, with no thread inside the library:
#   initG16Hip(); loadKeyGpu(zkey); let pool = newProverPool(3)
#   submit until proveAsync returns 0 (G16_EBUSY), then repeat: collectProof the oldest ticket, proveAsync one more
type
  G16Prover {.importc: "g16_prover", header: "g16hip.h", incompleteStruct.} = object
  ProverPool* = ref object
    p: ptr G16Prover
    publicIO: Table[uint64, seq[Fr]]       # per ticket: Proof.publicIO (prover.nim:238-240)
const G16_EBUSY = -6'i32
proc g16_prover_create(device: int32, key: ptr G16PKey, depth: uint32, pool: ptr ptr G16Prover): int32 {.importc, header: "g16hip.h".}
proc g16_prover_destroy(pool: ptr G16Prover) {.importc, header: "g16hip.h".}
proc g16_prover_last_error(pool: ptr G16Prover): cstring {.importc, header: "g16hip.h".}
proc g16_prover_submit(pool: ptr G16Prover, witness: pointer, flags: uint32, r, s: pointer,
                       ticket: ptr uint64): int32 {.importc, header: "g16hip.h".}
proc g16_prover_poll(pool: ptr G16Prover, ticket: uint64): int32 {.importc, header: "g16hip.h".}
proc g16_prover_collect(pool: ptr G16Prover, ticket: uint64, res: ptr G16Proof): int32 {.importc, header: "g16hip.h".}
# pinned host memory: a witness there uploads without making proveAsync wait for the copy
proc g16_host_alloc(device: int32, bytes: csize_t, res: ptr pointer): int32 {.importc, header: "g16hip.h".}
proc g16_host_free(p: pointer) {.importc, header: "g16hip.h".}

proc checkPool(pool: ProverPool, rc: int32) =
  if rc < 0: raise newException(AssertionDefect, "g16hip pool: " & $g16_prover_last_error(pool.p))

proc newProverPool*(depth = 3, device = 0): ProverPool =
  ## after initG16Hip + loadKeyGpu: `depth` proofs on the GPU at once, all against the loaded key
  result = ProverPool(publicIO: initTable[uint64, seq[Fr]]())
  if g16_prover_create(int32(device), gkey, uint32(depth), addr result.p) != 0:
    raise newException(AssertionDefect, "g16hip: g16_prover_create failed")

proc proveAsync*(pool: ProverPool, zkey: ZKey, wtns: Witness, mask: Mask): uint64 =
  ## generateProofWithMask without the wait: the ticket of the proof, or 0 while depth + 1 proofs are outstanding
  ## (G16_EBUSY).  `wtns` must stay alive and unmodified until collectProof of its ticket has returned.
  assert zkey.header.curve == wtns.curve and zkey.header.nvars == wtns.values.len   # prover.nim:224,236
  let rc = g16_prover_submit(pool.p, unsafeAddr wtns.values[0], G16_SCALARS_MONT, unsafeAddr mask.r,
                             unsafeAddr mask.s, addr result)
  if rc == G16_EBUSY: return 0
  pool.checkPool rc
  pool.publicIO[result] = wtns.values[0..zkey.header.npubs]

proc collectProof*(pool: ProverPool, ticket: uint64): Proof =
  ## waits for the proof of `ticket`: the same bytes generateProofWithMask returns for the same inputs
  var p: G16Proof
  pool.checkPool g16_prover_collect(pool.p, ticket, addr p)
  result = Proof(curve: "bn128", publicIO: pool.publicIO[ticket])
  pool.publicIO.del(ticket)
  copyMem(addr result.pi_a, addr p.pi_a, 64); copyMem(addr result.pi_b, addr p.pi_b, 128); copyMem(addr result.pi_c, addr p.pi_c, 64)

proc proofDone*(pool: ProverPool, ticket: uint64): bool =
  ## never blocks
  let rc = g16_prover_poll(pool.p, ticket)
  pool.checkPool rc
  result = rc == 1

proc destroy*(pool: ProverPool) =
  ## waits for the outstanding proofs and discards them; the key stays loaded
  if pool.p != nil: g16_prover_destroy(pool.p)
  pool.p = nil

# --- one proof over several GPUs of the node: the device group (include/g16hip.h "device group") ------------------------
# The reference shards every MSM over Taskpool threads (msm.nim:96-122) and runs the three coset pipelines as three tasks
# (prover.nim:165-173); a group does the same over GPUs, one host thread per device INSIDE the library.  The Nim host only
# names the devices:   initG16Hip([0, 1, 2, 3, 4, 5, 6, 7]);  loadKeyGpu(zkey);  generateProofWithMask(...)
type
  G16Group    {.importc: "g16_group",      header: "g16hip.h", incompleteStruct.} = object
  G16GroupKey {.importc: "g16_group_pkey", header: "g16hip.h", incompleteStruct.} = object
proc g16_group_create(devices: ptr int32, ndev: int32, grp: ptr ptr G16Group): int32 {.importc, header: "g16hip.h".}
proc g16_group_last_error(grp: ptr G16Group): cstring {.importc, header: "g16hip.h".}
proc g16_group_pkey_create(grp: ptr G16Group, desc: ptr G16PKeyDesc, key: ptr ptr G16GroupKey): int32 {.importc, header: "g16hip.h".}
proc g16_group_pkey_create_lean(grp: ptr G16Group, desc: ptr G16PKeyDesc, tableStride: uint32, key: ptr ptr G16GroupKey): int32 {.importc, header: "g16hip.h".}
proc g16_group_prove(grp: ptr G16Group, key: ptr G16GroupKey, witness: pointer, flags: uint32, r, s: pointer,
                     res: ptr G16Proof): int32 {.importc, header: "g16hip.h".}

var ggroup: ptr G16Group
var ggroupKey: ptr G16GroupKey

proc checkGroup(rc: int32) =
  if rc != 0: raise newException(AssertionDefect, "g16hip group: " & $g16_group_last_error(ggroup))

proc initG16Hip*(devices: openArray[int]) =
  ## several GPUs: MSMs, NTTs and the verifier of single calls run on devices[0]; proofs are sharded over all of them
  initG16Hip(devices[0])
  var ds = newSeq[int32](devices.len)
  for i, d in devices: ds[i] = int32(d)
  if g16_group_create(addr ds[0], int32(ds.len), addr ggroup) != 0:
    raise newException(AssertionDefect, "g16hip: g16_group_create failed")

proc loadKeyGroup*(zkey: ZKey, tableStride = 0) =
  ## like loadKeyGpu, sharded: member g keeps index range g of every ProverPoints array (msm.nim:105-115)
  var cs = newSeq[G16Coeff](zkey.coeffs.len)
  for i, c in zkey.coeffs:
    cs[i] = G16Coeff(matrix: uint32(ord(c.matrix)), row: uint32(c.row), col: uint32(c.col))
    copyMem(addr cs[i].value, unsafeAddr c.coeff, 32)
  var d = G16PKeyDesc(nvars: uint32(zkey.header.nvars), npubs: uint32(zkey.header.npubs),
    log2_domain: uint32(zkey.header.logDomainSize), flavour: uint32(ord(zkey.header.flavour)),
    pointsA1: unsafeAddr zkey.pPoints.pointsA1[0], pointsB1: unsafeAddr zkey.pPoints.pointsB1[0],
    pointsB2: unsafeAddr zkey.pPoints.pointsB2[0], pointsC1: unsafeAddr zkey.pPoints.pointsC1[0],
    pointsH1: unsafeAddr zkey.pPoints.pointsH1[0], coeffs: addr cs[0], ncoeffs: csize_t(cs.len),
    alpha1: unsafeAddr zkey.specPoints.alpha1, beta1: unsafeAddr zkey.specPoints.beta1,
    delta1: unsafeAddr zkey.specPoints.delta1, beta2: unsafeAddr zkey.specPoints.beta2,
    delta2: unsafeAddr zkey.specPoints.delta2, shard_index: 0, shard_count: 1)
  checkGroup g16_group_pkey_create_lean(ggroup, addr d, uint32(tableStride), addr ggroupKey)

proc generateProofWithMaskGroup*(nthreads: int, printTimings: bool, zkey: ZKey, wtns: Witness, mask: Mask): Proof =
  ## generateProofWithMask (prover.nim:215-304) over the device group: bit-identical to the one-GPU proof
  assert zkey.header.curve == wtns.curve and zkey.header.nvars == wtns.values.len   # prover.nim:224,236
  var p: G16Proof
  checkGroup g16_group_prove(ggroup, ggroupKey, unsafeAddr wtns.values[0], G16_SCALARS_MONT, unsafeAddr mask.r,
                             unsafeAddr mask.s, addr p)
  result = Proof(curve: "bn128", publicIO: wtns.values[0..zkey.header.npubs])        # prover.nim:238-240
  copyMem(addr result.pi_a, addr p.pi_a, 64); copyMem(addr result.pi_b, addr p.pi_b, 128); copyMem(addr result.pi_c, addr p.pi_c, 64)

# continues groth16/gpu/g16hip.nim above: same `header:` style, every type it names is declared here
type
  G16VKey {.importc: "g16_vkey", header: "g16hip.h", incompleteStruct.} = object
  G16VKeyDesc {.importc: "g16_vkey_desc", header: "g16hip.h".} = object
    npubs: uint32
    alpha1, beta2, gamma2, delta2, pointsIC: pointer

proc g16_vkey_create(ctx: ptr G16Ctx, desc: ptr G16VKeyDesc, key: ptr ptr G16VKey): int32 {.importc, header: "g16hip.h".}
proc g16_vkey_destroy(key: ptr G16VKey) {.importc, header: "g16hip.h".}
proc g16_verify(ctx: ptr G16Ctx, key: ptr G16VKey, proofs: ptr G16Proof, publicIO: pointer, flags: uint32,
                count: csize_t, status: ptr int32): int32 {.importc, header: "g16hip.h".}

proc verifyProof*(vkey: VKey, prf: Proof): bool =
  assert prf.curve == "bn128"                                             # verifier.nim:33
  var d = G16VKeyDesc(npubs: uint32(vkey.vpoints.pointsIC.len - 1), alpha1: unsafeAddr vkey.spec.alpha1,
    beta2: unsafeAddr vkey.spec.beta2, gamma2: unsafeAddr vkey.spec.gamma2, delta2: unsafeAddr vkey.spec.delta2,
    pointsIC: unsafeAddr vkey.vpoints.pointsIC[0])
  var k: ptr G16VKey
  check g16_vkey_create(gctx, addr d, addr k)            # keep `k` per circuit: it caches the (alpha,beta) Miller value
  defer: g16_vkey_destroy(k)
  var p: G16Proof; var st: int32
  copyMem(addr p.pi_a, unsafeAddr prf.pi_a, 64); copyMem(addr p.pi_b, unsafeAddr prf.pi_b, 128); copyMem(addr p.pi_c, unsafeAddr prf.pi_c, 64)
  check g16_verify(gctx, k, addr p, unsafeAddr prf.publicIO[0], G16_SCALARS_MONT, 1, addr st)
  assert st != -1, "pi_a is not in G1"; assert st != -2, "pi_b is not in G2"; assert st != -3, "pi_c is not in G1"   # verifier.nim:35-37
  assert st != -5 and st != -6, "non-canonical field element in the proof / public input"
  result = st == 1

proc g16_verify_batch(ctx: ptr G16Ctx, key: ptr G16VKey, proofs: ptr G16Proof, publicIO: pointer, flags: uint32,
                      count: csize_t, multipliers: pointer, res: ptr int32, status: ptr int32): int32 {.importc, header: "g16hip.h".}

proc verifyProofsBatch*(vkey: VKey, prfs: openArray[Proof]): bool =
  ## "do they all verify?": ONE pairing product for the batch (count + 3 Miller loops, one final exponentiation).
  ## False if any proof is malformed, has pi_b outside the order-r subgroup (always checked) or fails; a batch with a
  ## bad proof passes with probability <= 1/(2^128 - 1) over the multipliers, which are drawn HERE, after the proofs
  ## are fixed, from the OS CSPRNG (std/sysrand) -- the library draws none.  verifyProof tells which proof failed.
  if prfs.len == 0: return true
  var d = G16VKeyDesc(npubs: uint32(vkey.vpoints.pointsIC.len - 1), alpha1: unsafeAddr vkey.spec.alpha1,
    beta2: unsafeAddr vkey.spec.beta2, gamma2: unsafeAddr vkey.spec.gamma2, delta2: unsafeAddr vkey.spec.delta2,
    pointsIC: unsafeAddr vkey.vpoints.pointsIC[0])
  var k: ptr G16VKey
  check g16_vkey_create(gctx, addr d, addr k)
  defer: g16_vkey_destroy(k)
  let nio = vkey.vpoints.pointsIC.len
  var ps = newSeq[G16Proof](prfs.len)
  var io = newSeq[Fr](prfs.len * nio)
  for j, prf in prfs:
    assert prf.curve == "bn128" and prf.publicIO.len == nio
    copyMem(addr ps[j].pi_a, unsafeAddr prf.pi_a, 64); copyMem(addr ps[j].pi_b, unsafeAddr prf.pi_b, 128); copyMem(addr ps[j].pi_c, unsafeAddr prf.pi_c, 64)
    copyMem(addr io[j * nio], unsafeAddr prf.publicIO[0], 32 * nio)
  var zs = newSeq[array[16, byte]](prfs.len)                 # 128-bit little-endian multipliers, none zero
  for z in zs.mitems:
    while true:
      doAssert urandom(z)
      var any = false
      for b in z: any = any or b != 0
      if any: break
  var res: int32
  check g16_verify_batch(gctx, k, addr ps[0], addr io[0], G16_SCALARS_MONT, csize_t(prfs.len), addr zs[0], addr res, nil)
  result = res == 1

# --- key audit (include/g16hip.h "key audit"): is a ZKey from a third party fit to prove with? -------------------------
# The reference asserts the curve equations while it loads a .zkey (mkG1 / mkG2, curves.nim:95-107).  auditKey is for the
# host that is handed keys: canonical encodings, curve membership, the order-r subgroup of every G2 point, coefficient
# values < r, and pointsB1 ~ pointsB2, beta1 ~ beta2, delta1 ~ delta2 -- before loadKeyGpu, and without touching any state.
# It cannot tell whether the key belongs to a circuit: nothing ties A1 / C1 / H1 / IC to an R1CS without the transcript.
const
  G16_AUDIT_SECTIONS* = 13
  auditSectionNames* = ["alpha1", "beta1", "delta1", "beta2", "gamma2", "delta2", "pointsIC", "pointsA1", "pointsB1",
                        "pointsB2", "pointsC1", "pointsH1", "coeffs"]
  auditCheckNames* = ["is not a canonical encoding", "is not on the curve", "is not in the order-r subgroup"]
  auditRelationNames* = ["pointsB1~pointsB2", "beta1~beta2", "delta1~delta2"]
type
  KeyReport* {.importc: "g16_key_report", header: "g16hip.h".} = object
    failed*: uint32                 ## OR of G16_AUDIT_*: 0 = fit to prove with
    spec_infinity*: uint32          ## bit s: spec point s is (0,0)
    relation*: array[3, int32]      ## 1 holds, 0 fails, -1 not run
    reserved: uint32
    first_bad*: array[G16_AUDIT_SECTIONS, array[3, csize_t]]   ## high(csize_t) = none
    bad_count*: array[G16_AUDIT_SECTIONS, array[3, csize_t]]

proc g16_points_audit_g1(ctx: ptr G16Ctx, points: pointer, n: csize_t, firstBad, badCount: ptr csize_t): int32 {.importc, header: "g16hip.h".}
proc g16_points_audit_g2(ctx: ptr G16Ctx, points: pointer, n: csize_t, firstBad, badCount: ptr csize_t): int32 {.importc, header: "g16hip.h".}
proc g16_points_pairs_check(ctx: ptr G16Ctx, g1Points, g2Points: pointer, n: csize_t, multipliers: pointer,
                            res: ptr int32): int32 {.importc, header: "g16hip.h".}
proc g16_key_audit(ctx: ptr G16Ctx, desc: ptr G16PKeyDesc, vk: ptr G16VKeyDesc, section4: pointer, section4Bytes: csize_t,
                   multipliers: pointer, res: ptr KeyReport): int32 {.importc, header: "g16hip.h".}

proc ok*(r: KeyReport): bool = r.failed == 0

proc `$`*(r: KeyReport): string =
  ## the section, index and check of every first finding
  if r.ok: return "key audit: ok"
  result = "key audit: FAILED"
  for s in 0 ..< G16_AUDIT_SECTIONS:
    for k in 0 ..< 3:
      if r.bad_count[s][k] > 0:
        result.add "\n  " & auditSectionNames[s] & "[" & $r.first_bad[s][k] & "] " & auditCheckNames[k]
        if r.bad_count[s][k] > 1: result.add " (and " & $(r.bad_count[s][k] - 1) & " more)"
  for k in 0 ..< 3:
    if r.relation[k] == 0: result.add "\n  " & auditRelationNames[k] & ": not the same multiples of the two generators"
  for s in 0 ..< 6:
    if ((r.spec_infinity shr s) and 1) != 0: result.add "\n  " & auditSectionNames[s] & " is the point at infinity"

proc auditKey*(zkey: ZKey): KeyReport =
  ## g16_key_audit over the whole ZKey (its verifier half included); the multipliers of the batched B1 ~ B2 relation
  ## are drawn HERE from the OS CSPRNG (std/sysrand), as verifyProofsBatch draws its own.
  var cs = newSeq[G16Coeff](max(zkey.coeffs.len, 1))
  for i, c in zkey.coeffs:
    cs[i] = G16Coeff(matrix: uint32(ord(c.matrix)), row: uint32(c.row), col: uint32(c.col))
    copyMem(addr cs[i].value, unsafeAddr c.coeff, 32)
  var d = G16PKeyDesc(nvars: uint32(zkey.header.nvars), npubs: uint32(zkey.header.npubs),
    log2_domain: uint32(zkey.header.logDomainSize), flavour: uint32(ord(zkey.header.flavour)),
    pointsA1: unsafeAddr zkey.pPoints.pointsA1[0], pointsB1: unsafeAddr zkey.pPoints.pointsB1[0],
    pointsB2: unsafeAddr zkey.pPoints.pointsB2[0],
    pointsC1: (if zkey.pPoints.pointsC1.len > 0: unsafeAddr zkey.pPoints.pointsC1[0] else: nil),
    pointsH1: unsafeAddr zkey.pPoints.pointsH1[0], coeffs: addr cs[0], ncoeffs: csize_t(zkey.coeffs.len),
    alpha1: unsafeAddr zkey.specPoints.alpha1, beta1: unsafeAddr zkey.specPoints.beta1,
    delta1: unsafeAddr zkey.specPoints.delta1, beta2: unsafeAddr zkey.specPoints.beta2,
    delta2: unsafeAddr zkey.specPoints.delta2, shard_index: 0, shard_count: 1)
  var v = G16VKeyDesc(npubs: uint32(zkey.header.npubs), alpha1: unsafeAddr zkey.specPoints.alpha1,
    beta2: unsafeAddr zkey.specPoints.beta2, gamma2: unsafeAddr zkey.specPoints.gamma2,
    delta2: unsafeAddr zkey.specPoints.delta2, pointsIC: unsafeAddr zkey.vPoints.pointsIC[0])
  var zs = newSeq[array[16, byte]](zkey.header.nvars)         # 128-bit little-endian multipliers, none zero
  for z in zs.mitems:
    while true:
      doAssert urandom(z)
      var any = false
      for b in z: any = any or b != 0
      if any: break
  check g16_key_audit(gctx, addr d, addr v, nil, 0, addr zs[0], addr result)

# --- circuit audit (include/g16hip.h "circuit audit"): does the key belong to THIS .r1cs and THIS .ptau? ---------------
# What `snarkjs zkey verify circuit.r1cs pot.ptau circuit.zkey` checks before the contribution chain: the key's
# coefficients against the r1cs as linear maps, every point array of the key against the powers of tau.  Declarations
# only: the caller fills the two descriptions from its own r1cs / ptau readers and draws the multipliers (nvars and
# 2^log2_domain of them, 16 bytes each, none zero) from the OS CSPRNG as auditKey does.
const
  G16_PTAU_SECTIONS* = 5
  G16_CIRCUIT_RELATIONS* = 9
  ptauSectionNames* = ["tauG1", "tauG2", "alphaTauG1", "betaTauG1", "betaG2"]
  circuitRelationNames* = ["COEFFS_A", "COEFFS_B", "SPEC", "A1", "B1", "B2", "C1", "IC", "H1"]
type
  G16R1csDesc* {.importc: "g16_r1cs_desc", header: "g16hip.h".} = object
    nvars*, npubs*, nconstraints*, flavour*: uint32
    row*, col*: array[3, ptr uint32]
    val*: array[3, pointer]
    nnz*: array[3, csize_t]
    flags*: uint32
  G16PtauDesc* {.importc: "g16_ptau_desc", header: "g16hip.h".} = object
    power*: uint32
    tauG1*, tauG2*, alphaTauG1*, betaTauG1*, betaG2*: pointer
  CircuitReport* {.importc: "g16_circuit_report", header: "g16hip.h".} = object
    key*: KeyReport
    ptau_first_bad*: array[G16_PTAU_SECTIONS, array[3, csize_t]]
    ptau_bad_count*: array[G16_PTAU_SECTIONS, array[3, csize_t]]
    relation*: array[G16_CIRCUIT_RELATIONS, int32]   ## 1 holds, 0 fails, -1 not run
    failed*: uint32                                   ## OR of G16_CIRCUIT_*: 0 = belongs to the circuit and the ptau
    first_row*: array[2, csize_t]                     ## COEFFS_A / COEFFS_B: first differing row, high(csize_t) = none

proc g16_circuit_audit(ctx: ptr G16Ctx, desc: ptr G16PKeyDesc, vk: ptr G16VKeyDesc, section4: pointer,
                       section4Bytes: csize_t, r1cs: ptr G16R1csDesc, ptau: ptr G16PtauDesc, wireMultipliers,
                       hMultipliers: pointer, res: ptr CircuitReport): int32 {.importc, header: "g16hip.h".}

proc ok*(r: CircuitReport): bool = r.failed == 0

# --- witness check (include/g16hip.h "witness check"): which constraints does an untrusted witness break? ---------------
# What `snarkjs wtns check circuit.r1cs witness.wtns` answers: every value < r, witness[0] == 1, and
# (A z)_i (B z)_i == (C z)_i for every constraint.  A service loads the circuit once (loadR1cs), checks every witness
# (checkWitness) and proves only when the report is ok.  Like the rest of this shim it has NOT been compiled: no `nim` in
# the image; the same calls run through ctypes and through tools/g16prove.cpp in tests/test_gpu_witness_check.py.
# Needs `import groth16/files/r1cs` beside the imports above.
const
  G16_WITNESS_CANONICAL* = 1'u32     ## some value is >= r
  G16_WITNESS_ONE* = 2'u32           ## witness[0] is not 1
  G16_WITNESS_CONSTRAINTS* = 4'u32   ## some constraint fails
  G16_WITNESS_LIST* = 16
type
  G16R1cs {.importc: "g16_r1cs", header: "g16hip.h", incompleteStruct.} = object
  R1csSystem* = ptr G16R1cs
  WitnessReport* {.importc: "g16_witness_report", header: "g16hip.h".} = object
    failed*: uint32                                   ## OR of G16_WITNESS_*: 0 = fit to prove with
    constraints*: int32                               ## 1 all hold, 0 some fail, -1 not run (a value is not canonical)
    noncanonical_count*, first_noncanonical*: csize_t ## first: high(csize_t) = none
    bad_count*: csize_t
    first_bad*: array[G16_WITNESS_LIST, csize_t]      ## the smallest failing constraints, ascending; high(csize_t) = none
    az*, bz*, cz*: array[32, byte]                    ## the sums at first_bad[0]: little-endian, standard form

proc g16_r1cs_create(ctx: ptr G16Ctx, desc: ptr G16R1csDesc, res: ptr ptr G16R1cs): int32 {.importc, header: "g16hip.h".}
proc g16_r1cs_destroy(r: ptr G16R1cs) {.importc, header: "g16hip.h".}
proc g16_r1cs_info(r: ptr G16R1cs, res: ptr array[4, csize_t]): int32 {.importc, header: "g16hip.h".}
proc g16_witness_check(ctx: ptr G16Ctx, r: ptr G16R1cs, witness: pointer, flags: uint32,
                       res: ptr WitnessReport): int32 {.importc, header: "g16hip.h".}

proc ok*(r: WitnessReport): bool = r.failed == 0

proc loadR1cs*(r1cs: R1CS): R1csSystem =
  ## the circuit resident on the GPU; release it with destroyR1cs
  var rows, cols: array[3, seq[uint32]]
  var vals: array[3, seq[Fr]]
  for i, ct in r1cs.constraints:                            # files/r1cs.nim:62-80 -> triplets per matrix
    for k, lc in [ct.A, ct.B, ct.C]:
      for term in lc:
        rows[k].add(uint32(i)); cols[k].add(uint32(term.wireIdx)); vals[k].add(term.value)
  var d = G16R1csDesc(nvars: uint32(r1cs.cfg.nWires), npubs: uint32(r1cs.cfg.nPubOut + r1cs.cfg.nPubIn),
    nconstraints: uint32(r1cs.constraints.len), flavour: uint32(ord(Snarkjs)), flags: G16_SCALARS_MONT)
  for k in 0..2:
    d.nnz[k] = csize_t(rows[k].len)
    if rows[k].len > 0:
      d.row[k] = addr rows[k][0]; d.col[k] = addr cols[k][0]; d.val[k] = addr vals[k][0]
  check g16_r1cs_create(gctx, addr d, addr result)

proc destroyR1cs*(r: R1csSystem) = g16_r1cs_destroy(r)

proc checkWitness*(r: R1csSystem, witness: Witness): WitnessReport =
  ## witness.values: seq[Fr], Montgomery limbs in memory
  check g16_witness_check(gctx, r, unsafeAddr witness.values[0], G16_SCALARS_MONT, addr result)

# --- drop-in for fakeCircuitSetup (groth16/fake_setup.nim:201-326): one g16_fake_setup call ----------------------------
# The Lagrange values, the column sums, the combinations and the H scalars are formed on the device and stay in HBM; the
# points come back into the seqs of the ZKey.  ZKey.coeffs is the reference's own r1csToCoeffs (fake_setup.nim:46-65).
# Needs `import groth16/files/r1cs` and `import groth16/fake_setup` (ToxicWaste, r1csToCoeffs) beside the imports above.
type
  G16SetupDesc {.importc: "g16_setup_desc", header: "g16hip.h".} = object
    nvars, npubs, nconstraints, flavour: uint32
    row, col: array[3, ptr uint32]
    val: array[3, pointer]
    nnz: array[3, csize_t]
    flags: uint32
    alpha, beta, gamma, delta, tau: pointer
  G16SetupPoints {.importc: "g16_setup_points", header: "g16hip.h".} = object
    alpha1, beta1, delta1, beta2, gamma2, delta2: pointer
    pointsIC, pointsA1, pointsB1, pointsB2, pointsC1, pointsH1: pointer
proc g16_setup_log2_domain(desc: ptr G16SetupDesc, log2Domain: ptr uint32): int32 {.importc, header: "g16hip.h".}
proc g16_fake_setup(ctx: ptr G16Ctx, desc: ptr G16SetupDesc, res: ptr G16SetupPoints): int32 {.importc, header: "g16hip.h".}

proc fakeCircuitSetup*(r1cs: R1CS, toxic: ToxicWaste, flavour = Snarkjs): ZKey =
  let nvars = r1cs.cfg.nWires
  let npubs = r1cs.cfg.nPubOut + r1cs.cfg.nPubIn
  var rows, cols: array[3, seq[uint32]]
  var vals: array[3, seq[Fr]]
  for i, ct in r1cs.constraints:                            # files/r1cs.nim:62-80 -> triplets per matrix
    for k, lc in [ct.A, ct.B, ct.C]:
      for term in lc:
        rows[k].add(uint32(i)); cols[k].add(uint32(term.wireIdx)); vals[k].add(term.value)
  var d = G16SetupDesc(nvars: uint32(nvars), npubs: uint32(npubs), nconstraints: uint32(r1cs.constraints.len),
    flavour: uint32(ord(flavour)), flags: G16_SCALARS_MONT,
    alpha: unsafeAddr toxic.alpha, beta: unsafeAddr toxic.beta, gamma: unsafeAddr toxic.gamma,
    delta: unsafeAddr toxic.delta, tau: unsafeAddr toxic.tau)
  for k in 0..2:
    d.nnz[k] = csize_t(rows[k].len)
    if rows[k].len > 0:
      d.row[k] = addr rows[k][0]; d.col[k] = addr cols[k][0]; d.val[k] = addr vals[k][0]
  var logDom: uint32
  check g16_setup_log2_domain(addr d, addr logDom)
  let domSize = 1 shl int(logDom)
  var spec: SpecPoints
  var ic = newSeq[G1](npubs + 1)
  var pts = ProverPoints(pointsA1: newSeq[G1](nvars), pointsB1: newSeq[G1](nvars), pointsB2: newSeq[G2](nvars),
                         pointsC1: newSeq[G1](max(nvars - npubs - 1, 1)), pointsH1: newSeq[G1](domSize))
  var o = G16SetupPoints(alpha1: addr spec.alpha1, beta1: addr spec.beta1, delta1: addr spec.delta1,
    beta2: addr spec.beta2, gamma2: addr spec.gamma2, delta2: addr spec.delta2, pointsIC: addr ic[0],
    pointsA1: addr pts.pointsA1[0], pointsB1: addr pts.pointsB1[0], pointsB2: addr pts.pointsB2[0],
    pointsC1: addr pts.pointsC1[0], pointsH1: addr pts.pointsH1[0])
  check g16_fake_setup(gctx, addr d, addr o)                # tau inside the domain: the reference's assert, poly.nim:245
  pts.pointsC1.setLen(nvars - npubs - 1)
  spec.alphaBeta = pairing(spec.alpha1, spec.beta2)         # fake_setup.nim: the verifier-only pairing value
  let header = GrothHeader(curve: "bn128", flavour: flavour, p: primeP, r: primeR, nvars: nvars, npubs: npubs,
                           domainSize: domSize, logDomainSize: int(logDom))
  return ZKey(header: header, specPoints: spec, vPoints: VerifierPoints(pointsIC: ic), pPoints: pts,
              coeffs: r1csToCoeffs(r1cs))

# --- real circuit setup (include/g16hip.h "circuit setup"): the key of `snarkjs zkey new circuit.r1cs pot.ptau` ----------
# One g16_circuit_setup call from the R1CS and the powers of tau of a ceremony (sections 2-6 of the .ptau, which the
# caller's reader hands over as a G16PtauDesc: Montgomery affine points, power >= log2 of the domain + 1); no toxic waste.
# gamma = 1, and delta = 1 unless one is given: such a key is sound only after a phase-2 contribution.  For the powers of
# a known tau it is fakeCircuitSetup's key for (alpha, beta, 1, delta, tau), byte for byte.
proc g16_points_intt_g1(ctx: ptr G16Ctx, points: pointer, log2n: uint32, res: pointer): int32 {.importc, header: "g16hip.h".}
proc g16_points_intt_g2(ctx: ptr G16Ctx, points: pointer, log2n: uint32, res: pointer): int32 {.importc, header: "g16hip.h".}
proc g16_circuit_setup(ctx: ptr G16Ctx, r1cs: ptr G16R1csDesc, ptau: ptr G16PtauDesc, delta: pointer,
                       res: ptr G16SetupPoints): int32 {.importc, header: "g16hip.h".}

## out[k] = sum_j (omega^(-jk) / n) points[j]: the inverse NTT with curve points for elements; points.len a power of two
proc pointsInverseNTT*(points: seq[G1]): seq[G1] =
  result = newSeq[G1](points.len)
  var log2n = 0'u32
  while (1 shl int(log2n)) < points.len: inc log2n
  doAssert (1 shl int(log2n)) == points.len, "a power-of-two number of points"
  check g16_points_intt_g1(gctx, unsafeAddr points[0], log2n, addr result[0])
proc pointsInverseNTT*(points: seq[G2]): seq[G2] =
  result = newSeq[G2](points.len)
  var log2n = 0'u32
  while (1 shl int(log2n)) < points.len: inc log2n
  doAssert (1 shl int(log2n)) == points.len, "a power-of-two number of points"
  check g16_points_intt_g2(gctx, unsafeAddr points[0], log2n, addr result[0])

proc circuitSetup*(r1cs: R1CS, ptau: G16PtauDesc, flavour = Snarkjs, delta: ptr Fr = nil): ZKey =
  let nvars = r1cs.cfg.nWires
  let npubs = r1cs.cfg.nPubOut + r1cs.cfg.nPubIn
  var rows, cols: array[3, seq[uint32]]
  var vals: array[3, seq[Fr]]
  for i, ct in r1cs.constraints:                            # files/r1cs.nim:62-80 -> triplets per matrix
    for k, lc in [ct.A, ct.B, ct.C]:
      for term in lc:
        rows[k].add(uint32(i)); cols[k].add(uint32(term.wireIdx)); vals[k].add(term.value)
  var d = G16R1csDesc(nvars: uint32(nvars), npubs: uint32(npubs), nconstraints: uint32(r1cs.constraints.len),
    flavour: uint32(ord(flavour)), flags: G16_SCALARS_MONT)
  for k in 0..2:
    d.nnz[k] = csize_t(rows[k].len)
    if rows[k].len > 0:
      d.row[k] = addr rows[k][0]; d.col[k] = addr cols[k][0]; d.val[k] = addr vals[k][0]
  var logDom = 0
  while (1 shl logDom) < r1cs.constraints.len + npubs + 1: inc logDom     # ceilingLog2, as g16_setup_log2_domain
  let domSize = 1 shl logDom
  var spec: SpecPoints
  var ic = newSeq[G1](npubs + 1)
  var pts = ProverPoints(pointsA1: newSeq[G1](nvars), pointsB1: newSeq[G1](nvars), pointsB2: newSeq[G2](nvars),
                         pointsC1: newSeq[G1](max(nvars - npubs - 1, 1)), pointsH1: newSeq[G1](domSize))
  var o = G16SetupPoints(alpha1: addr spec.alpha1, beta1: addr spec.beta1, delta1: addr spec.delta1,
    beta2: addr spec.beta2, gamma2: addr spec.gamma2, delta2: addr spec.delta2, pointsIC: addr ic[0],
    pointsA1: addr pts.pointsA1[0], pointsB1: addr pts.pointsB1[0], pointsB2: addr pts.pointsB2[0],
    pointsC1: addr pts.pointsC1[0], pointsH1: addr pts.pointsH1[0])
  var pd = ptau
  check g16_circuit_setup(gctx, addr d, addr pd, delta, addr o)
  pts.pointsC1.setLen(nvars - npubs - 1)
  spec.alphaBeta = pairing(spec.alpha1, spec.beta2)
  let header = GrothHeader(curve: "bn128", flavour: flavour, p: primeP, r: primeR, nvars: nvars, npubs: npubs,
                           domainSize: domSize, logDomainSize: logDom)
  return ZKey(header: header, specPoints: spec, vPoints: VerifierPoints(pointsIC: ic), pPoints: pts,
              coeffs: r1csToCoeffs(r1cs))

# --- phase-2 contribution (include/g16hip.h "scaling an array of points", "phase-2 contribution") -------------------------
# Declarations only.  g16_key_contribute turns the key of circuitSetup (delta = 1) into a sound one; the library hashes and
# draws nothing: the secrets and the challenge point are the caller's, and the transcript rule of the Python package
# (nim_groth16_amd/phase2.py) is the project's own, not snarkjs's.
type
  G16Phase2Key* {.importc: "g16_phase2_key", header: "g16hip.h", bycopy.} = object
    delta1*, delta2*, pointsC1*, pointsH1*: pointer
    nc1*, nh1*: csize_t
  G16Contribution* {.importc: "g16_contribution", header: "g16hip.h", bycopy.} = object
    delta_after*, g1_s*, g1_sx*: array[64, uint8]
    g2_spx*: array[128, uint8]
  G16Phase2Out* {.importc: "g16_phase2_out", header: "g16hip.h", bycopy.} = object
    delta1*, delta2*, pointsC1*, pointsH1*: pointer
    record*: ptr G16Contribution
  G16ChainReport* {.importc: "g16_chain_report", header: "g16hip.h", bycopy.} = object
    failed*: uint32
    relation*: array[7, int32]
    first_record*: array[2, csize_t]
    first_bad*, bad_count*: array[9, array[3, csize_t]]
    first_infinity*: array[9, csize_t]
proc g16_points_scale_g1(ctx: ptr G16Ctx, points: pointer, n: csize_t, k: pointer, flags: uint32,
                         res: pointer): int32 {.importc, header: "g16hip.h".}
proc g16_points_scale_g2(ctx: ptr G16Ctx, points: pointer, n: csize_t, k: pointer, flags: uint32,
                         res: pointer): int32 {.importc, header: "g16hip.h".}
proc g16_key_contribute(ctx: ptr G16Ctx, key: ptr G16Phase2Key, d, s: pointer, flags: uint32, challenge_g2: pointer,
                        res: ptr G16Phase2Out): int32 {.importc, header: "g16hip.h".}
proc g16_contributions_verify(ctx: ptr G16Ctx, initial, final: ptr G16Phase2Key, records: ptr G16Contribution,
                              challenges_g2: pointer, count: csize_t, c1_multipliers, h1_multipliers: pointer,
                              res: ptr G16ChainReport): int32 {.importc, header: "g16hip.h".}

# --- a scalar per point, and the phase-1 contribution (include/g16hip.h "scaling an array of points", "phase-1
# contribution") ---------------------------------------------------------------------------------------------------------
# g16_ptau_contribute takes the powers of (tau, alpha, beta) to those of (t tau, a alpha, b beta).  As in phase 2 the library
# hashes and draws nothing; the transcript rule of nim_groth16_amd/phase1.py is the project's own, not snarkjs's.
# g16_ptau_verify checks a .ptau and a chain of such records under caller-drawn 128-bit multipliers.
type
  G16PtauOut* {.importc: "g16_ptau_out", header: "g16hip.h", bycopy.} = object
    tauG1*, tauG2*, alphaTauG1*, betaTauG1*, betaG2*: pointer
  G16PtauPok* {.importc: "g16_ptau_pok", header: "g16hip.h", bycopy.} = object
    g1_s*, g1_sx*: array[64, uint8]
    g2_spx*: array[128, uint8]
  G16PtauContribution* {.importc: "g16_ptau_contribution", header: "g16hip.h", bycopy.} = object
    tauG1*, alphaG1*, betaG1*: array[64, uint8]
    tauG2*, betaG2*: array[128, uint8]
    pok*: array[3, G16PtauPok]
proc g16_points_scale_each_g1(ctx: ptr G16Ctx, points: pointer, n: csize_t, scalars: pointer, flags: uint32,
                              res: pointer): int32 {.importc, header: "g16hip.h".}
proc g16_points_scale_each_g2(ctx: ptr G16Ctx, points: pointer, n: csize_t, scalars: pointer, flags: uint32,
                              res: pointer): int32 {.importc, header: "g16hip.h".}
proc g16_ptau_contribute(ctx: ptr G16Ctx, ptau: ptr G16PtauDesc, t, a, b, s3: pointer, flags: uint32,
                         challenges_g2: pointer, res: ptr G16PtauOut, record: ptr G16PtauContribution): int32 {.
                         importc, header: "g16hip.h".}

proc scaleEach*(points: seq[G1], scalars: seq[Fr]): seq[G1] =
  ## res[i] = scalars[i] * points[i]; the points on the curve, (0,0) anywhere
  assert points.len == scalars.len
  result = newSeq[G1](points.len)
  if points.len > 0:
    check g16_points_scale_each_g1(gctx, unsafeAddr points[0], csize_t(points.len), unsafeAddr scalars[0],
                                   G16_SCALARS_MONT, addr result[0])

proc scaleEach*(points: seq[G2], scalars: seq[Fr]): seq[G2] =
  assert points.len == scalars.len
  result = newSeq[G2](points.len)
  if points.len > 0:
    check g16_points_scale_each_g2(gctx, unsafeAddr points[0], csize_t(points.len), unsafeAddr scalars[0],
                                   G16_SCALARS_MONT, addr result[0])

proc ptauContribute*(ptau: G16PtauDesc, t, a, b: Fr, pokSecrets: array[3, Fr], challenges: array[3, G2],
                     res: G16PtauOut): G16PtauContribution =
  ## one phase-1 contribution into the caller's buffers `res` (sized as the arrays of `ptau`); the six scalars are
  ## non-zero, the three challenge points the caller's (for t, a, b in this order).  Returns the record.
  var o = res
  check g16_ptau_contribute(gctx, unsafeAddr ptau, unsafeAddr t, unsafeAddr a, unsafeAddr b, unsafeAddr pokSecrets[0],
                            G16_SCALARS_MONT, unsafeAddr challenges[0], addr o, addr result)

type
  G16PtauReport* {.importc: "g16_ptau_report", header: "g16hip.h", bycopy.} = object
    failed*: uint32
    relation*: array[10, int32]
    first_record*: array[2, csize_t]
    first_bad*, bad_count*: array[14, array[3, csize_t]]
    first_infinity*: array[14, csize_t]
proc g16_ptau_verify(ctx: ptr G16Ctx, ptau: ptr G16PtauDesc, records: ptr G16PtauContribution, challenges_g2: pointer,
                     count: csize_t, multipliers: pointer, res: ptr G16PtauReport): int32 {.importc, header: "g16hip.h".}

proc ptauVerify*(ptau: G16PtauDesc, records: seq[G16PtauContribution], challenges: seq[G2], multipliers: seq[array[16, uint8]],
                 checkChain = true): G16PtauReport =
  ## is `ptau` the powers of some tau, alpha, beta, and (checkChain) do the records lead to it from the generators?
  ## challenges: three per record; multipliers: 2^(power+1) - 2 non-zero 128-bit values drawn by the caller
  assert challenges.len == 3 * records.len and multipliers.len == (2 shl ptau.power.int) - 2
  var one: G16PtauContribution
  let recs = if not checkChain: nil elif records.len > 0: unsafeAddr records[0] else: addr one
  check g16_ptau_verify(gctx, unsafeAddr ptau, recs, (if records.len > 0: unsafeAddr challenges[0] else: nil),
                        csize_t(if checkChain: records.len else: 0), unsafeAddr multipliers[0], addr result)
