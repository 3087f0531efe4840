#!/usr/bin/env python3
"""Prove from circom/snarkjs artifacts on the GPU (the `-p` path of the reference CLI, cli/cli_main.nim:162-231):
    python tools/prove_files.py --zkey circuit.zkey --wtns witness.wtns -o proof.json -i public.json [-k vkey.json] [-y] [-c]
The outputs are snarkjs-compatible (`snarkjs groth16 verify vkey.json public.json proof.json`).

BASELINE config 5 hand-off (a real circom Poseidon-Merkle .zkey cannot be produced in the build container: no circom,
snarkjs, ptau or network).  Given external files the checked recipe is
    python tools/prove_files.py -z circuit.zkey -w witness.wtns -c -y -t -k verification_key.json
      -c  every point of the key is checked to be on its curve on the GPU (the mkG1 / mkG2 asserts of the reference's
          loaders, curves.nim:95-107) and the witness is checked against the key's header
      -y  the proof is verified on the GPU against the key's own verification key (verifier.nim:31-52)
      -t  phase timings, and the fraction of points at infinity per ProverPoints array together with whether the
          library put A1 / B1+B2 on compacted entry lists (g16_pkey_inf_counts)
      --audit  for a key from a third party: before it is loaded, every section is audited on the GPU (auditZKey:
          canonical encodings, curve, order-r subgroup, coefficient values, the B1/B2, beta and delta relations);
          findings are printed, and a key that fails gives exit code 2 and no proof
      --audit-circuit R1CS PTAU  the same and more: the key must also belong to this circuit and this powers of tau
          (auditCircuit: the key's coefficients against the r1cs, every point array against the ptau -- what
          `snarkjs zkey verify` checks before the contribution chain); exit code 2 and no proof otherwise
      --setup-ptau PTAU -r R1CS  first make the key: the circuit setup of `snarkjs zkey new` on the GPU (circuitSetup:
          gamma = delta = 1, sound only after a phase-2 contribution) written to the --zkey path; without --wtns the
          run ends there, with it the proof is made from the new key
      --contribute [--contribute-name N] [--contribute-out OUT]  one phase-2 contribution to the --zkey key (setup.contribute:
          fresh secrets from `secrets`, forgotten when the process ends; the transcript rule is this project's own, not
          snarkjs's: nim_groth16_amd/phase2.py), written with its log (section 10) to OUT, by default back to the --zkey
          path; without --wtns the run ends there, with it the proof is made from the contributed key
      --verify-contributions INITIAL.zkey  before the key is loaded: do the records of its section 10 lead from the
          initial key (the caller's anchor: made with --setup-ptau or tied to its circuit with --audit-circuit) to this
          key?  The report is printed; a chain that fails gives exit code 2 and no proof, like --audit-circuit
      --check-witness R1CS  before proving: is every witness value < r, is witness[0] one, and which constraints of this
          circuit does the witness break (witnessCheck: `snarkjs wtns check` on the GPU)?  The findings are printed with
          the constraint indices; a witness that fails gives exit code 2 and no proof
    snarkjs groth16 verify verification_key.json public.json proof.json        # offline, wherever snarkjs exists
(the reference's own recipe: groth16/example/prove.sh:52-59)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import secrets  # noqa: E402

from nim_groth16_amd import Context, Mask, generateProofWithMask, loadProvingKey  # noqa: E402
from nim_groth16_amd import bn128 as F  # noqa: E402
from nim_groth16_amd.files import exportProof, exportPublicIO, parseWitness, parseZKey  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-z", "--zkey", required=True)
    ap.add_argument("-w", "--wtns", default=None, help="required unless --setup-ptau only makes the key")
    ap.add_argument("--setup-ptau", metavar="PTAU", default=None,
                    help="make the key from -r R1CS and this powers of tau and write it to --zkey (then prove, if a "
                         "witness is given)")
    ap.add_argument("-r", "--r1cs", default=None, help="the circuit of --setup-ptau")
    ap.add_argument("-o", "--output", default="proof.json")
    ap.add_argument("-i", "--io", default="public.json")
    ap.add_argument("-n", "--nomask", action="store_true", help="trivial mask r = s = 0 (cli_main.nim -n)")
    ap.add_argument("-t", "--time", action="store_true")
    ap.add_argument("--table-stride", type=int, default=0,
                    help="a lean key: window tables for every S-th window only (about 1 / S of the HBM, same proof)")
    ap.add_argument("-k", "--vkey", default=None, help="also write the verification key as snarkjs verification_key.json")
    ap.add_argument("-c", "--check", action="store_true",
                    help="check every key point against its curve equation on the GPU while parsing")
    ap.add_argument("--audit", action="store_true",
                    help="audit the key on the GPU before loading it; no proof from a key that fails")
    ap.add_argument("--audit-circuit", nargs=2, metavar=("R1CS", "PTAU"), default=None,
                    help="audit the key against its circuit and powers of tau before loading it; no proof from a key "
                         "that does not belong to them")
    ap.add_argument("--contribute", action="store_true",
                    help="make one phase-2 contribution to the key and write it (see --contribute-out)")
    ap.add_argument("--contribute-name", default="", help="the name recorded with the contribution")
    ap.add_argument("--contribute-out", metavar="OUT", default=None,
                    help="where --contribute writes the contributed key (default: back to the --zkey path)")
    ap.add_argument("--verify-contributions", metavar="INITIAL", default=None,
                    help="check the key's contribution chain against this initial key before loading it; no proof from "
                         "a key whose chain fails")
    ap.add_argument("--check-witness", metavar="R1CS", default=None,
                    help="check the witness against this circuit on the GPU before proving; no proof from a witness that "
                         "is not canonical or breaks a constraint")
    ap.add_argument("-y", "--verify", action="store_true",
                    help="also verify the proof against the zkey's verification key (cli_main.nim -y)")
    args = ap.parse_args()
    ctx = Context(0)
    ctx.selftest()
    if args.setup_ptau:
        if not args.r1cs:
            ap.error("--setup-ptau goes together with -r R1CS")
        from nim_groth16_amd.files import parsePtau, parseR1CS, writeZKey
        from nim_groth16_amd.setup import circuitSetup
        ts = time.time()
        writeZKey(args.zkey, circuitSetup(parseR1CS(args.r1cs), parsePtau(args.setup_ptau), ctx=ctx))
        print(f"circuit setup: wrote {args.zkey}" + (f" ({time.time() - ts:.3f}s)" if args.time else ""))
        if not args.wtns:
            return
    elif args.r1cs:
        ap.error("-r R1CS goes together with --setup-ptau")
    if args.contribute:
        from nim_groth16_amd.files import parseContributions, writeZKey
        from nim_groth16_amd.setup import contribute
        zk = parseZKey(args.zkey, ctx=ctx, rawCoeffs=True)
        zk.contributions = parseContributions(args.zkey)
        out = args.contribute_out or args.zkey
        done = contribute(zk, name=args.contribute_name, ctx=ctx)
        writeZKey(out, done)
        print(f"contribution {len(done.contributions.records)}" +
              (f" ({args.contribute_name})" if args.contribute_name else "") + f": wrote {out}")
        args.zkey = out
        if not args.wtns and not args.verify_contributions:
            return
    if args.verify_contributions:
        from nim_groth16_amd.files import parseContributions
        from nim_groth16_amd.setup import verifyContributions
        zk = parseZKey(args.zkey, ctx=ctx, rawCoeffs=True)
        zk.contributions = parseContributions(args.zkey)
        try:
            report = verifyContributions(parseZKey(args.verify_contributions, ctx=ctx, rawCoeffs=True), zk, ctx=ctx)
        except ValueError as e:                  # a part of the key that no contribution touches differs
            print(f"contribution chain: FAILED\n  {e}")
            raise SystemExit(2)
        print(report)
        if not report.ok:
            raise SystemExit(2)
        if not args.wtns:
            return
    if not args.wtns:
        ap.error("the following arguments are required: -w/--wtns")
    t0 = time.time()
    zkey, wtns = parseZKey(args.zkey, check=args.check, ctx=ctx, rawCoeffs=True), parseWitness(args.wtns)
    assert wtns.nvars == zkey.header.nvars, "wrong witness length"        # prover.nim:236
    if args.audit:
        from nim_groth16_amd.files import auditZKey
        report = auditZKey(zkey, ctx)
        print(report)
        if not report.ok:
            raise SystemExit(2)
    if args.audit_circuit:
        from nim_groth16_amd.files import auditCircuit, parsePtau, parseR1CS
        report = auditCircuit(zkey, parseR1CS(args.audit_circuit[0]), parsePtau(args.audit_circuit[1]), ctx)
        print(report)
        if not report.ok:
            raise SystemExit(2)
    if args.check_witness:
        from nim_groth16_amd import witnessCheck
        from nim_groth16_amd.files import parseR1CS
        report = witnessCheck(parseR1CS(args.check_witness), wtns, ctx)
        print(report)
        if not report.ok:
            raise SystemExit(2)
    t1 = time.time()
    pkey = loadProvingKey(zkey, ctx, table_stride=args.table_stride)
    t2 = time.time()
    mask = Mask(0, 0) if args.nomask else Mask(secrets.randbelow(F.primeR), secrets.randbelow(F.primeR))
    proof = generateProofWithMask(0, args.time, zkey, wtns, mask, ctx, pkey=pkey)
    t3 = time.time()
    exportProof(args.output, proof)
    exportPublicIO(args.io, proof)
    if args.vkey:
        from nim_groth16_amd import extractVKey
        from nim_groth16_amd.files import exportVKey
        exportVKey(args.vkey, extractVKey(zkey))
    if args.verify:
        from nim_groth16_amd import extractVKey, verifyProof
        ok = verifyProof(extractVKey(zkey), proof, ctx)
        print("verification " + ("succeeded" if ok else "FAILED"))
        if not ok:
            raise SystemExit(1)
    if args.time:
        print(f"parsing {t1-t0:.3f}s | key upload + tables {t2-t1:.3f}s | proof {t3-t2:.3f}s")
        hdr, inf = zkey.header, pkey.inf_counts()
        sizes = {"A1": hdr.nvars, "B1": hdr.nvars, "B2": hdr.nvars, "C1": hdr.nvars - hdr.npubs - 1, "H1": hdr.domainSize}
        print("points at infinity (0,0): " + ", ".join(f"{k} {inf[k]}/{n} ({100.0 * inf[k] / max(n, 1):.1f} %)"
                                                      for k, n in sizes.items()))
        print(f"entry lists: A1 {'compacted' if inf['compact_A'] else 'shared witness sort'}, B1+B2 "
              f"{'compacted (their own sort without the ' + str(inf['B1_and_B2']) + ' dead wires)' if inf['compact_B'] else 'shared witness sort'}")


if __name__ == "__main__":
    main()
