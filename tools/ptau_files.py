#!/usr/bin/env python3
"""Phase 1 of a ceremony on `.ptau` files, with no toxic waste in any command:
    python tools/ptau_files.py new POWER -o pot_0000.ptau
    python tools/ptau_files.py contribute pot_0000.ptau -o pot_0001.ptau [--name alice]
`new` writes the file of generators (tau = alpha = beta = 1).  `contribute` draws t, a, b and the three proof-of-knowledge
secrets with `secrets`, forgets them when the process ends, multiplies the powers on the GPU (g16_ptau_contribute) and
appends its record to the log in section 7.  The transcript rule is this project's own, not snarkjs's
(nim_groth16_amd/phase1.py); sections 2-6 are a plain .ptau, so the result goes straight to
    python tools/prove_files.py --setup-ptau pot_0002.ptau -r circuit.r1cs -z circuit.zkey
    python tools/ptau_files.py verify pot_0002.ptau
`verify` checks the powers and the chain of records in section 7 on the GPU (g16_ptau_verify, multipliers from `secrets`),
prints the report and exits with 2 when anything fails."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nim_groth16_amd import phase1  # noqa: E402
from nim_groth16_amd.files import contributionsSection, parsePtau, parsePtauContributions, writePtau  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    p_new = sub.add_parser("new", help="the file of generators")
    p_new.add_argument("power", type=int)
    p_new.add_argument("-o", "--out", required=True)
    p_con = sub.add_parser("contribute", help="one contribution with fresh secrets")
    p_con.add_argument("ptau")
    p_con.add_argument("-o", "--out", required=True)
    p_con.add_argument("--name", default="")
    p_ver = sub.add_parser("verify", help="check the powers and the chain of records; exit code 2 when anything fails")
    p_ver.add_argument("ptau")
    args = ap.parse_args(argv)
    if args.cmd == "new":
        try:
            ptau = phase1.newPtau(args.power)
        except ValueError as e:
            ap.error(str(e))
        writePtau(args.out, ptau, extraSections=[(7, contributionsSection([], []))])
        print(f"new: wrote {args.out} (power {args.power}, every element its generator, no contribution)")
        return 0
    ptau = parsePtau(args.ptau)
    got = parsePtauContributions(args.ptau)
    log = phase1.PtauContributions(power=ptau.power, records=list(got[0]), names=list(got[1])) if got else None
    if args.cmd == "verify":
        rep = phase1.verifyPtau(ptau, log)
        print(f"{args.ptau}: power {ptau.power}, " + (f"{len(log.records)} records" if log else "no contribution log (chain not checked)"))
        print(rep)
        print("ptau: ok" if rep.ok else "ptau: FAILED")
        return 0 if rep.ok else 2
    ptau, log = phase1.contribute(ptau, log, name=args.name)
    writePtau(args.out, ptau, extraSections=[(7, contributionsSection(log.records, log.names))])
    label = f" ({args.name})" if args.name else ""
    print(f"contribution {len(log.records)}{label}: wrote {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
