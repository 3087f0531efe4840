"""ctypes binding of libg16hip.so (include/g16hip.h).  Fails loudly when the library is missing."""
from __future__ import annotations

import ctypes
import json
import os
import weakref

_HERE = os.path.dirname(os.path.abspath(__file__))

_R = 21888242871839275222246405745257275088548364400416034343698204186575808495617   # the order of Fr (bn128.primeR)
G16_OK, G16_EINVAL, G16_ENODEV, G16_EHIP, G16_ENOMEM, G16_ESELFTEST, G16_EBUSY = 0, -1, -2, -3, -4, -5, -6
SCALARS_MONT, SCALARS_STD, SCALARS_DEVICE, OUT_PARTIAL, OUT_DEVICE, NO_HOST_SYNC = 1, 0, 2, 4, 8, 32
PARTIALS_BYTES = 768

# every symbol include/g16hip.h declares (checked by tests/test_abi.py)
SYMBOLS = [
    "g16_ctx_create", "g16_ctx_destroy", "g16_last_error", "g16_ctx_set_stream", "g16_ctx_synchronize",
    "g16_selftest", "g16_msm_g1", "g16_msm_g2", "g16_msm_g1_dev", "g16_msm_g2_dev",
    "g16_msm_g1_partial_dev", "g16_msm_g2_partial_dev", "g16_g1_sum_partials", "g16_g2_sum_partials",
    "g16_points_register_g1", "g16_points_register_g2", "g16_points_register_g1_dev",
    "g16_points_register_g2_dev", "g16_points_release", "g16_points_count", "g16_points_inf_count", "g16_points_info", "g16_msm_points",
    "g16_points_check_g1", "g16_points_check_g2", "g16_fixed_base_g1", "g16_fixed_base_g2", "g16_quotient", "g16_quotient_dev", "g16_pkey_create",
    "g16_pkey_create_zkey", "g16_pkey_destroy", "g16_pkey_inf_counts", "g16_prove", "g16_build_abc", "g16_pkey_abc_info", "g16_spmv_fr", "g16_prove_partials", "g16_prove_combine",
    "g16_prove_partials_begin", "g16_prove_partials_end",
    "g16_ntt_fr", "g16_ntt_fr_dev", "g16_profile_enable", "g16_profile_reset", "g16_profile_report", "g16_profile_clock",
    "g16_vkey_create", "g16_vkey_destroy", "g16_verify", "g16_verify_batch", "g16_pairing",
    "g16_ctx_cancel", "g16_group_create", "g16_group_destroy", "g16_group_size", "g16_group_last_error",
    "g16_group_pkey_create", "g16_group_pkey_destroy", "g16_group_prove",
    "g16_prover_create", "g16_prover_destroy", "g16_prover_last_error", "g16_prover_submit", "g16_prover_poll",
    "g16_prover_collect", "g16_host_alloc", "g16_host_free",
    "g16_points_register_g1_lean", "g16_points_register_g2_lean", "g16_points_register_g1_lean_dev",
    "g16_points_register_g2_lean_dev", "g16_points_table_bytes", "g16_points_plan", "g16_pkey_create_lean",
    "g16_pkey_create_zkey_lean", "g16_group_pkey_create_lean",
    "g16_setup_log2_domain", "g16_fake_setup", "g16_lagrange_fr", "g16_powers_fr",
    "g16_points_audit_g1", "g16_points_audit_g2", "g16_points_pairs_check", "g16_key_audit",
    "g16_pkey_b1_fold", "g16_pkey_b1_sparse", "g16_circuit_audit",
    "g16_points_intt_g1", "g16_points_intt_g2", "g16_circuit_setup",
    "g16_points_scale_g1", "g16_points_scale_g2", "g16_points_scale_each_g1", "g16_points_scale_each_g2",
    "g16_key_contribute", "g16_contributions_verify", "g16_ptau_contribute", "g16_ptau_verify",
    "g16_r1cs_create", "g16_r1cs_destroy", "g16_r1cs_info", "g16_witness_check",
]
VERIFY_SUBGROUP = 16
GT_BYTES = 384


class PkeyDesc(ctypes.Structure):
    """g16_pkey_desc (include/g16hip.h)"""
    _fields_ = [("nvars", ctypes.c_uint32), ("npubs", ctypes.c_uint32), ("log2_domain", ctypes.c_uint32),
                ("flavour", ctypes.c_uint32),
                ("pointsA1", ctypes.c_void_p), ("pointsB1", ctypes.c_void_p), ("pointsB2", ctypes.c_void_p),
                ("pointsC1", ctypes.c_void_p), ("pointsH1", ctypes.c_void_p),
                ("coeffs", ctypes.c_void_p), ("ncoeffs", ctypes.c_size_t),
                ("alpha1", ctypes.c_void_p), ("beta1", ctypes.c_void_p), ("delta1", ctypes.c_void_p),
                ("beta2", ctypes.c_void_p), ("delta2", ctypes.c_void_p),
                ("shard_index", ctypes.c_uint32), ("shard_count", ctypes.c_uint32)]


class VkeyDesc(ctypes.Structure):
    """g16_vkey_desc (include/g16hip.h)"""
    _fields_ = [("npubs", ctypes.c_uint32), ("alpha1", ctypes.c_void_p), ("beta2", ctypes.c_void_p),
                ("gamma2", ctypes.c_void_p), ("delta2", ctypes.c_void_p), ("pointsIC", ctypes.c_void_p)]


class SetupDesc(ctypes.Structure):
    """g16_setup_desc (include/g16hip.h)"""
    _fields_ = [("nvars", ctypes.c_uint32), ("npubs", ctypes.c_uint32), ("nconstraints", ctypes.c_uint32),
                ("flavour", ctypes.c_uint32),
                ("row", ctypes.c_void_p * 3), ("col", ctypes.c_void_p * 3), ("val", ctypes.c_void_p * 3),
                ("nnz", ctypes.c_size_t * 3), ("flags", ctypes.c_uint32),
                ("alpha", ctypes.c_void_p), ("beta", ctypes.c_void_p), ("gamma", ctypes.c_void_p),
                ("delta", ctypes.c_void_p), ("tau", ctypes.c_void_p)]


SETUP_POINTS = ("alpha1", "beta1", "delta1", "beta2", "gamma2", "delta2", "pointsIC", "pointsA1", "pointsB1", "pointsB2",
                "pointsC1", "pointsH1")


class SetupPoints(ctypes.Structure):
    """g16_setup_points (include/g16hip.h)"""
    _fields_ = [(name, ctypes.c_void_p) for name in SETUP_POINTS]


# key audit (include/g16hip.h): the sections of a report in order, the checks in precedence, the bits of `failed`
AUDIT_SECTIONS = ("alpha1", "beta1", "delta1", "beta2", "gamma2", "delta2", "pointsIC", "pointsA1", "pointsB1", "pointsB2",
                  "pointsC1", "pointsH1", "coeffs")
AUDIT_CHECKS = ("canonical", "curve", "subgroup")
AUDIT_RELATIONS = ("pointsB1~pointsB2", "beta1~beta2", "delta1~delta2")
AUDIT_CANONICAL, AUDIT_CURVE, AUDIT_SUBGROUP, AUDIT_RELATION, AUDIT_SPEC_INFINITY = 1, 2, 4, 8, 16
# what an element that fails AUDIT_CHECKS[k] is said to be, in every report and error text (CHECK_TEXT, relation_plan.hpp)
CHECK_TEXTS = ("is not a canonical encoding", "is not on the curve", "is not in the order-r subgroup")


def _element_findings(names, first_bad, bad_count, first_infinity=None, prefix=""):
    """one line per first finding of the element passes over the arrays `names`: index and check, then the first (0,0)"""
    out = []
    for a, name in enumerate(names):
        for k, what in enumerate(CHECK_TEXTS):
            if bad_count[a][k]:
                more = bad_count[a][k] - 1
                out.append(f"{prefix}{name}[{first_bad[a][k]}] {what}" + (f" (and {more} more)" if more else ""))
        if first_infinity is not None and first_infinity[a] is not None:
            out.append(f"{prefix}{name}[{first_infinity[a]}] is the point at infinity")
    return out


class KeyReportC(ctypes.Structure):
    """g16_key_report (include/g16hip.h)"""
    _fields_ = [("failed", ctypes.c_uint32), ("spec_infinity", ctypes.c_uint32), ("relation", ctypes.c_int32 * 3),
                ("reserved", ctypes.c_uint32),
                ("first_bad", (ctypes.c_size_t * 3) * len(AUDIT_SECTIONS)),
                ("bad_count", (ctypes.c_size_t * 3) * len(AUDIT_SECTIONS))]


class KeyReport:
    """What g16_key_audit found.  first_bad[section][check] is an index or None, bad_count[section][check] a count;
    relation[k] is 1 (holds), 0 (fails) or -1 (not run) for AUDIT_RELATIONS[k]."""

    def __init__(self, failed, spec_infinity, relation, first_bad, bad_count):
        self.failed, self.spec_infinity, self.relation = failed, spec_infinity, list(relation)
        self.first_bad, self.bad_count = first_bad, bad_count

    @property
    def ok(self) -> bool:
        """fit to prove with"""
        return self.failed == 0

    def as_dict(self) -> dict:
        return {"failed": self.failed, "spec_infinity": self.spec_infinity, "relation": self.relation,
                "first_bad": self.first_bad, "bad_count": self.bad_count}

    def findings(self):
        """one line per first finding: section, index and check; failed relations; spec points at infinity"""
        out = _element_findings(AUDIT_SECTIONS, self.first_bad, self.bad_count)
        for k, name in enumerate(AUDIT_RELATIONS):
            if self.relation[k] == 0:
                out.append(f"{name}: not the same multiples of the two generators")
        for s in range(6):
            if self.spec_infinity >> s & 1:
                out.append(f"{AUDIT_SECTIONS[s]} is the point at infinity")
        return out

    def __str__(self):
        if self.ok:
            skipped = [AUDIT_RELATIONS[k] for k in range(3) if self.relation[k] < 0]
            return "key audit: ok" + (f" (not run: {', '.join(skipped)})" if skipped else "")
        return "key audit: FAILED\n" + "\n".join("  " + f for f in self.findings())


class R1csDesc(ctypes.Structure):
    """g16_r1cs_desc (include/g16hip.h): the first members of g16_setup_desc"""
    _fields_ = [("nvars", ctypes.c_uint32), ("npubs", ctypes.c_uint32), ("nconstraints", ctypes.c_uint32),
                ("flavour", ctypes.c_uint32),
                ("row", ctypes.c_void_p * 3), ("col", ctypes.c_void_p * 3), ("val", ctypes.c_void_p * 3),
                ("nnz", ctypes.c_size_t * 3), ("flags", ctypes.c_uint32)]


class PtauDesc(ctypes.Structure):
    """g16_ptau_desc (include/g16hip.h)"""
    _fields_ = [("power", ctypes.c_uint32), ("tauG1", ctypes.c_void_p), ("tauG2", ctypes.c_void_p),
                ("alphaTauG1", ctypes.c_void_p), ("betaTauG1", ctypes.c_void_p), ("betaG2", ctypes.c_void_p)]


# circuit audit (include/g16hip.h): the ptau arrays and the relations of a report in order, the bits of `failed`
PTAU_SECTIONS = ("tauG1", "tauG2", "alphaTauG1", "betaTauG1", "betaG2")
PTAU_GROUP = {"tauG1": 1, "tauG2": 2, "alphaTauG1": 1, "betaTauG1": 1, "betaG2": 2}
CIRCUIT_RELATIONS = ("COEFFS_A", "COEFFS_B", "SPEC", "A1", "B1", "B2", "C1", "IC", "H1")
CIRCUIT_KEY, CIRCUIT_PTAU, CIRCUIT_COEFFS, CIRCUIT_SPEC, CIRCUIT_POINTS = 1, 2, 4, 8, 16


class CircuitReportC(ctypes.Structure):
    """g16_circuit_report (include/g16hip.h)"""
    _fields_ = [("key", KeyReportC),
                ("ptau_first_bad", (ctypes.c_size_t * 3) * len(PTAU_SECTIONS)),
                ("ptau_bad_count", (ctypes.c_size_t * 3) * len(PTAU_SECTIONS)),
                ("relation", ctypes.c_int32 * len(CIRCUIT_RELATIONS)), ("failed", ctypes.c_uint32),
                ("first_row", ctypes.c_size_t * 2)]


class CircuitReport:
    """What g16_circuit_audit found: `key`, the KeyReport of the key on its own; ptau_first_bad / ptau_bad_count
    [array][check] for PTAU_SECTIONS as in a KeyReport; relation[k] = 1 (holds), 0 (fails) or -1 (not run) for
    CIRCUIT_RELATIONS[k]; first_row[m] = the first row where matrix A (m = 0) / B (m = 1) of the key and of the r1cs
    act differently on the multipliers, or None."""

    def __init__(self, key: KeyReport, ptau_first_bad, ptau_bad_count, relation, failed, first_row):
        self.key, self.ptau_first_bad, self.ptau_bad_count = key, ptau_first_bad, ptau_bad_count
        self.relation, self.failed, self.first_row = list(relation), failed, list(first_row)

    @property
    def ok(self) -> bool:
        """the key is fit to prove with and belongs to the circuit and the powers of tau"""
        return self.failed == 0

    def as_dict(self) -> dict:
        return {"key": self.key.as_dict(), "ptau_first_bad": self.ptau_first_bad, "ptau_bad_count": self.ptau_bad_count,
                "relation": self.relation, "failed": self.failed, "first_row": self.first_row}

    def findings(self):
        out = self.key.findings() + _element_findings(PTAU_SECTIONS, self.ptau_first_bad, self.ptau_bad_count, prefix="ptau ")
        for m in range(2):
            if self.relation[m] == 0:
                out.append(f"coeffs: matrix {'AB'[m]} differs from the r1cs first at row {self.first_row[m]}")
        if self.relation[2] == 0:
            out.append("alpha1 / beta1 / beta2 are not those of the powers of tau (or its first powers are not the generators)")
        for k in range(3, len(CIRCUIT_RELATIONS)):
            if self.relation[k] == 0:
                out.append(f"points{CIRCUIT_RELATIONS[k]} does not belong to the circuit")
        return out

    def __str__(self):
        if self.ok:
            skipped = [AUDIT_RELATIONS[k] for k in range(3) if self.key.relation[k] < 0]
            skipped += [CIRCUIT_RELATIONS[k] for k in range(len(CIRCUIT_RELATIONS)) if self.relation[k] < 0]
            return "circuit audit: ok" + (f" (not run: {', '.join(skipped)})" if skipped else "")
        return "circuit audit: FAILED\n" + "\n".join("  " + f for f in self.findings())


# witness check (include/g16hip.h): the bits of `failed`, the length of the list of failing constraints
WITNESS_CANONICAL, WITNESS_ONE, WITNESS_CONSTRAINTS = 1, 2, 4
WITNESS_LIST = 16


class WitnessReportC(ctypes.Structure):
    """g16_witness_report (include/g16hip.h)"""
    _fields_ = [("failed", ctypes.c_uint32), ("constraints", ctypes.c_int32),
                ("noncanonical_count", ctypes.c_size_t), ("first_noncanonical", ctypes.c_size_t),
                ("bad_count", ctypes.c_size_t), ("first_bad", ctypes.c_size_t * WITNESS_LIST),
                ("az", ctypes.c_uint8 * 32), ("bz", ctypes.c_uint8 * 32), ("cz", ctypes.c_uint8 * 32)]


class WitnessReport:
    """What g16_witness_check found.  constraints = 1 (all hold), 0 (some fail) or -1 (not run: a value is not
    canonical); first_noncanonical is an index or None; first_bad the (at most WITNESS_LIST) smallest failing constraint
    indices, ascending; az, bz, cz the three sums at first_bad[0] as integers (0 when there is none)."""

    def __init__(self, failed, constraints, noncanonical_count, first_noncanonical, bad_count, first_bad, az, bz, cz):
        self.failed, self.constraints = failed, constraints
        self.noncanonical_count, self.first_noncanonical = noncanonical_count, first_noncanonical
        self.bad_count, self.first_bad = bad_count, list(first_bad)
        self.az, self.bz, self.cz = az, bz, cz

    @property
    def ok(self) -> bool:
        """fit to prove with"""
        return self.failed == 0

    def as_dict(self) -> dict:
        return {"failed": self.failed, "constraints": self.constraints, "noncanonical_count": self.noncanonical_count,
                "first_noncanonical": self.first_noncanonical, "bad_count": self.bad_count, "first_bad": self.first_bad,
                "az": self.az, "bz": self.bz, "cz": self.cz}

    def findings(self):
        """one line per finding: the first value that is not canonical, witness[0], the failing constraints"""
        out = []
        if self.noncanonical_count:
            more = self.noncanonical_count - 1
            out.append(f"witness[{self.first_noncanonical}] is not canonical (>= r)" + (f" (and {more} more)" if more else ""))
        if self.failed & WITNESS_ONE:
            out.append("witness[0] is not 1")
        if self.bad_count:
            ab = self.az * self.bz % _R
            out.append(f"constraint {self.first_bad[0]}: (A z)(B z) = {ab:#x}, C z = {self.cz:#x}")
            rest = self.first_bad[1:]
            if rest:
                more = self.bad_count - len(self.first_bad)
                out.append("also failing: constraints " + ", ".join(map(str, rest)) + (f" (and {more} more)" if more else ""))
        return out

    def __str__(self):
        if self.ok:
            return "witness check: ok"
        return "witness check: FAILED\n" + "\n".join("  " + f for f in self.findings())


class Phase2Key(ctypes.Structure):
    """g16_phase2_key (include/g16hip.h): the part of a key a contribution touches"""
    _fields_ = [("delta1", ctypes.c_void_p), ("delta2", ctypes.c_void_p), ("pointsC1", ctypes.c_void_p),
                ("pointsH1", ctypes.c_void_p), ("nc1", ctypes.c_size_t), ("nh1", ctypes.c_size_t)]


class ContributionC(ctypes.Structure):
    """g16_contribution (include/g16hip.h): 320 bytes"""
    _fields_ = [("delta_after", ctypes.c_uint8 * 64), ("g1_s", ctypes.c_uint8 * 64), ("g1_sx", ctypes.c_uint8 * 64),
                ("g2_spx", ctypes.c_uint8 * 128)]


CONTRIBUTION_BYTES = 320
assert ctypes.sizeof(ContributionC) == CONTRIBUTION_BYTES


class Phase2Out(ctypes.Structure):
    """g16_phase2_out (include/g16hip.h)"""
    _fields_ = [("delta1", ctypes.c_void_p), ("delta2", ctypes.c_void_p), ("pointsC1", ctypes.c_void_p),
                ("pointsH1", ctypes.c_void_p), ("record", ctypes.POINTER(ContributionC))]


class PtauOut(ctypes.Structure):
    """g16_ptau_out (include/g16hip.h)"""
    _fields_ = [(name, ctypes.c_void_p) for name in PTAU_SECTIONS]


class PtauPokC(ctypes.Structure):
    _fields_ = [("g1_s", ctypes.c_uint8 * 64), ("g1_sx", ctypes.c_uint8 * 64), ("g2_spx", ctypes.c_uint8 * 128)]


class PtauContributionC(ctypes.Structure):
    """g16_ptau_contribution (include/g16hip.h): 1216 bytes"""
    _fields_ = [("tauG1", ctypes.c_uint8 * 64), ("alphaG1", ctypes.c_uint8 * 64), ("betaG1", ctypes.c_uint8 * 64),
                ("tauG2", ctypes.c_uint8 * 128), ("betaG2", ctypes.c_uint8 * 128), ("pok", PtauPokC * 3)]


PTAU_CONTRIBUTION_BYTES = 1216
assert ctypes.sizeof(PtauContributionC) == PTAU_CONTRIBUTION_BYTES


# the check of a .ptau (include/g16hip.h): the arrays and the relations of a report in order
PTAU_REPORT_ARRAYS = PTAU_SECTIONS + ("record tauG1", "record alphaG1", "record betaG1", "record tauG2", "record betaG2",
                                      "g1_s", "g1_sx", "g2_spx", "challenges")
PTAU_RELATIONS = ("ELEMENTS", "FIRST", "TAU_G1", "TAU_G2", "ALPHA", "BETA", "BETA_G2", "POK", "STEP", "LAST")


class PtauReportC(ctypes.Structure):
    """g16_ptau_report (include/g16hip.h)"""
    _fields_ = [("failed", ctypes.c_uint32), ("relation", ctypes.c_int32 * len(PTAU_RELATIONS)),
                ("first_record", ctypes.c_size_t * 2),
                ("first_bad", (ctypes.c_size_t * 3) * len(PTAU_REPORT_ARRAYS)),
                ("bad_count", (ctypes.c_size_t * 3) * len(PTAU_REPORT_ARRAYS)),
                ("first_infinity", ctypes.c_size_t * len(PTAU_REPORT_ARRAYS))]


class PtauReport:
    """What g16_ptau_verify found: relation[k] = 1 (holds), 0 (fails) or -1 (not run) for PTAU_RELATIONS[k]; first_record =
    the first record whose POK / STEP fails, or None; first_bad / bad_count [array][check] for PTAU_REPORT_ARRAYS as in a
    KeyReport (the three-per-record arrays count 3 j + x); first_infinity[array] = the first (0,0) element, or None."""

    def __init__(self, failed, relation, first_record, first_bad, bad_count, first_infinity):
        self.failed, self.relation, self.first_record = failed, list(relation), list(first_record)
        self.first_bad, self.bad_count, self.first_infinity = first_bad, bad_count, list(first_infinity)

    @property
    def ok(self) -> bool:
        return self.failed == 0

    def as_dict(self) -> dict:
        return {"failed": self.failed, "relation": self.relation, "first_record": self.first_record,
                "first_bad": self.first_bad, "bad_count": self.bad_count, "first_infinity": self.first_infinity}

    def findings(self):
        out = _element_findings(PTAU_REPORT_ARRAYS, self.first_bad, self.bad_count, self.first_infinity)
        for k, name in enumerate(PTAU_RELATIONS):
            if k and self.relation[k] == 0:
                rec = f" (first at record {self.first_record[k - 7]})" if name in ("POK", "STEP") else ""
                out.append(f"{name} fails{rec}")
        return out

    def __str__(self):
        rel = "  ".join(f"{n} {'ok' if v == 1 else 'FAILS' if v == 0 else 'not run'}" for n, v in zip(PTAU_RELATIONS, self.relation))
        return rel + "".join("\n  " + f for f in self.findings())


# contribution chain (include/g16hip.h): the arrays and the relations of a report in order
CHAIN_ARRAYS = ("delta_after", "g1_s", "g1_sx", "g2_spx", "challenges", "final delta1", "final delta2", "final pointsC1",
                "final pointsH1")
CHAIN_RELATIONS = ("ELEMENTS", "POK", "STEP", "LAST", "DELTA", "C1", "H1")


class ChainReportC(ctypes.Structure):
    """g16_chain_report (include/g16hip.h)"""
    _fields_ = [("failed", ctypes.c_uint32), ("relation", ctypes.c_int32 * len(CHAIN_RELATIONS)),
                ("first_record", ctypes.c_size_t * 2),
                ("first_bad", (ctypes.c_size_t * 3) * len(CHAIN_ARRAYS)),
                ("bad_count", (ctypes.c_size_t * 3) * len(CHAIN_ARRAYS)),
                ("first_infinity", ctypes.c_size_t * len(CHAIN_ARRAYS))]


class ChainReport:
    """What g16_contributions_verify found: relation[k] = 1 (holds), 0 (fails) or -1 (not run) for CHAIN_RELATIONS[k];
    first_record = the first record whose POK / STEP fails, or None; first_bad / bad_count [array][check] for
    CHAIN_ARRAYS as in a KeyReport; first_infinity[array] = the first (0,0) element, or None.  `transcript`: None from
    the C call, which hashes nothing; setup.verifyContributions sets it to 1 / 0: the key's cs_hash is the initial key's
    and every stored transcript hash is the one its predecessors give (the challenges are always re-derived)."""

    def __init__(self, failed, relation, first_record, first_bad, bad_count, first_infinity, transcript=None):
        self.failed, self.relation, self.first_record = failed, list(relation), list(first_record)
        self.first_bad, self.bad_count, self.first_infinity = first_bad, bad_count, list(first_infinity)
        self.transcript = transcript

    @property
    def ok(self) -> bool:
        """the records lead from the initial key to the final one"""
        return self.failed == 0 and self.transcript != 0

    def as_dict(self) -> dict:
        return {"failed": self.failed, "relation": self.relation, "first_record": self.first_record,
                "first_bad": self.first_bad, "bad_count": self.bad_count, "first_infinity": self.first_infinity,
                "transcript": self.transcript}

    def findings(self):
        out = []
        if self.transcript == 0:
            out.append("the transcript hashes are not those of the initial key and the records")
        out += _element_findings(CHAIN_ARRAYS, self.first_bad, self.bad_count, self.first_infinity)
        if self.relation[1] == 0:
            out.append(f"record {self.first_record[0]}: the proof of knowledge does not hold")
        if self.relation[2] == 0:
            out.append(f"record {self.first_record[1]}: delta_after is not the contribution's multiple of the delta before")
        if self.relation[3] == 0:
            out.append("the final delta1 is not the last record's delta_after")
        if self.relation[4] == 0:
            out.append("the final delta1 / delta2 are not the same multiple of the two generators")
        for k in (5, 6):
            if self.relation[k] == 0:
                out.append(f"the final points{CHAIN_RELATIONS[k]} is not the initial one rescaled by the deltas")
        return out

    def __str__(self):
        if self.ok:
            skipped = [CHAIN_RELATIONS[k] for k in range(len(CHAIN_RELATIONS)) if self.relation[k] < 0]
            return "contribution chain: ok" + (f" (not run: {', '.join(skipped)})" if skipped else "")
        return "contribution chain: FAILED\n" + "\n".join("  " + f for f in self.findings())


class G16Error(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"g16hip error {code}: {msg}")
        self.code = code


def lib_path() -> str:
    return os.environ.get("G16HIP_LIB", os.path.join(_HERE, "csrc", "libg16hip.so"))


def device_code_sha16(path: str = None) -> str:
    """Identity of the KERNELS of a libg16hip.so build: sha256 prefix of its .hip_fatbin section (the gfx950 code
    objects).  Host-side edits of the library leave it unchanged; any kernel change alters it.  bench.py reports
    counter-derived numbers (HBM traffic, VALU instruction counts) only next to files stamped with the same value."""
    import hashlib
    import struct
    b = open(path or lib_path(), "rb").read()
    h = hashlib.sha256()
    try:
        assert b[:4] == b"\x7fELF" and b[4] == 2
        shoff = struct.unpack_from("<Q", b, 0x28)[0]
        shentsize, shnum, shstrndx = struct.unpack_from("<HHH", b, 0x3A)

        def sh(i):
            name, _typ, _flags, _addr, off, size = struct.unpack_from("<IIQQQQ", b, shoff + i * shentsize)
            return name, off, size
        _, stro, _ = sh(shstrndx)
        hit = False
        for i in range(shnum):
            n, off, size = sh(i)
            if b[stro + n: b.index(b"\0", stro + n)] == b".hip_fatbin":
                h.update(b[off: off + size])
                hit = True
        assert hit
    except Exception:
        h = hashlib.sha256(b)             # not an ELF with a fat binary: the whole file
    return h.hexdigest()[:16]


_lib = None


def load_library():
    """Loads libg16hip.so.  Raises (never falls back) if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise G16Error(G16_ENODEV, f"{path} not found: build it with `make -C nim_groth16_amd/csrc` "
                                   "(or __graft_entry__.build()); there is no CPU fallback")
    # torch bundles its own libamdhip64.so.7; load it first so that this library binds to the SAME HIP
    # runtime (same SONAME) -- two HIP runtimes in one process cannot both own the GPU.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(path)
    vp, u32, i32, sz = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32, ctypes.c_size_t
    lib.g16_ctx_create.argtypes = [i32, ctypes.POINTER(vp)]
    lib.g16_ctx_destroy.argtypes = [vp]
    lib.g16_ctx_destroy.restype = None
    lib.g16_last_error.argtypes = [vp]
    lib.g16_last_error.restype = ctypes.c_char_p
    lib.g16_ctx_set_stream.argtypes = [vp, vp]
    lib.g16_ctx_synchronize.argtypes = [vp]
    lib.g16_selftest.argtypes = [vp]
    for name in ("g16_msm_g1", "g16_msm_g2", "g16_msm_g1_dev", "g16_msm_g2_dev",
                 "g16_msm_g1_partial_dev", "g16_msm_g2_partial_dev"):
        getattr(lib, name).argtypes = [vp, vp, u32, vp, sz, vp]
    for name in ("g16_g1_sum_partials", "g16_g2_sum_partials"):
        getattr(lib, name).argtypes = [vp, vp, sz, vp]
    for name in ("g16_points_register_g1", "g16_points_register_g2", "g16_points_register_g1_dev",
                 "g16_points_register_g2_dev"):
        getattr(lib, name).argtypes = [vp, vp, sz, ctypes.POINTER(vp)]
    for name in ("g16_points_register_g1_lean", "g16_points_register_g2_lean", "g16_points_register_g1_lean_dev",
                 "g16_points_register_g2_lean_dev"):
        getattr(lib, name).argtypes = [vp, vp, sz, u32, ctypes.POINTER(vp)]
    lib.g16_points_table_bytes.argtypes = [vp, ctypes.POINTER(sz)]
    lib.g16_points_plan.argtypes = [ctypes.c_int, sz, u32, ctypes.POINTER(u32), ctypes.POINTER(u32), ctypes.POINTER(sz)]
    lib.g16_pkey_create_lean.argtypes = [vp, ctypes.POINTER(PkeyDesc), u32, ctypes.POINTER(vp)]
    lib.g16_pkey_create_zkey_lean.argtypes = [vp, ctypes.POINTER(PkeyDesc), vp, sz, u32, ctypes.POINTER(vp)]
    lib.g16_group_pkey_create_lean.argtypes = [vp, ctypes.POINTER(PkeyDesc), u32, ctypes.POINTER(vp)]
    lib.g16_points_release.argtypes = [vp]
    lib.g16_points_release.restype = None
    lib.g16_points_count.argtypes = [vp]
    lib.g16_points_count.restype = sz
    lib.g16_points_inf_count.argtypes = [vp]
    lib.g16_points_inf_count.restype = sz
    lib.g16_pkey_inf_counts.argtypes = [vp, ctypes.POINTER(sz)]
    lib.g16_pkey_b1_fold.argtypes = [vp, ctypes.POINTER(sz)]
    lib.g16_pkey_b1_sparse.argtypes = [vp, ctypes.POINTER(sz)]
    lib.g16_points_info.argtypes = [vp, ctypes.POINTER(u32), ctypes.POINTER(u32)]
    lib.g16_msm_points.argtypes = [vp, vp, vp, u32, vp]
    lib.g16_points_check_g1.argtypes = [vp, vp, sz, ctypes.POINTER(sz)]
    lib.g16_points_check_g2.argtypes = [vp, vp, sz, ctypes.POINTER(sz)]
    lib.g16_fixed_base_g1.argtypes = [vp, vp, u32, sz, vp]
    lib.g16_fixed_base_g2.argtypes = [vp, vp, u32, sz, vp]
    lib.g16_quotient.argtypes = [vp, vp, vp, vp, u32, u32, vp]
    lib.g16_quotient_dev.argtypes = [vp, vp, vp, vp, u32, u32, vp]
    lib.g16_pkey_create.argtypes = [vp, ctypes.POINTER(PkeyDesc), ctypes.POINTER(vp)]
    lib.g16_pkey_create_zkey.argtypes = [vp, ctypes.POINTER(PkeyDesc), vp, sz, ctypes.POINTER(vp)]
    lib.g16_pkey_destroy.argtypes = [vp]
    lib.g16_pkey_destroy.restype = None
    lib.g16_prove.argtypes = [vp, vp, vp, u32, vp, vp, vp]
    lib.g16_build_abc.argtypes = [vp, vp, vp, u32, vp]
    lib.g16_pkey_abc_info.argtypes = [vp, ctypes.POINTER(sz)]
    lib.g16_spmv_fr.argtypes = [vp, vp, vp, vp, sz, vp, sz, sz, vp]
    lib.g16_prove_partials.argtypes = [vp, vp, vp, u32, vp]
    lib.g16_prove_combine.argtypes = [vp, vp, vp, sz, u32, vp, vp, vp]
    lib.g16_prove_partials_begin.argtypes = [vp, vp, vp, u32, u32, vp]
    lib.g16_prove_partials_end.argtypes = [vp, vp, vp, vp, vp, u32, vp]
    lib.g16_ntt_fr.argtypes = [vp, vp, vp, u32, i32]
    lib.g16_ntt_fr_dev.argtypes = [vp, vp, vp, u32, i32]
    lib.g16_vkey_create.argtypes = [vp, ctypes.POINTER(VkeyDesc), ctypes.POINTER(vp)]
    lib.g16_vkey_destroy.argtypes = [vp]
    lib.g16_vkey_destroy.restype = None
    lib.g16_verify.argtypes = [vp, vp, vp, vp, u32, sz, ctypes.POINTER(i32)]
    lib.g16_verify_batch.argtypes = [vp, vp, vp, vp, u32, sz, vp, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    lib.g16_pairing.argtypes = [vp, vp, vp, sz, vp]
    lib.g16_ctx_cancel.argtypes = [vp]
    lib.g16_group_create.argtypes = [ctypes.POINTER(i32), i32, ctypes.POINTER(vp)]
    lib.g16_group_destroy.argtypes = [vp]
    lib.g16_group_destroy.restype = None
    lib.g16_group_size.argtypes = [vp]
    lib.g16_group_last_error.argtypes = [vp]
    lib.g16_group_last_error.restype = ctypes.c_char_p
    lib.g16_group_pkey_create.argtypes = [vp, ctypes.POINTER(PkeyDesc), ctypes.POINTER(vp)]
    lib.g16_group_pkey_destroy.argtypes = [vp]
    lib.g16_group_pkey_destroy.restype = None
    lib.g16_group_prove.argtypes = [vp, vp, vp, u32, vp, vp, vp]
    lib.g16_prover_create.argtypes = [i32, vp, u32, ctypes.POINTER(vp)]
    lib.g16_prover_destroy.argtypes = [vp]
    lib.g16_prover_destroy.restype = None
    lib.g16_prover_last_error.argtypes = [vp]
    lib.g16_prover_last_error.restype = ctypes.c_char_p
    lib.g16_prover_submit.argtypes = [vp, vp, u32, vp, vp, ctypes.POINTER(ctypes.c_uint64)]
    lib.g16_prover_poll.argtypes = [vp, ctypes.c_uint64]
    lib.g16_prover_collect.argtypes = [vp, ctypes.c_uint64, vp]
    lib.g16_host_alloc.argtypes = [i32, sz, ctypes.POINTER(vp)]
    lib.g16_host_free.argtypes = [vp]
    lib.g16_host_free.restype = None
    lib.g16_profile_enable.argtypes = [vp, i32]
    lib.g16_profile_reset.argtypes = [vp]
    lib.g16_profile_report.argtypes = [vp, ctypes.c_char_p, sz]
    lib.g16_profile_clock.argtypes = [vp, ctypes.POINTER(ctypes.c_double)]
    lib.g16_setup_log2_domain.argtypes = [ctypes.POINTER(SetupDesc), ctypes.POINTER(u32)]
    lib.g16_fake_setup.argtypes = [vp, ctypes.POINTER(SetupDesc), ctypes.POINTER(SetupPoints)]
    lib.g16_lagrange_fr.argtypes = [vp, u32, u32, u32, sz, vp, vp, vp]
    lib.g16_powers_fr.argtypes = [vp, vp, vp, sz, vp]
    lib.g16_points_audit_g1.argtypes = [vp, vp, sz, ctypes.POINTER(sz), ctypes.POINTER(sz)]
    lib.g16_points_audit_g2.argtypes = [vp, vp, sz, ctypes.POINTER(sz), ctypes.POINTER(sz)]
    lib.g16_points_pairs_check.argtypes = [vp, vp, vp, sz, vp, ctypes.POINTER(i32)]
    lib.g16_key_audit.argtypes = [vp, ctypes.POINTER(PkeyDesc), ctypes.POINTER(VkeyDesc), vp, sz, vp,
                                  ctypes.POINTER(KeyReportC)]
    lib.g16_circuit_audit.argtypes = [vp, ctypes.POINTER(PkeyDesc), ctypes.POINTER(VkeyDesc), vp, sz,
                                      ctypes.POINTER(R1csDesc), ctypes.POINTER(PtauDesc), vp, vp,
                                      ctypes.POINTER(CircuitReportC)]
    lib.g16_points_intt_g1.argtypes = [vp, vp, u32, vp]
    lib.g16_points_intt_g2.argtypes = [vp, vp, u32, vp]
    lib.g16_circuit_setup.argtypes = [vp, ctypes.POINTER(R1csDesc), ctypes.POINTER(PtauDesc), vp,
                                      ctypes.POINTER(SetupPoints)]
    lib.g16_points_scale_g1.argtypes = [vp, vp, sz, vp, u32, vp]
    lib.g16_points_scale_g2.argtypes = [vp, vp, sz, vp, u32, vp]
    lib.g16_points_scale_each_g1.argtypes = [vp, vp, sz, vp, u32, vp]
    lib.g16_points_scale_each_g2.argtypes = [vp, vp, sz, vp, u32, vp]
    lib.g16_key_contribute.argtypes = [vp, ctypes.POINTER(Phase2Key), vp, vp, u32, vp, ctypes.POINTER(Phase2Out)]
    lib.g16_contributions_verify.argtypes = [vp, ctypes.POINTER(Phase2Key), ctypes.POINTER(Phase2Key),
                                             ctypes.POINTER(ContributionC), vp, sz, vp, vp, ctypes.POINTER(ChainReportC)]
    lib.g16_ptau_contribute.argtypes = [vp, ctypes.POINTER(PtauDesc), vp, vp, vp, vp, u32, vp, ctypes.POINTER(PtauOut),
                                        ctypes.POINTER(PtauContributionC)]
    lib.g16_ptau_verify.argtypes = [vp, ctypes.POINTER(PtauDesc), ctypes.POINTER(PtauContributionC), vp, sz, vp,
                                    ctypes.POINTER(PtauReportC)]
    lib.g16_r1cs_create.argtypes = [vp, ctypes.POINTER(R1csDesc), ctypes.POINTER(vp)]
    lib.g16_r1cs_destroy.argtypes = [vp]
    lib.g16_r1cs_destroy.restype = None
    lib.g16_r1cs_info.argtypes = [vp, ctypes.POINTER(sz)]
    lib.g16_witness_check.argtypes = [vp, vp, vp, u32, ctypes.POINTER(WitnessReportC)]
    for name in SYMBOLS:
        if name not in ("g16_ctx_destroy", "g16_r1cs_destroy", "g16_last_error", "g16_points_release", "g16_points_count",
                        "g16_points_inf_count",
                        "g16_pkey_destroy", "g16_vkey_destroy", "g16_group_destroy", "g16_group_last_error",
                        "g16_group_pkey_destroy", "g16_prover_destroy", "g16_prover_last_error", "g16_host_free"):
            getattr(lib, name).restype = i32
    _lib = lib
    return lib


def _buf(b):
    """bytes / bytearray / numpy array / int (device pointer) -> c_void_p-compatible"""
    if isinstance(b, int):
        return ctypes.c_void_p(b)
    if isinstance(b, (bytes, bytearray)):
        return ctypes.cast(ctypes.c_char_p(bytes(b)), ctypes.c_void_p) if isinstance(b, bytes) else \
            ctypes.cast((ctypes.c_char * len(b)).from_buffer(b), ctypes.c_void_p)
    if hasattr(b, "ctypes"):            # numpy
        return ctypes.c_void_p(b.ctypes.data)
    raise TypeError(type(b))


class Context:
    """One g16_ctx = one GPU + one stream; used by one host thread at a time (include/g16hip.h)."""

    def __init__(self, device: int = 0):
        self._lib = load_library()
        h = ctypes.c_void_p()
        rc = self._lib.g16_ctx_create(device, ctypes.byref(h))
        if rc != G16_OK:
            raise G16Error(rc, "g16_ctx_create failed (no usable HIP device?)")
        self._h = h
        self.device = device
        # point sets / keys created through this context.  They belong to the DEVICE (include/g16hip.h): the C ABI
        # lets them outlive the context or die first, in any order; the set only serves close(release_children=True)
        self._children = weakref.WeakSet()

    def close(self, release_children: bool = False):
        if getattr(self, "_h", None):
            if release_children:
                for child in list(self._children):
                    child._free()
            self._lib.g16_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != G16_OK:
            raise G16Error(rc, self._lib.g16_last_error(self._h).decode())

    def selftest(self):
        self._check(self._lib.g16_selftest(self._h))

    def set_stream(self, stream_ptr):
        self._check(self._lib.g16_ctx_set_stream(self._h, ctypes.c_void_p(stream_ptr)))

    def synchronize(self):
        self._check(self._lib.g16_ctx_synchronize(self._h))

    def cancel(self):
        """drain the main stream and every MSM lane, forget a pending prove_partials_begin (g16_ctx_cancel)"""
        self._check(self._lib.g16_ctx_cancel(self._h))

    # ---- MSM -----------------------------------------------------------------------------------
    def msm(self, group: int, scalars, points, n: int, mont: bool = True, device: bool = False,
            partial: bool = False) -> bytes:
        """group 1 -> G1 (64-byte points), 2 -> G2 (128-byte points).  Returns the affine result
        bytes (or the XYZZ partial when partial=True)."""
        psz = 64 if group == 1 else 128
        out = ctypes.create_string_buffer(2 * psz if partial else psz)
        if partial:
            fn = self._lib.g16_msm_g1_partial_dev if group == 1 else self._lib.g16_msm_g2_partial_dev
        elif device:
            fn = self._lib.g16_msm_g1_dev if group == 1 else self._lib.g16_msm_g2_dev
        else:
            fn = self._lib.g16_msm_g1 if group == 1 else self._lib.g16_msm_g2
        s = _buf(scalars) if n else None
        p = _buf(points) if n else None
        self._check(fn(self._h, s, SCALARS_MONT if mont else SCALARS_STD, p, n, out))
        return out.raw

    def register_points(self, group: int, points, n: int, device: bool = False, table_stride: int = 0) -> "PointSet":
        """table_stride >= 2: a lean set -- window tables for every table_stride-th window only (points_plan tells the
        bytes beforehand); 0 or 1: a table per window"""
        h = ctypes.c_void_p()
        p = _buf(points) if n else None
        if table_stride:
            name = f"g16_points_register_g{group}_lean" + ("_dev" if device else "")
            self._check(getattr(self._lib, name)(self._h, p, n, table_stride, ctypes.byref(h)))
        else:
            name = f"g16_points_register_g{group}" + ("_dev" if device else "")
            self._check(getattr(self._lib, name)(self._h, p, n, ctypes.byref(h)))
        return PointSet(self, h, group, n)

    def msm_points(self, pts: "PointSet", scalars, mont: bool = True, device: bool = False,
                   partial: bool = False) -> bytes:
        psz = 64 if pts.group == 1 else 128
        out = ctypes.create_string_buffer(2 * psz if partial else psz)
        flags = (SCALARS_MONT if mont else 0) | (SCALARS_DEVICE if device else 0) | (OUT_PARTIAL if partial else 0)
        self._check(self._lib.g16_msm_points(self._h, pts._h, _buf(scalars) if pts.n else None, flags, out))
        return out.raw

    def points_check(self, group: int, points: bytes):
        """index of the first point off the curve, or None (curves.nim:95-107 mkG1/mkG2 asserts)"""
        psz = 64 if group == 1 else 128
        n = len(points) // psz
        bad = ctypes.c_size_t()
        fn = self._lib.g16_points_check_g1 if group == 1 else self._lib.g16_points_check_g2
        self._check(fn(self._h, _buf(points) if n else None, n, ctypes.byref(bad)))
        return None if bad.value == ctypes.c_size_t(-1).value else bad.value

    # ---- key audit ------------------------------------------------------------------------------
    def points_audit(self, group: int, points: bytes):
        """g16_points_audit_g1/g2 -> (first_bad, bad_count): per check (canonical, curve, subgroup) the index of the
        first failing element (None: none) and how many fail; an element counts under the first check it fails"""
        psz = 64 if group == 1 else 128
        assert len(points) % psz == 0
        n = len(points) // psz
        first, count = (ctypes.c_size_t * 3)(), (ctypes.c_size_t * 3)()
        fn = self._lib.g16_points_audit_g1 if group == 1 else self._lib.g16_points_audit_g2
        self._check(fn(self._h, _buf(points) if n else None, n, first, count))
        none = ctypes.c_size_t(-1).value
        return [None if f == none else f for f in first], list(count)

    def pairs_check(self, g1_points: bytes, g2_points: bytes, multipliers) -> bool:
        """g16_points_pairs_check: are g1_points[i] and g2_points[i] the same multiple of gen1 and gen2 for every i?
        Both arrays must pass points_audit.  multipliers: one int in [1, 2^128) per pair, drawn by the caller."""
        n = len(g1_points) // 64
        assert len(g1_points) == 64 * n and len(g2_points) == 128 * n and len(multipliers) == n
        zs = b"".join(int(z).to_bytes(16, "little") for z in multipliers)
        res = ctypes.c_int32(-1)
        self._check(self._lib.g16_points_pairs_check(self._h, _buf(g1_points) if n else None,
                                                     _buf(g2_points) if n else None, n, _buf(zs) if n else None,
                                                     ctypes.byref(res)))
        return res.value == 1

    def key_audit(self, desc: PkeyDesc, vk: VkeyDesc = None, section4: bytes = None, multipliers=None) -> KeyReport:
        """g16_key_audit.  desc / section4 as for ProvingKey; vk: a VkeyDesc (gamma2 and pointsIC are read) or None;
        multipliers: desc.nvars ints in [1, 2^128) (or their 16-byte encodings, joined), or None to skip the pointsB1 ~ pointsB2 relation."""
        zs = None
        if isinstance(multipliers, (bytes, bytearray)):             # already 16 little-endian bytes each
            assert len(multipliers) == 16 * desc.nvars, "one multiplier per wire"
            zs = bytes(multipliers)
        elif multipliers is not None:
            assert len(multipliers) == desc.nvars, "one multiplier per wire"
            zs = b"".join(int(z).to_bytes(16, "little") for z in multipliers)
        rep = KeyReportC()
        self._check(self._lib.g16_key_audit(self._h, ctypes.byref(desc), ctypes.byref(vk) if vk is not None else None,
                                            _buf(section4) if section4 is not None else None,
                                            len(section4) if section4 is not None else 0,
                                            _buf(zs) if zs is not None else None, ctypes.byref(rep)))
        none = ctypes.c_size_t(-1).value
        return KeyReport(rep.failed, rep.spec_infinity, list(rep.relation),
                         [[None if f == none else f for f in row] for row in rep.first_bad],
                         [list(row) for row in rep.bad_count])

    def circuit_audit(self, desc: PkeyDesc, vk, section4, r1cs: R1csDesc, ptau: PtauDesc, wire_multipliers,
                      h_multipliers) -> CircuitReport:
        """g16_circuit_audit.  desc / vk / section4 as for key_audit; r1cs, ptau: the two descriptions (the caller keeps
        their buffers alive); wire_multipliers: desc.nvars ints in [1, 2^128), h_multipliers: 2^log2_domain of them (or
        their 16-byte encodings, joined), drawn by the caller after every input is fixed."""
        def enc(zs, n, what):
            if isinstance(zs, (bytes, bytearray)):
                assert len(zs) == 16 * n, f"one {what} multiplier of 16 bytes each"
                return bytes(zs)
            assert len(zs) == n, f"{n} {what} multipliers"
            return b"".join(int(z).to_bytes(16, "little") for z in zs)
        zw = enc(wire_multipliers, desc.nvars, "wire")
        zh = enc(h_multipliers, 1 << min(desc.log2_domain, 28), "h")
        rep = CircuitReportC()
        self._check(self._lib.g16_circuit_audit(self._h, ctypes.byref(desc), ctypes.byref(vk) if vk is not None else None,
                                                _buf(section4) if section4 is not None else None,
                                                len(section4) if section4 is not None else 0,
                                                ctypes.byref(r1cs), ctypes.byref(ptau), _buf(zw), _buf(zh),
                                                ctypes.byref(rep)))
        none = ctypes.c_size_t(-1).value
        fix = lambda rows: [[None if f == none else f for f in row] for row in rows]     # noqa: E731
        key = KeyReport(rep.key.failed, rep.key.spec_infinity, list(rep.key.relation), fix(rep.key.first_bad),
                        [list(row) for row in rep.key.bad_count])
        return CircuitReport(key, fix(rep.ptau_first_bad), [list(row) for row in rep.ptau_bad_count], list(rep.relation),
                             rep.failed, [None if f == none else f for f in rep.first_row])

    def r1cs_load(self, desc: R1csDesc, keepalive=None) -> "R1csSystem":
        """g16_r1cs_create: the constraint system of `desc` resident on this context's device"""
        return R1csSystem(self, desc, keepalive)

    def fixed_base(self, group: int, scalars: bytes, mont: bool = True) -> bytes:
        """scalars[i] * generator -> affine points (fake_setup.nim:258-261 `y ** gen1/gen2`)."""
        n = len(scalars) // 32
        psz = 64 if group == 1 else 128
        out = ctypes.create_string_buffer(max(n, 1) * psz)
        fn = self._lib.g16_fixed_base_g1 if group == 1 else self._lib.g16_fixed_base_g2
        self._check(fn(self._h, _buf(scalars) if n else None, SCALARS_MONT if mont else 0, n, out))
        return out.raw[: n * psz]

    def spmv(self, row, col, val, x: bytes, nrows: int) -> bytes:
        """y = M x over Fr (Montgomery): M as triplets -- row, col: uint32 numpy arrays; val: nnz x 32 bytes (numpy
        uint8 array or bytes); x: ncols Fr.  The sparse column dot products of fake_setup.nim:159-187 on the GPU."""
        import numpy as np
        row = np.ascontiguousarray(row, dtype=np.uint32)
        col = np.ascontiguousarray(col, dtype=np.uint32)
        nnz = len(row)
        if not isinstance(val, (bytes, bytearray)):
            val = np.ascontiguousarray(val, dtype=np.uint8)
        assert len(col) == nnz and (len(val) if isinstance(val, (bytes, bytearray)) else val.size) == 32 * nnz
        out = ctypes.create_string_buffer(max(1, 32 * nrows))
        self._check(self._lib.g16_spmv_fr(self._h, _buf(row) if nnz else None, _buf(col) if nnz else None,
                                          _buf(val) if nnz else None, nnz, _buf(x) if len(x) else None, len(x) // 32,
                                          nrows, out))
        return out.raw[: 32 * nrows]

    def lagrange(self, log2n: int, tau: bytes, first: int = 0, step: int = 1, count: int = None,
                 scale: bytes = None) -> bytes:
        """scale * L_{first + step i}(tau) for i < count on the 2^log2n domain (math/poly.nim:242-250), Montgomery Fr
        bytes in and out; count None = every index from `first` at `step` that the domain holds"""
        if count is None:
            count = ((1 << log2n) - first + step - 1) // step if step else 1
        out = ctypes.create_string_buffer(max(1, 32 * count))
        self._check(self._lib.g16_lagrange_fr(self._h, log2n, first, step, count, _buf(tau),
                                              _buf(scale) if scale is not None else None, out))
        return out.raw[: 32 * count]

    def powers(self, base: bytes, count: int, scale: bytes = None) -> bytes:
        """scale * base^i for i < count (fake_setup.nim:290-294), Montgomery Fr bytes in and out"""
        out = ctypes.create_string_buffer(max(1, 32 * count))
        self._check(self._lib.g16_powers_fr(self._h, _buf(base), _buf(scale) if scale is not None else None, count, out))
        return out.raw[: 32 * count]

    def fake_setup(self, nvars: int, npubs: int, nconstraints: int, flavour: int, matrices, toxic, mont: bool = True):
        """g16_fake_setup: matrices = three (constraint, wire, values) triplet sets for A, B, C -- uint32 numpy arrays
        and nnz x 32 value bytes (numpy uint8 array or bytes); toxic = (alpha, beta, gamma, delta, tau) as 32-byte
        strings in the form `mont` names.  -> (log2 of the domain, {name: bytes} for every member of g16_setup_points)"""
        import numpy as np
        d = SetupDesc()
        d.nvars, d.npubs, d.nconstraints, d.flavour = nvars, npubs, nconstraints, flavour
        d.flags = SCALARS_MONT if mont else SCALARS_STD
        keep = []
        for k, (rows, wires, vals) in enumerate(matrices):
            rows = np.ascontiguousarray(rows, dtype=np.uint32)
            wires = np.ascontiguousarray(wires, dtype=np.uint32)
            if not isinstance(vals, (bytes, bytearray)):
                vals = np.ascontiguousarray(vals, dtype=np.uint8)
            nnz = len(rows)
            assert len(wires) == nnz and (len(vals) if isinstance(vals, (bytes, bytearray)) else vals.size) == 32 * nnz
            keep += [rows, wires, vals]
            d.nnz[k] = nnz
            if nnz:
                d.row[k], d.col[k], d.val[k] = (_buf(x).value for x in (rows, wires, vals))
        toxic = [bytes(t) for t in toxic]
        d.alpha, d.beta, d.gamma, d.delta, d.tau = (_buf(t).value for t in toxic)
        log2 = ctypes.c_uint32()
        rc = self._lib.g16_setup_log2_domain(ctypes.byref(d), ctypes.byref(log2))
        if rc != G16_OK:
            raise G16Error(rc, "g16_setup_log2_domain failed")
        sizes = dict(alpha1=64, beta1=64, delta1=64, beta2=128, gamma2=128, delta2=128, pointsIC=64 * (npubs + 1),
                     pointsA1=64 * nvars, pointsB1=64 * nvars, pointsB2=128 * nvars,
                     pointsC1=64 * max(0, nvars - npubs - 1), pointsH1=64 << min(log2.value, 40))
        if log2.value + (1 if flavour == 1 else 0) > 28:     # the call rejects the domain before it writes anything
            sizes = dict.fromkeys(sizes, 0)
        o = SetupPoints()
        bufs = {}
        for name, nbytes in sizes.items():
            bufs[name] = ctypes.create_string_buffer(max(1, nbytes))
            setattr(o, name, ctypes.cast(bufs[name], ctypes.c_void_p).value)
        self._check(self._lib.g16_fake_setup(self._h, ctypes.byref(d), ctypes.byref(o)))
        return log2.value, {name: bufs[name].raw[: sizes[name]] for name in SETUP_POINTS}

    def points_intt(self, group: int, points: bytes, log2n: int) -> bytes:
        """g16_points_intt_g1/g2: out[k] = sum_j (omega^-jk / n) points[j] over n = 2^log2n affine points -- the inverse
        NTT with curve points for elements (the Lagrange form of a run of powers of tau)"""
        psz = 64 if group == 1 else 128
        assert len(points) == psz << log2n, f"2^{log2n} points of {psz} bytes"
        out = ctypes.create_string_buffer(len(points))
        fn = self._lib.g16_points_intt_g1 if group == 1 else self._lib.g16_points_intt_g2
        self._check(fn(self._h, _buf(points), log2n, out))
        return out.raw

    def circuit_setup(self, r1cs: R1csDesc, ptau: PtauDesc, delta: bytes = None):
        """g16_circuit_setup: the key of `snarkjs zkey new` from the two descriptions of the circuit audit (the caller
        keeps their buffers alive); delta: None (= 1) or 32 bytes in the form r1cs.flags names.
        -> (log2 of the domain, {name: bytes} for every member of g16_setup_points)"""
        nvars, npubs = r1cs.nvars, r1cs.npubs
        log2 = max(0, (r1cs.nconstraints + npubs).bit_length())          # ceilingLog2(nconstraints + npubs + 1)
        sizes = dict(alpha1=64, beta1=64, delta1=64, beta2=128, gamma2=128, delta2=128, pointsIC=64 * (npubs + 1),
                     pointsA1=64 * nvars, pointsB1=64 * nvars, pointsB2=128 * nvars,
                     pointsC1=64 * max(0, nvars - npubs - 1), pointsH1=64 << log2)
        if log2 > 24:                                        # the call rejects the domain before it writes anything
            sizes = dict.fromkeys(sizes, 0)
        o = SetupPoints()
        bufs = {}
        for name, nbytes in sizes.items():
            bufs[name] = ctypes.create_string_buffer(max(1, nbytes))
            setattr(o, name, ctypes.cast(bufs[name], ctypes.c_void_p).value)
        self._check(self._lib.g16_circuit_setup(self._h, ctypes.byref(r1cs), ctypes.byref(ptau),
                                                _buf(bytes(delta)) if delta is not None else None, ctypes.byref(o)))
        return log2, {name: bufs[name].raw[: sizes[name]] for name in SETUP_POINTS}

    def points_scale(self, group: int, points: bytes, k: bytes, mont: bool = True) -> bytes:
        """g16_points_scale_g1/g2: out[i] = k * points[i] for one 32-byte scalar k (canonical; zero is legal) and affine
        points of the curve, (0,0) anywhere"""
        psz = 64 if group == 1 else 128
        assert len(points) % psz == 0 and len(k) == 32, f"points of {psz} bytes and a 32-byte scalar"
        out = ctypes.create_string_buffer(max(1, len(points)))
        fn = self._lib.g16_points_scale_g1 if group == 1 else self._lib.g16_points_scale_g2
        self._check(fn(self._h, _buf(bytes(points)), len(points) // psz, _buf(bytes(k)),
                       SCALARS_MONT if mont else SCALARS_STD, out))
        return out.raw[: len(points)]

    def points_scale_each(self, group: int, points: bytes, scalars: bytes, mont: bool = True) -> bytes:
        """g16_points_scale_each_g1/g2: out[i] = scalars[i] * points[i], one 32-byte scalar per point (canonical, all in
        one form; zero is legal) and affine points of the curve, (0,0) anywhere"""
        psz = 64 if group == 1 else 128
        assert len(points) % psz == 0 and len(scalars) == 32 * (len(points) // psz), \
            f"points of {psz} bytes and one 32-byte scalar for each"
        out = ctypes.create_string_buffer(max(1, len(points)))
        fn = self._lib.g16_points_scale_each_g1 if group == 1 else self._lib.g16_points_scale_each_g2
        self._check(fn(self._h, _buf(bytes(points)), len(points) // psz, _buf(bytes(scalars)),
                       SCALARS_MONT if mont else SCALARS_STD, out))
        return out.raw[: len(points)]

    @staticmethod
    def _phase2_key(key: dict):
        """{delta1, delta2, pointsC1, pointsH1: bytes} -> (Phase2Key, the buffers it points into)"""
        assert len(key["delta1"]) == 64 and len(key["delta2"]) == 128, "delta1: 64 bytes, delta2: 128 bytes"
        assert len(key["pointsC1"]) % 64 == 0 and len(key["pointsH1"]) % 64 == 0, "G1 points of 64 bytes"
        keep = {name: bytes(key[name]) for name in ("delta1", "delta2", "pointsC1", "pointsH1")}
        pk = Phase2Key()
        for name, b in keep.items():
            setattr(pk, name, ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p).value if b else None)
        pk.nc1, pk.nh1 = len(keep["pointsC1"]) // 64, len(keep["pointsH1"]) // 64
        return pk, keep

    def key_contribute(self, key: dict, d: bytes, s: bytes, challenge_g2: bytes, mont: bool = True):
        """g16_key_contribute.  key: {delta1, delta2, pointsC1, pointsH1: bytes}; d, s: 32-byte secrets, non-zero;
        challenge_g2: the 128-byte challenge point of this contribution (the caller derives it: phase2.py).
        -> ({delta1, delta2, pointsC1, pointsH1} of the contributed key, the 320-byte record)"""
        assert len(d) == 32 and len(s) == 32 and len(challenge_g2) == 128
        pk, keep = self._phase2_key(key)
        bufs = {name: ctypes.create_string_buffer(max(1, len(b))) for name, b in keep.items()}
        rec = ContributionC()
        o = Phase2Out()
        for name in bufs:
            setattr(o, name, ctypes.cast(bufs[name], ctypes.c_void_p).value)
        o.record = ctypes.pointer(rec)
        self._check(self._lib.g16_key_contribute(self._h, ctypes.byref(pk), _buf(bytes(d)), _buf(bytes(s)),
                                                 SCALARS_MONT if mont else SCALARS_STD, _buf(bytes(challenge_g2)),
                                                 ctypes.byref(o)))
        return {name: bufs[name].raw[: len(keep[name])] for name in keep}, bytes(rec)

    def ptau_contribute(self, ptau: dict, t: bytes, a: bytes, b: bytes, s3: bytes, challenges_g2: bytes, mont: bool = True,
                        power: int = None):
        """g16_ptau_contribute.  ptau: {tauG1, tauG2, alphaTauG1, betaTauG1, betaG2: bytes} of the power `power` (None:
        from the length of tauG2); t, a, b: 32-byte secrets, s3: the three proof-of-knowledge secrets (96 bytes), all
        non-zero; challenges_g2: the three 128-byte challenge points for t, a, b (the caller derives them: phase1.py).
        -> ({tauG1, ...} of the contributed powers, the 1216-byte record)"""
        assert len(t) == len(a) == len(b) == 32 and len(s3) == 96 and len(challenges_g2) == 384
        keep = {name: bytes(ptau[name]) for name in PTAU_SECTIONS}
        if power is None:
            power = max(0, (len(keep["tauG2"]) // 128).bit_length() - 1)
            assert [len(keep[n]) for n in PTAU_SECTIONS] == [64 * ((2 << power) - 1), 128 << power, 64 << power,
                                                             64 << power, 128], "not the arrays of one power"
        desc = PtauDesc(power, *[ctypes.cast(ctypes.c_char_p(keep[n]), ctypes.c_void_p) if keep[n] else None
                                 for n in PTAU_SECTIONS])
        bufs = {name: ctypes.create_string_buffer(max(1, len(v))) for name, v in keep.items()}
        o = PtauOut(*[ctypes.cast(bufs[n], ctypes.c_void_p) for n in PTAU_SECTIONS])
        rec = PtauContributionC()
        self._check(self._lib.g16_ptau_contribute(self._h, ctypes.byref(desc), _buf(bytes(t)), _buf(bytes(a)), _buf(bytes(b)),
                                                  _buf(bytes(s3)), SCALARS_MONT if mont else SCALARS_STD,
                                                  _buf(bytes(challenges_g2)), ctypes.byref(o), ctypes.byref(rec)))
        return {name: bufs[name].raw[: len(keep[name])] for name in PTAU_SECTIONS}, bytes(rec)

    def ptau_verify(self, ptau: dict, records, challenges_g2, multipliers, power: int = None) -> PtauReport:
        """g16_ptau_verify.  ptau: {tauG1, ...: bytes}; records: the 1216-byte records in order, or None (no chain to
        check); challenges_g2: 384 bytes per record; multipliers: 2^(power+1) - 2 ints in [1, 2^128) (or their 16-byte
        encodings, joined), drawn by the caller after every input is fixed."""
        keep = {name: bytes(ptau[name]) for name in PTAU_SECTIONS}
        if power is None:
            power = max(0, (len(keep["tauG2"]) // 128).bit_length() - 1)
            assert [len(keep[n]) for n in PTAU_SECTIONS] == [64 * ((2 << power) - 1), 128 << power, 64 << power,
                                                             64 << power, 128], "not the arrays of one power"
        desc = PtauDesc(power, *[ctypes.cast(ctypes.c_char_p(keep[n]), ctypes.c_void_p) for n in PTAU_SECTIONS])
        m = (2 << power) - 2
        if isinstance(multipliers, (bytes, bytearray)):
            zs = bytes(multipliers)
        else:
            zs = b"".join(int(z).to_bytes(16, "little") for z in multipliers)
        assert len(zs) == 16 * m or not 1 <= power <= 25, f"{m} multipliers of 16 bytes each"
        recs, ch, count = None, None, 0
        if records is not None:
            count = len(records)
            assert all(len(r) == PTAU_CONTRIBUTION_BYTES for r in records)
            recs = (PtauContributionC * max(1, count)).from_buffer_copy(b"".join(records) or bytes(PTAU_CONTRIBUTION_BYTES))
            ch = b"".join(challenges_g2)
            assert len(ch) == 384 * count, "three 128-byte challenge points per record"
        rep = PtauReportC()
        self._check(self._lib.g16_ptau_verify(self._h, ctypes.byref(desc), recs, _buf(ch) if ch else None, count, _buf(zs),
                                              ctypes.byref(rep)))
        none = ctypes.c_size_t(-1).value
        opt = lambda row: [None if f == none else f for f in row]     # noqa: E731
        return PtauReport(rep.failed, list(rep.relation), opt(rep.first_record), [opt(row) for row in rep.first_bad],
                          [list(row) for row in rep.bad_count], opt(rep.first_infinity))

    def contributions_verify(self, initial: dict, final: dict, records, challenges_g2, c1_multipliers,
                             h1_multipliers) -> ChainReport:
        """g16_contributions_verify.  initial (the trusted anchor) / final: {delta1, delta2, pointsC1, pointsH1: bytes};
        records: the 320-byte records in order; challenges_g2: one 128-byte point per record; the multipliers: ints in
        [1, 2^128) (or their 16-byte encodings, joined), one per point of pointsC1 / pointsH1, drawn by the caller
        after every input is fixed."""
        def enc(zs, n, what):
            if isinstance(zs, (bytes, bytearray)):
                assert len(zs) == 16 * n, f"one {what} multiplier of 16 bytes each"
                return bytes(zs)
            assert len(zs) == n, f"{n} {what} multipliers"
            return b"".join(int(z).to_bytes(16, "little") for z in zs)
        records, challenges_g2 = list(records), list(challenges_g2)
        assert len(records) == len(challenges_g2) and all(len(r) == CONTRIBUTION_BYTES for r in records) and \
            all(len(c) == 128 for c in challenges_g2), "one 320-byte record and one 128-byte challenge per contribution"
        ki, keep_i = self._phase2_key(initial)
        kf, keep_f = self._phase2_key(final)
        zc, zh = enc(c1_multipliers, kf.nc1, "c1"), enc(h1_multipliers, kf.nh1, "h1")
        recs = (ContributionC * max(1, len(records))).from_buffer_copy(b"".join(records) or bytes(CONTRIBUTION_BYTES))
        ch = b"".join(challenges_g2)
        rep = ChainReportC()
        self._check(self._lib.g16_contributions_verify(self._h, ctypes.byref(ki), ctypes.byref(kf), recs,
                                                       _buf(ch) if ch else None, len(records),
                                                       _buf(zc) if zc else None, _buf(zh) if zh else None,
                                                       ctypes.byref(rep)))
        none = ctypes.c_size_t(-1).value
        opt = lambda row: [None if f == none else f for f in row]     # noqa: E731
        return ChainReport(rep.failed, list(rep.relation), opt(rep.first_record), [opt(row) for row in rep.first_bad],
                           [list(row) for row in rep.bad_count], opt(rep.first_infinity))

    def quotient(self, Az, Bz, Cz, log2n: int, flavour: int, out=None, device: bool = False):
        if device:
            self._check(self._lib.g16_quotient_dev(self._h, _buf(Az), _buf(Bz), _buf(Cz), log2n, flavour, _buf(out)))
            return None
        res = ctypes.create_string_buffer(32 << log2n)
        self._check(self._lib.g16_quotient(self._h, _buf(Az), _buf(Bz), _buf(Cz), log2n, flavour, res))
        return res.raw

    def sum_partials(self, group: int, xyzz: bytes, count: int) -> bytes:
        psz = 64 if group == 1 else 128
        out = ctypes.create_string_buffer(psz)
        fn = self._lib.g16_g1_sum_partials if group == 1 else self._lib.g16_g2_sum_partials
        self._check(fn(self._h, _buf(xyzz) if count else None, count, out))
        return out.raw

    # ---- NTT -----------------------------------------------------------------------------------
    def ntt(self, src, log2n: int, inverse: bool, dst=None, device: bool = False):
        n = 1 << log2n
        if device:
            self._check(self._lib.g16_ntt_fr_dev(self._h, _buf(src), _buf(dst), log2n, 1 if inverse else 0))
            return None
        out = ctypes.create_string_buffer(32 * n)
        self._check(self._lib.g16_ntt_fr(self._h, _buf(src), out, log2n, 1 if inverse else 0))
        return out.raw

    # ---- profiling -----------------------------------------------------------------------------
    def pairing(self, g1_points: bytes, g2_points: bytes) -> bytes:
        """e(P_i, Q_i) for n pairs -> n x 384 bytes (6 x Fp2 over w^k, Montgomery; curves.nim:218-221)"""
        n = len(g1_points) // 64
        assert len(g1_points) == 64 * n and len(g2_points) == 128 * n
        out = ctypes.create_string_buffer(max(1, GT_BYTES * n))
        self._check(self._lib.g16_pairing(self._h, _buf(g1_points) if n else None, _buf(g2_points) if n else None,
                                          n, out))
        return out.raw[:GT_BYTES * n]

    def profile(self, on):
        """False/0: off; True/1: HIP events around every kernel; 2: around the bucket-accumulation kernels only"""
        self._check(self._lib.g16_profile_enable(self._h, int(on)))

    def profile_reset(self):
        self._check(self._lib.g16_profile_reset(self._h))

    def profile_clock(self) -> float:
        """shader clock (GHz) sustained while the accumulate kernels since the last call ran (profiling on); 0 if none"""
        g = ctypes.c_double()
        self._check(self._lib.g16_profile_clock(self._h, ctypes.byref(g)))
        return g.value

    def profile_report(self) -> dict:
        buf = ctypes.create_string_buffer(1 << 16)
        self._check(self._lib.g16_profile_report(self._h, buf, len(buf)))
        return json.loads(buf.value.decode())


class ProvingKey:
    """Device-resident proving key (g16_pkey): registered ProverPoints + CSR of the A/B matrices."""

    def __init__(self, ctx: Context, desc: PkeyDesc, keepalive, section4: bytes = None, table_stride: int = 0):
        """section4: the .zkey file's coefficient section as it lies on disk (g16_pkey_create_zkey); desc.coeffs must
        then be NULL.  table_stride: all five point sets as lean sets (Context.register_points)"""
        self.ctx = ctx
        h = ctypes.c_void_p()
        if table_stride and section4 is not None:
            ctx._check(ctx._lib.g16_pkey_create_zkey_lean(ctx._h, ctypes.byref(desc), _buf(section4), len(section4),
                                                          table_stride, ctypes.byref(h)))
        elif table_stride:
            ctx._check(ctx._lib.g16_pkey_create_lean(ctx._h, ctypes.byref(desc), table_stride, ctypes.byref(h)))
        elif section4 is not None:
            ctx._check(ctx._lib.g16_pkey_create_zkey(ctx._h, ctypes.byref(desc), _buf(section4), len(section4),
                                                     ctypes.byref(h)))
        else:
            ctx._check(ctx._lib.g16_pkey_create(ctx._h, ctypes.byref(desc), ctypes.byref(h)))
        self._h = h
        self.nvars, self.npubs, self.log2n = desc.nvars, desc.npubs, desc.log2_domain
        ctx._children.add(self)
        del keepalive

    # Every call takes an optional `ctx`: the key is a per-DEVICE constant, and any context of its device may
    # prove against it -- several proofs in flight on one GPU = several contexts (private streams + workspaces)
    # sharing ONE resident key.  Default: the context the key was created through.
    def _check_len(self, witness):
        # the C ABI takes a bare pointer and reads nvars * 32 bytes: refuse a short host buffer here
        # (generateProofWithMask's "wrong witness length", prover.nim:236)
        if isinstance(witness, (bytes, bytearray)) and len(witness) != 32 * self.nvars:
            raise ValueError(f"wrong witness length: {len(witness)} bytes, expected {32 * self.nvars}")

    def prove(self, witness, mont: bool = True, r: bytes = None, s: bytes = None, device: bool = False, ctx=None):
        """-> (pi_a 64 B, pi_b 128 B, pi_c 64 B); r, s: Fr Montgomery bytes or None (trivial mask)."""
        c = ctx or self.ctx
        self._check_len(witness)
        out = ctypes.create_string_buffer(256)
        flags = (SCALARS_MONT if mont else 0) | (SCALARS_DEVICE if device else 0)
        c._check(c._lib.g16_prove(c._h, self._h, _buf(witness), flags, _buf(r) if r else None,
                                  _buf(s) if s else None, out))
        raw = out.raw
        return raw[0:64], raw[64:192], raw[192:256]

    def prove_partials(self, witness, mont: bool = True, device: bool = False, out=None, ctx=None):
        """this rank's five XYZZ MSM partials (768 bytes); out = device pointer to write them into HBM."""
        c = ctx or self.ctx
        self._check_len(witness)
        flags = (SCALARS_MONT if mont else 0) | (SCALARS_DEVICE if device else 0)
        if out is not None:
            c._check(c._lib.g16_prove_partials(c._h, self._h, _buf(witness), flags | OUT_DEVICE, _buf(out)))
            return None
        buf = ctypes.create_string_buffer(PARTIALS_BYTES)
        c._check(c._lib.g16_prove_partials(c._h, self._h, _buf(witness), flags, buf))
        return buf.raw

    def prove_partials_begin(self, witness, task_mask: int, task_out=None, mont: bool = True, device: bool = False,
                             ctx=None, nosync: bool = False):
        """first half of a sharded proof with a task-parallel quotient: launches this key's witness MSMs and writes
        the coset vectors named by task_mask (bit 0: A, 1: B, 2: C) to the device pointer task_out.  nosync: do not
        wait for the coset vectors on the host (G16_NO_HOST_SYNC: the caller orders its exchange behind them through
        the context's stream)"""
        c = ctx or self.ctx
        self._check_len(witness)
        flags = (SCALARS_MONT if mont else 0) | (SCALARS_DEVICE if device else 0) | (NO_HOST_SYNC if nosync else 0)
        c._check(c._lib.g16_prove_partials_begin(c._h, self._h, _buf(witness), flags, task_mask,
                                                 _buf(task_out) if task_out is not None else None))

    def prove_partials_end(self, a1, b1, c1, out=None, ctx=None, nosync: bool = False):
        """second half: a1 / b1 / c1 = device pointers to this key's [h_lo, h_hi) slices of the three coset vectors
        (None for an empty range); -> the 768-byte record (or written to the device pointer `out`)"""
        c = ctx or self.ctx
        ptr = lambda x: _buf(x) if x is not None else None          # noqa: E731
        if out is not None:
            c._check(c._lib.g16_prove_partials_end(c._h, self._h, ptr(a1), ptr(b1), ptr(c1),
                                                   OUT_DEVICE | (NO_HOST_SYNC if nosync else 0), _buf(out)))
            return None
        buf = ctypes.create_string_buffer(PARTIALS_BYTES)
        c._check(c._lib.g16_prove_partials_end(c._h, self._h, ptr(a1), ptr(b1), ptr(c1), 0, buf))
        return buf.raw

    def prove_combine(self, partials, count: int, r: bytes = None, s: bytes = None, device: bool = False, ctx=None):
        c = ctx or self.ctx
        out = ctypes.create_string_buffer(256)
        c._check(c._lib.g16_prove_combine(c._h, self._h, _buf(partials), count, SCALARS_DEVICE if device else 0,
                                          _buf(r) if r else None, _buf(s) if s else None, out))
        raw = out.raw
        return raw[0:64], raw[64:192], raw[192:256]

    def inf_counts(self) -> dict:
        """points at infinity per ProverPoints array (this shard) and whether A1 / B1+B2 use compacted entry lists"""
        out = (ctypes.c_size_t * 8)()
        self.ctx._check(self.ctx._lib.g16_pkey_inf_counts(self._h, out))
        v = list(out)
        return {"A1": v[0], "B1": v[1], "B2": v[2], "C1": v[3], "H1": v[4], "B1_and_B2": v[5],
                "compact_A": bool(v[6]), "compact_B": bool(v[7])}

    def b1_fold(self) -> dict:
        """what the key keeps in place of pointsB1 (g16_pkey_b1_fold): form "PLAIN" (pointsB1), "EMPTY" (nothing: every
        wire's B1 point equals its A1 point) or "DELTA" (the differences B1 - A1), and the two counts over the whole
        wire range it was decided from"""
        out = (ctypes.c_size_t * 3)()
        self.ctx._check(self.ctx._lib.g16_pkey_b1_fold(self._h, out))
        return {"form": ("PLAIN", "EMPTY", "DELTA")[out[0]], "live_b1": out[1], "live_delta": out[2]}

    def b1_sparse(self) -> dict:
        """how a DELTA key runs its B1 job (g16_pkey_b1_sparse): `sparse` if from the witness values of its live wires
        alone (at most `max` live differences over the whole wire range), and the live differences in this key's range"""
        out = (ctypes.c_size_t * 3)()
        self.ctx._check(self.ctx._lib.g16_pkey_b1_sparse(self._h, out))
        return {"sparse": bool(out[0]), "live": out[1], "max": out[2]}

    def abc_info(self) -> dict:
        """shape of the A / B matrices as buildABC runs them (g16_pkey_abc_info)"""
        out = (ctypes.c_size_t * 11)()
        self.ctx._check(self.ctx._lib.g16_pkey_abc_info(self._h, out))
        v = list(out)
        names = ("L<=1", "L=2", "L<=4", "L<=8", "L<=16", "L<=32", "L<=64", "L<=128", "L>128")
        return {"ncoeffs": v[0], "dict_values": v[1], "rows_by_terms": dict(zip(names, v[2:]))}

    def build_abc(self, witness: bytes, mont: bool = True, ctx=None):
        c = ctx or self.ctx
        self._check_len(witness)
        n = 1 << self.log2n
        out = ctypes.create_string_buffer(3 * n * 32)
        c._check(c._lib.g16_build_abc(c._h, self._h, _buf(witness), SCALARS_MONT if mont else 0, out))
        raw = out.raw
        return raw[: 32 * n], raw[32 * n: 64 * n], raw[64 * n:]

    def _free(self):
        if self._h:                      # valid whether or not the creating context is still alive
            self.ctx._lib.g16_pkey_destroy(self._h)
        self._h = None

    destroy = _free

    def __del__(self):
        try:
            self._free()
        except Exception:
            pass


class R1csSystem:
    """Device-resident constraint system (g16_r1cs): A, B and C of a circuit as one row-balanced sparse matrix.  Like a
    ProvingKey it belongs to the device: any context of that device may check against it."""

    def __init__(self, ctx: Context, desc: R1csDesc, keepalive=None):
        self.ctx = ctx
        self._h = None
        h = ctypes.c_void_p()
        ctx._check(ctx._lib.g16_r1cs_create(ctx._h, ctypes.byref(desc), ctypes.byref(h)))
        self._h = h
        self.nvars, self.nconstraints = desc.nvars, desc.nconstraints
        ctx._children.add(self)
        del keepalive

    def info(self) -> dict:
        out = (ctypes.c_size_t * 4)()
        self.ctx._check(self.ctx._lib.g16_r1cs_info(self._h, out))
        return {"nvars": out[0], "nconstraints": out[1], "nnz": out[2], "dict_values": out[3]}

    def check(self, witness, mont: bool = True, device: bool = False, ctx=None) -> WitnessReport:
        """g16_witness_check.  witness: nvars x 32 bytes (or a device pointer with device=True)"""
        c = ctx or self.ctx
        if isinstance(witness, (bytes, bytearray)) and len(witness) != 32 * self.nvars:
            raise ValueError(f"wrong witness length: {len(witness)} bytes, expected {32 * self.nvars}")
        rep = WitnessReportC()
        flags = (SCALARS_MONT if mont else 0) | (SCALARS_DEVICE if device else 0)
        c._check(c._lib.g16_witness_check(c._h, self._h, _buf(witness), flags, ctypes.byref(rep)))
        none = ctypes.c_size_t(-1).value
        le = lambda a: int.from_bytes(bytes(a), "little")     # noqa: E731
        return WitnessReport(rep.failed, rep.constraints, rep.noncanonical_count,
                             None if rep.first_noncanonical == none else rep.first_noncanonical, rep.bad_count,
                             [f for f in rep.first_bad if f != none], le(rep.az), le(rep.bz), le(rep.cz))

    def _free(self):
        if self._h:                      # valid whether or not the creating context is still alive
            self.ctx._lib.g16_r1cs_destroy(self._h)
        self._h = None

    destroy = _free

    def __del__(self):
        try:
            self._free()
        except Exception:
            pass


class DeviceGroup:
    """g16_group: one proof sharded over several GPUs from ONE process, one host thread per device inside the library
    (the reference's Taskpool shape, msm.nim:96-122).  devices: HIP ordinals, one per member (repeats allowed)."""

    def __init__(self, devices):
        self._lib = load_library()
        arr = (ctypes.c_int32 * len(devices))(*devices)
        h = ctypes.c_void_p()
        rc = self._lib.g16_group_create(arr, len(devices), ctypes.byref(h))
        if rc != G16_OK:
            raise G16Error(rc, "g16_group_create failed")
        self._h, self.devices = h, list(devices)

    def _check(self, rc):
        if rc != G16_OK:
            raise G16Error(rc, self._lib.g16_group_last_error(self._h).decode())

    def size(self) -> int:
        return self._lib.g16_group_size(self._h)

    def load_key(self, desc: PkeyDesc, keepalive=None, table_stride: int = 0) -> "GroupKey":
        h = ctypes.c_void_p()
        if table_stride:
            self._check(self._lib.g16_group_pkey_create_lean(self._h, ctypes.byref(desc), table_stride, ctypes.byref(h)))
        else:
            self._check(self._lib.g16_group_pkey_create(self._h, ctypes.byref(desc), ctypes.byref(h)))
        return GroupKey(self, h, desc.nvars)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.g16_group_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GroupKey:
    def __init__(self, group: DeviceGroup, handle, nvars: int):
        self.group, self._h, self.nvars = group, handle, nvars

    def prove(self, witness: bytes, mont: bool = True, r: bytes = None, s: bytes = None):
        """-> (pi_a, pi_b, pi_c): g16_group_prove, bit-identical to ProvingKey.prove on the unsharded key"""
        if len(witness) != 32 * self.nvars:
            raise ValueError(f"wrong witness length: {len(witness)} bytes, expected {32 * self.nvars}")
        out = ctypes.create_string_buffer(256)
        g = self.group
        g._check(g._lib.g16_group_prove(g._h, self._h, _buf(witness), SCALARS_MONT if mont else 0,
                                        _buf(r) if r else None, _buf(s) if s else None, out))
        raw = out.raw
        return raw[0:64], raw[64:192], raw[192:256]

    def destroy(self):
        if self._h:
            self.group._lib.g16_group_pkey_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class ProverPool:
    """g16_prover: `depth` proofs in flight on one GPU from ONE host thread, against one resident key (include/g16hip.h,
    "prover pool").  submit() never waits for the GPU and accepts depth + 1 outstanding proofs (the extra one's witness
    uploads while the others run); collect() returns what ProvingKey.prove returns for the same inputs.  The witness
    object is kept alive here until its proof is collected."""

    def __init__(self, pkey: ProvingKey, depth: int = 3, device: int = 0):
        self._lib = load_library()
        self.pkey, self.depth, self.device = pkey, depth, device   # the key must outlive the pool
        h = ctypes.c_void_p()
        rc = self._lib.g16_prover_create(device, pkey._h, depth, ctypes.byref(h))
        if rc != G16_OK:
            raise G16Error(rc, "g16_prover_create failed (sharded key, key of another device, or depth not in 1..8)")
        self._h = h
        self._witness = {}                 # ticket -> witness object (the library reads it until the proof is done)

    def _check(self, rc):
        if rc == G16_EBUSY:
            raise G16Error(rc, f"{self.depth + 1} proofs outstanding: collect one first")
        if rc < 0:
            raise G16Error(rc, self._lib.g16_prover_last_error(self._h).decode())
        return rc

    def submit(self, witness, mont: bool = True, r: bytes = None, s: bytes = None, device: bool = False) -> int:
        """-> ticket.  witness: bytes / bytearray / numpy array / HostBuffer, or with device=True a device pointer (int)
        or a GPU tensor (the caller orders its writes before the call, e.g. torch.cuda.synchronize()); r, s: Fr
        Montgomery bytes or None.  Raises G16Error with code G16_EBUSY when depth + 1 proofs are outstanding."""
        self.pkey._check_len(witness)
        if isinstance(witness, HostBuffer) and witness.nbytes < 32 * self.pkey.nvars:
            raise ValueError("host buffer shorter than the witness")
        ptr = ctypes.c_void_p(witness.data_ptr()) if device and hasattr(witness, "data_ptr") else _buf(witness)
        t = ctypes.c_uint64()
        flags = (SCALARS_MONT if mont else 0) | (SCALARS_DEVICE if device else 0)
        self._check(self._lib.g16_prover_submit(self._h, ptr, flags, _buf(r) if r else None,
                                                _buf(s) if s else None, ctypes.byref(t)))
        self._witness[t.value] = witness
        return t.value

    def poll(self, ticket: int) -> bool:
        return self._check(self._lib.g16_prover_poll(self._h, ticket)) == 1

    def collect(self, ticket: int):
        """-> (pi_a 64 B, pi_b 128 B, pi_c 64 B); waits for the proof"""
        out = ctypes.create_string_buffer(256)
        self._check(self._lib.g16_prover_collect(self._h, ticket, out))
        self._witness.pop(ticket, None)
        raw = out.raw
        return raw[0:64], raw[64:192], raw[192:256]

    def close(self):
        """waits for the outstanding proofs and discards them"""
        if getattr(self, "_h", None):
            self._lib.g16_prover_destroy(self._h)
            self._h = None
            self._witness.clear()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HostBuffer:
    """Pinned (page-locked) host memory from g16_host_alloc: a witness in it uploads without blocking submit().
    `.array` is a uint8 numpy view; the buffer passes anywhere a host pointer is taken."""

    def __init__(self, nbytes: int, device: int = 0):
        import numpy as np
        self._lib = load_library()
        p = ctypes.c_void_p()
        rc = self._lib.g16_host_alloc(device, nbytes, ctypes.byref(p))
        if rc != G16_OK:
            raise G16Error(rc, "g16_host_alloc failed")
        self._p, self.nbytes = p, nbytes
        self.array = np.ctypeslib.as_array((ctypes.c_uint8 * nbytes).from_address(p.value))
        self.ctypes = self.array.ctypes    # (_buf takes the pointer from here)

    @classmethod
    def from_bytes(cls, data: bytes, device: int = 0) -> "HostBuffer":
        import numpy as np
        b = cls(len(data), device)
        b.array[:] = np.frombuffer(data, dtype=np.uint8)
        return b

    def __len__(self):
        return self.nbytes

    def free(self):
        if getattr(self, "_p", None):
            self.array = self.ctypes = None
            self._lib.g16_host_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class VerifyingKey:
    """Device-resident verification key (g16_vkey): IC points, gamma2, delta2 and the Miller value of
    (alpha1, beta2) -- the reference's VKey (zkey_types.nim:62-73)."""

    def __init__(self, ctx: Context, npubs: int, alpha1: bytes, beta2: bytes, gamma2: bytes, delta2: bytes,
                 pointsIC: bytes):
        assert len(alpha1) == 64 and len(beta2) == len(gamma2) == len(delta2) == 128
        assert len(pointsIC) == 64 * (npubs + 1), "pointsIC must hold npubs + 1 points"
        self.ctx, self.npubs = ctx, npubs
        bufs = [ctypes.create_string_buffer(x, len(x)) for x in (alpha1, beta2, gamma2, delta2, pointsIC)]
        a = [ctypes.cast(b, ctypes.c_void_p) for b in bufs]
        desc = VkeyDesc(npubs, a[0], a[1], a[2], a[3], a[4])
        h = ctypes.c_void_p()
        ctx._check(ctx._lib.g16_vkey_create(ctx._h, ctypes.byref(desc), ctypes.byref(h)))
        self._h = h
        ctx._children.add(self)

    def verify(self, proofs, public_io: bytes, mont: bool = True, subgroup: bool = False):
        """proofs: list of (pi_a, pi_b, pi_c) byte triples; public_io: len(proofs) x (npubs+1) Fr scalars (each row
        starts with the constant 1, like Proof.publicIO).  -> list of status codes (1 ok, 0 fails, <0 malformed)."""
        n = len(proofs)
        assert len(public_io) == 32 * n * (self.npubs + 1)
        raw = b"".join(a + b + c for a, b, c in proofs)
        assert len(raw) == 256 * n
        st = (ctypes.c_int32 * max(n, 1))()
        flags = (SCALARS_MONT if mont else 0) | (VERIFY_SUBGROUP if subgroup else 0)
        self.ctx._check(self.ctx._lib.g16_verify(self.ctx._h, self._h, _buf(raw) if n else None,
                                                 _buf(public_io) if n else None, flags, n, st))
        return list(st)[:n]

    def verify_batch(self, proofs, public_io: bytes, mont: bool = True, multipliers=None, want_status: bool = False):
        """One pairing-product check for the whole batch (g16_verify_batch): True iff no proof has a structural defect
        and the combination of all pairing equations under the multipliers holds.  The order-r check of pi_b always
        runs.  multipliers: one int in [1, 2^128) per proof, unpredictable to whoever made the proofs; None draws
        them with `secrets`.  want_status: -> (bool, statuses); the statuses of a rejected batch are those of
        verify(..., subgroup=True), of an accepted one all 1."""
        n = len(proofs)
        assert len(public_io) == 32 * n * (self.npubs + 1)
        raw = b"".join(a + b + c for a, b, c in proofs)
        assert len(raw) == 256 * n
        if multipliers is None:
            import secrets
            multipliers = [secrets.randbelow((1 << 128) - 1) + 1 for _ in range(n)]
        assert len(multipliers) == n, "one multiplier per proof"
        zs = b"".join(int(z).to_bytes(16, "little") for z in multipliers)
        res = ctypes.c_int32(-1)
        st = (ctypes.c_int32 * max(n, 1))() if want_status else None
        flags = SCALARS_MONT if mont else 0
        self.ctx._check(self.ctx._lib.g16_verify_batch(self.ctx._h, self._h, _buf(raw) if n else None,
                                                       _buf(public_io) if n else None, flags, n,
                                                       _buf(zs) if n else None, ctypes.byref(res), st))
        return (res.value == 1, list(st)[:n]) if want_status else res.value == 1

    def _free(self):
        if self._h:
            self.ctx._lib.g16_vkey_destroy(self._h)
        self._h = None

    destroy = _free

    def __del__(self):
        try:
            self._free()
        except Exception:
            pass


def points_plan(group: int, n: int, table_stride: int = 0):
    """(window bits, tables, bytes of HBM) that registering n points of group 1 (G1) / 2 (G2) at table_stride would
    choose: g16_points_plan, a pure function -- no GPU, no context.  What a caller with a memory budget asks first."""
    lib = load_library()
    c, t, b = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_size_t()
    rc = lib.g16_points_plan(group, n, table_stride, ctypes.byref(c), ctypes.byref(t), ctypes.byref(b))
    if rc != G16_OK:
        raise G16Error(rc, "g16_points_plan: bad group, or too many points for 31-bit entry indices")
    return c.value, t.value, b.value


class PointSet:
    """Device-resident point set with precomputed window tables (g16_points)."""

    def __init__(self, ctx: Context, handle, group: int, n: int):
        self.ctx, self._h, self.group, self.n = ctx, handle, group, n
        ctx._children.add(self)

    def inf_count(self) -> int:
        """points at infinity (0,0) in the set"""
        return self.ctx._lib.g16_points_inf_count(self._h)

    def info(self):
        """(window bits c, number of tables)"""
        c, w = ctypes.c_uint32(), ctypes.c_uint32()
        self.ctx._check(self.ctx._lib.g16_points_info(self._h, ctypes.byref(c), ctypes.byref(w)))
        return c.value, w.value

    @property
    def table_bytes(self) -> int:
        """HBM held by the set's window tables (g16_points_table_bytes)"""
        b = ctypes.c_size_t()
        self.ctx._check(self.ctx._lib.g16_points_table_bytes(self._h, ctypes.byref(b)))
        return b.value

    def _free(self):
        if self._h:
            self.ctx._lib.g16_points_release(self._h)
        self._h = None

    release = _free

    def __del__(self):
        try:
            self._free()
        except Exception:
            pass


_default_ctx = None


def default_context() -> Context:
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(int(os.environ.get("LOCAL_RANK", "0")))
    return _default_ctx
