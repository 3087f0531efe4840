// What a checker decides, as data (key audit, circuit audit, contribution chain, ptau verify and the element lists of the
// two contribute calls): the arrays it reads, which relation reads which array, what a finding is called and how the
// results of the pairing products fold into a report.  Host only, plain C++17 and no HIP header, so that the CPU test
// (tests/cpu_kernels/relation_plan_main.cpp) holds these tables to the Python models of the picture tests.  What is
// launched from them is checker.hpp.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/g16hip.h"

namespace g16 {

constexpr size_t NONE = (size_t)-1;   // "no such index" of every report

// ---- arrays: the name as error texts and reports spell it, and the group (1 = G1, 2 = G2, 0 = no points) ------------------
struct ArrayRow {
  const char* name;
  int group;
};
struct ArrayTable {
  const ArrayRow* row;
  int n;
  int nscan;   // the first `nscan` arrays are scanned for (0,0) after their element passes
};
constexpr ArrayRow KEY_ARRAY_ROWS[G16_AUDIT_SECTIONS] = {
    {"alpha1", 1},   {"beta1", 1},    {"delta1", 1},   {"beta2", 2},    {"gamma2", 2},   {"delta2", 2}, {"pointsIC", 1},
    {"pointsA1", 1}, {"pointsB1", 1}, {"pointsB2", 2}, {"pointsC1", 1}, {"pointsH1", 1}, {"coeffs", 0}};
constexpr ArrayRow PTAU_ARRAY_ROWS[G16_PTAU_REPORT_ARRAYS] = {
    {"tauG1", 1},         {"tauG2", 2},        {"alphaTauG1", 1},   {"betaTauG1", 1},    {"betaG2", 2},
    {"record tauG1", 1},  {"record alphaG1", 1}, {"record betaG1", 1}, {"record tauG2", 2}, {"record betaG2", 2},
    {"g1_s", 1},          {"g1_sx", 1},        {"g2_spx", 2},       {"challenges", 2}};
constexpr ArrayRow CHAIN_ARRAY_ROWS[G16_CHAIN_ARRAYS] = {
    {"delta_after", 1},  {"g1_s", 1},         {"g1_sx", 1},          {"g2_spx", 2},         {"challenges", 2},
    {"final delta1", 1}, {"final delta2", 2}, {"final pointsC1", 1}, {"final pointsH1", 1}};
constexpr ArrayRow KEY_CONTRIBUTE_ROWS[5] = {{"delta1", 1}, {"delta2", 2}, {"pointsC1", 1}, {"pointsH1", 1}, {"challenge", 2}};
constexpr ArrayRow PTAU_CONTRIBUTE_ROWS[6] = {{"ptau tauG1", 1},     {"ptau tauG2", 2}, {"ptau alphaTauG1", 1},
                                              {"ptau betaTauG1", 1}, {"ptau betaG2", 2}, {"challenges", 2}};
// the key audit's spec points go to spec_infinity; the circuit audit reads the file's five arrays and scans none; the
// chain scans up to G16_CHAIN_FINAL_DELTA2; g16_key_contribute refuses its three single points before it is entered
constexpr ArrayTable KEY_ARRAYS{KEY_ARRAY_ROWS, G16_AUDIT_SECTIONS - 1, 6};   // the points; coeffs: its own pass
constexpr ArrayTable CIRCUIT_PTAU_ARRAYS{PTAU_ARRAY_ROWS, G16_PTAU_SECTIONS, 0};
constexpr ArrayTable PTAU_ARRAYS{PTAU_ARRAY_ROWS, G16_PTAU_REPORT_ARRAYS, G16_PTAU_REPORT_ARRAYS};
constexpr ArrayTable CHAIN_ARRAYS{CHAIN_ARRAY_ROWS, G16_CHAIN_ARRAYS, G16_CHAIN_FINAL_DELTA2 + 1};
constexpr ArrayTable KEY_CONTRIBUTE_ARRAYS{KEY_CONTRIBUTE_ROWS, 5, 0};
constexpr ArrayTable PTAU_CONTRIBUTE_ARRAYS{PTAU_CONTRIBUTE_ROWS, 6, 6};
constexpr ArrayTable CIRCUIT_SETUP_ARRAYS{PTAU_CONTRIBUTE_ROWS, G16_PTAU_SECTIONS, 0};   // the file's five, as error texts

// ---- relations: the arrays one reads (bit a = array a), what else it needs, and its bit of `failed` -----------------------
enum Need : uint32_t { NEED_RECORDS = 1, NEED_VK = 2, NEED_MULTIPLIERS = 4 };
struct RelationRow {
  uint32_t reads;
  uint32_t need;
  uint32_t failed;
};
struct RelationTable {
  const RelationRow* row;
  int n;
  // the relations held per record: rows [from, to) of the record's `stride` rows of the product table; first_record[i]
  struct PerRecord {
    int relation, from, to;
  } rec[2];
  int stride;
};
constexpr uint32_t array_bits() { return 0; }
template <class... T>
constexpr uint32_t array_bits(int a, T... more) {
  return 1u << a | array_bits(more...);
}
constexpr uint32_t array_span(int from, int to) { return (2u << to) - (1u << from); }   // arrays from..to

constexpr RelationRow KEY_RELATION_ROWS[3] = {
    {array_bits(G16_SEC_POINTS_B1, G16_SEC_POINTS_B2), NEED_MULTIPLIERS, G16_AUDIT_RELATION},
    {array_bits(G16_SEC_BETA1, G16_SEC_BETA2), 0, G16_AUDIT_RELATION},
    {array_bits(G16_SEC_DELTA1, G16_SEC_DELTA2), 0, G16_AUDIT_RELATION}};
constexpr RelationTable KEY_RELATIONS{KEY_RELATION_ROWS, 3, {}, 0};

// the circuit audit: the key's sections, then ptau array p at bit CIRCUIT_PTAU_BIT + p
constexpr int CIRCUIT_PTAU_BIT = G16_AUDIT_SECTIONS;
constexpr uint32_t circuit_ptau(int p) { return 1u << (CIRCUIT_PTAU_BIT + p); }
constexpr uint32_t CIRCUIT_TAU1 = circuit_ptau(G16_PTAU_TAU_G1),
                   CIRCUIT_TAU1_A_B = CIRCUIT_TAU1 | circuit_ptau(G16_PTAU_ALPHA_TAU_G1) | circuit_ptau(G16_PTAU_BETA_TAU_G1);
constexpr RelationRow CIRCUIT_RELATION_ROWS[G16_CIRCUIT_RELATIONS] = {
    {array_bits(G16_SEC_COEFFS), 0, G16_CIRCUIT_COEFFS},
    {array_bits(G16_SEC_COEFFS), 0, G16_CIRCUIT_COEFFS},
    {array_bits(G16_SEC_ALPHA1, G16_SEC_BETA1, G16_SEC_BETA2) | array_span(CIRCUIT_PTAU_BIT, CIRCUIT_PTAU_BIT + 4), 0,
     G16_CIRCUIT_SPEC},   // all five ptau arrays
    {array_bits(G16_SEC_POINTS_A1) | CIRCUIT_TAU1, 0, G16_CIRCUIT_POINTS},
    {array_bits(G16_SEC_POINTS_B1) | CIRCUIT_TAU1, 0, G16_CIRCUIT_POINTS},
    {array_bits(G16_SEC_POINTS_B2) | circuit_ptau(G16_PTAU_TAU_G2), 0, G16_CIRCUIT_POINTS},
    {array_bits(G16_SEC_POINTS_C1, G16_SEC_DELTA2) | CIRCUIT_TAU1_A_B, 0, G16_CIRCUIT_POINTS},
    {array_bits(G16_SEC_POINTS_IC, G16_SEC_GAMMA2) | CIRCUIT_TAU1_A_B, NEED_VK, G16_CIRCUIT_POINTS},
    {array_bits(G16_SEC_POINTS_H1, G16_SEC_DELTA2) | CIRCUIT_TAU1, 0, G16_CIRCUIT_POINTS}};
constexpr RelationTable CIRCUIT_RELATIONS{CIRCUIT_RELATION_ROWS, G16_CIRCUIT_RELATIONS, {}, 0};

// the chain: ELEMENTS reads nothing here (it is the element pass itself).  Record j holds POK at row 2j, STEP at 2j + 1.
constexpr RelationRow CHAIN_RELATION_ROWS[G16_CHAIN_RELATIONS] = {
    {0, 0, 1u << G16_CHAIN_ELEMENTS},
    {array_bits(G16_CHAIN_G1_S, G16_CHAIN_G1_SX, G16_CHAIN_G2_SPX, G16_CHAIN_CHALLENGES), 0, 1u << G16_CHAIN_POK},
    {array_bits(G16_CHAIN_DELTA_AFTER, G16_CHAIN_G2_SPX, G16_CHAIN_CHALLENGES), 0, 1u << G16_CHAIN_STEP},
    {array_bits(G16_CHAIN_DELTA_AFTER, G16_CHAIN_FINAL_DELTA1), 0, 1u << G16_CHAIN_LAST},
    {array_bits(G16_CHAIN_FINAL_DELTA1, G16_CHAIN_FINAL_DELTA2), 0, 1u << G16_CHAIN_DELTA},
    {array_bits(G16_CHAIN_FINAL_DELTA2, G16_CHAIN_FINAL_POINTS_C1), 0, 1u << G16_CHAIN_C1},
    {array_bits(G16_CHAIN_FINAL_DELTA2, G16_CHAIN_FINAL_POINTS_H1), 0, 1u << G16_CHAIN_H1}};
constexpr RelationTable CHAIN_RELATIONS{
    CHAIN_RELATION_ROWS, G16_CHAIN_RELATIONS, {{G16_CHAIN_POK, 0, 1}, {G16_CHAIN_STEP, 1, 2}}, 2};

// ptau verify: STEP is checked only where POK holds, so its arrays contain POK's.  Record j: three POK rows, five STEP rows.
constexpr uint32_t PTAU_TAU = array_bits(G16_PTAU_TAU_G1, G16_PTAU_TAU_G2);
constexpr RelationRow PTAU_RELATION_ROWS[G16_PTAU_RELATIONS] = {
    {0, 0, 1u << G16_PTAUV_ELEMENTS},
    {PTAU_TAU, 0, 1u << G16_PTAUV_FIRST},
    {PTAU_TAU, 0, 1u << G16_PTAUV_TAU_G1},
    {PTAU_TAU, 0, 1u << G16_PTAUV_TAU_G2},
    {array_bits(G16_PTAU_ALPHA_TAU_G1, G16_PTAU_TAU_G2), 0, 1u << G16_PTAUV_ALPHA},
    {array_bits(G16_PTAU_BETA_TAU_G1, G16_PTAU_TAU_G2), 0, 1u << G16_PTAUV_BETA},
    {array_bits(G16_PTAU_BETA_TAU_G1, G16_PTAU_BETA_G2), 0, 1u << G16_PTAUV_BETA_G2},
    {array_span(G16_PTAUV_G1_S, G16_PTAUV_CHALLENGES), NEED_RECORDS, 1u << G16_PTAUV_POK},
    {array_span(G16_PTAUV_REC_TAU_G1, G16_PTAUV_CHALLENGES), NEED_RECORDS, 1u << G16_PTAUV_STEP},
    {array_span(G16_PTAU_TAU_G1, G16_PTAUV_REC_BETA_G2), NEED_RECORDS, 1u << G16_PTAUV_LAST}};
constexpr int PTAU_FIXED_ROWS = 5;   // TAU_G1, TAU_G2, ALPHA, BETA, BETA_G2, before the records' rows
constexpr RelationTable PTAU_RELATIONS{
    PTAU_RELATION_ROWS, G16_PTAU_RELATIONS, {{G16_PTAUV_POK, 0, 3}, {G16_PTAUV_STEP, 3, 8}}, 8};

// bit a: array a has an element that fails a check of the element passes
inline uint32_t dirty_mask(const size_t (*bad_count)[3], int n) {
  uint32_t m = 0;
  for (int a = 0; a < n; ++a)
    if (bad_count[a][0] | bad_count[a][1] | bad_count[a][2]) m |= 1u << a;
  return m;
}
// run[k]: every array relation k reads is clean (bit a of `clean`) and everything else it needs is there (`have`: Need bits)
inline void relations_run(const RelationTable& t, uint32_t clean, uint32_t have, bool* run) {
  for (int k = 0; k < t.n; ++k) run[k] = !(t.row[k].reads & ~clean) && !(t.row[k].need & ~have);
}

// The end of a checker.  The per-record relations that ran are read off the product results (`result`: the first row of
// record 0): one holds if none of its rows is 0, else first_record[i] is the first record with such a row.  Then every
// relation that is 0 sets its bit of `failed`.
inline void fold_report(const RelationTable& t, const bool* run, const int32_t* result, size_t count, int32_t* relation,
                        size_t* first_record, uint32_t& failed) {
  for (int i = 0; i < 2 && t.stride; ++i) {
    const RelationTable::PerRecord& r = t.rec[i];
    if (!run[r.relation]) continue;
    relation[r.relation] = 1;
    for (size_t j = 0; j < count && relation[r.relation]; ++j)
      for (int q = r.from; q < r.to; ++q)
        if (!result[t.stride * j + q]) {
          relation[r.relation] = 0, first_record[i] = j;
          break;
        }
  }
  for (int k = 0; k < t.n; ++k)
    if (relation[k] == 0) failed |= t.row[k].failed;
}

// a report before its checker runs: all zero, every relation "not run", no record and no (0,0) found
template <class Report>
inline void report_reset(Report* out) {
  memset(out, 0, sizeof *out);
  for (int32_t& r : out->relation) r = -1;
  for (size_t& f : out->first_record) f = NONE;
  for (size_t& f : out->first_infinity) f = NONE;
}

// ---- findings ----------------------------------------------------------------------------------------------------------
constexpr const char* CHECK_TEXT[3] = {"is not a canonical encoding", "is not on the curve", "is not in the order-r subgroup"};
// "<name>[<first>] <check>", and " (and <count - 1> more)" if there are more
inline std::string finding_text(const char* name, size_t first, int check, size_t count) {
  std::string text = std::string(name) + "[" + std::to_string(first) + "] " + CHECK_TEXT[check];
  if (count > 1) text += " (and " + std::to_string(count - 1) + " more)";
  return text;
}
inline std::string infinity_text(const char* name, size_t i) {
  return std::string(name) + "[" + std::to_string(i) + "] is the point at infinity";
}
// is the point of `bytes` (64 or 128) at p the all-zero encoding (0,0)?
inline bool is_infinity(const void* p, size_t bytes) {
  static const unsigned char zeros[128] = {};
  return !memcmp(p, zeros, bytes);
}

}  // namespace g16
