// Prints what relation_plan.hpp decides, for tests/test_relation_plan_cpu.py: the tables of every checker, run[] for
// every single dirty array and every flag, fold_report over planted product results, and the finding texts.  A
// stand-alone program: the test compiles it with -fsanitize=address,undefined, which makes it the bounds check of the
// tables and of the row arithmetic of fold_report.  Fields are separated by tabs (array names hold blanks).
#include <cstdio>
#include <memory>
#include <vector>

#include "../../nim_groth16_amd/csrc/relation_plan.hpp"

using namespace g16;

struct Checker {
  const char* name;
  const ArrayTable* arrays;
  const RelationTable* relations;
  int narrays;         // bits of `clean` the relations read
  size_t fixed_rows;   // rows of the product table before record 0
  size_t tail_rows;    // ... and behind the last record
};
static const Checker CHECKERS[] = {{"key", &KEY_ARRAYS, &KEY_RELATIONS, G16_AUDIT_SECTIONS, 0, 0},
                                   {"circuit", &CIRCUIT_PTAU_ARRAYS, &CIRCUIT_RELATIONS, CIRCUIT_PTAU_BIT + G16_PTAU_SECTIONS, 0, 0},
                                   {"chain", &CHAIN_ARRAYS, &CHAIN_RELATIONS, G16_CHAIN_ARRAYS, 0, 3},
                                   {"ptau", &PTAU_ARRAYS, &PTAU_RELATIONS, G16_PTAU_REPORT_ARRAYS, PTAU_FIXED_ROWS, 0},
                                   {"key_contribute", &KEY_CONTRIBUTE_ARRAYS, nullptr, 0, 0, 0},
                                   {"ptau_contribute", &PTAU_CONTRIBUTE_ARRAYS, nullptr, 0, 0, 0},
                                   {"circuit_setup", &CIRCUIT_SETUP_ARRAYS, nullptr, 0, 0, 0}};

static void print_run(const Checker& c, uint32_t clean, uint32_t have) {
  std::unique_ptr<bool[]> run(new bool[c.relations->n]);   // on the heap, exactly n: the sanitizer guards the bytes behind
  relations_run(*c.relations, clean, have, run.get());
  std::printf("run\t%s\t%u\t%u", c.name, clean, have);
  for (int k = 0; k < c.relations->n; ++k) std::printf("\t%d", run[k]);
  std::printf("\n");
}

// every product holds but those of `zeros` (rows of the records, counted from record 0); the fixed relations hold
static void print_fold(const Checker& c, size_t count, const std::vector<size_t>& zeros, int not_run) {
  const RelationTable& t = *c.relations;
  std::vector<int32_t> result(c.fixed_rows + t.stride * count + c.tail_rows, 1), relation(t.n, 1);
  std::unique_ptr<bool[]> run(new bool[t.n]);
  for (int k = 0; k < t.n; ++k) run[k] = k != not_run;
  std::vector<size_t> first_record(2, NONE);
  for (size_t z : zeros) result[c.fixed_rows + z] = 0;
  for (int i = 0; i < 2; ++i) relation[t.rec[i].relation] = -1;
  if (not_run >= 0) relation[not_run] = -1;
  uint32_t failed = 0;
  fold_report(t, run.get(), result.data() + c.fixed_rows, count, relation.data(), first_record.data(), failed);
  std::printf("fold\t%s\t%zu\t%d\t", c.name, count, not_run);
  for (size_t z : zeros) std::printf("%zu,", z);
  std::printf("\t%u\t%lld\t%lld", failed, (long long)first_record[0], (long long)first_record[1]);
  for (int32_t r : relation) std::printf("\t%d", r);
  std::printf("\n");
}

int main() {
  for (const Checker& c : CHECKERS) {
    for (int a = 0; a < c.arrays->n + (c.arrays == &KEY_ARRAYS ? 1 : 0); ++a)   // the key's coeffs: a row, no point array
      std::printf("array\t%s\t%d\t%s\t%d\t%d\n", c.name, a, c.arrays->row[a].name, c.arrays->row[a].group,
                  a < c.arrays->nscan);
    if (!c.relations) continue;
    const RelationTable& t = *c.relations;
    for (int k = 0; k < t.n; ++k)
      std::printf("relation\t%s\t%d\t%u\t%u\t%u\n", c.name, k, t.row[k].reads, t.row[k].need, t.row[k].failed);
    const uint32_t all = (c.narrays < 32 ? 1u << c.narrays : 0u) - 1;
    for (uint32_t have : {0u, (uint32_t)NEED_RECORDS, (uint32_t)NEED_VK, (uint32_t)NEED_MULTIPLIERS, 7u}) {
      print_run(c, all, have);
      for (int a = 0; a < c.narrays; ++a) print_run(c, all & ~(1u << a), have);
    }
    if (!t.stride) {
      std::vector<int32_t> relation(t.n, 1);
      relation[t.n - 1] = 0, relation[0] = -1;
      std::unique_ptr<bool[]> run(new bool[t.n]);
      for (int k = 0; k < t.n; ++k) run[k] = true;
      uint32_t failed = 0;
      fold_report(t, run.get(), nullptr, 0, relation.data(), nullptr, failed);
      std::printf("fold_fixed\t%s\t%u\n", c.name, failed);
      continue;
    }
    for (size_t count : {size_t(0), size_t(1), size_t(3)}) {
      print_fold(c, count, {}, -1);
      for (size_t z = 0; z < t.stride * count; ++z) {
        print_fold(c, count, {z}, -1);
        std::vector<size_t> from_z;
        for (size_t y = z; y < t.stride * count; ++y) from_z.push_back(y);
        print_fold(c, count, from_z, -1);
        for (int i = 0; i < 2; ++i) print_fold(c, count, from_z, t.rec[i].relation);
      }
    }
  }
  for (const char* name : {"tauG1", "ptau tauG1", "final pointsC1"})
    for (size_t first : {size_t(0), size_t(7), size_t(123456789012)}) {
      for (int check = 0; check < 3; ++check)
        for (size_t count : {size_t(1), size_t(2), size_t(17)})
          std::printf("finding\t%s\t%zu\t%d\t%zu\t%s\n", name, first, check, count,
                      finding_text(name, first, check, count).c_str());
      std::printf("infinity\t%s\t%zu\t%s\n", name, first, infinity_text(name, first).c_str());
    }
  std::vector<unsigned char> point(192, 0);
  point[63] = 1;
  std::printf("is_infinity\t%d\t%d\t%d\t%d\n", is_infinity(&point[0], 64), is_infinity(&point[64], 64), is_infinity(&point[1], 128),
              is_infinity(&point[64], 128));
  return 0;
}
