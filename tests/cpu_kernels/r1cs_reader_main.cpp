// Stand-alone driver of the .r1cs reader of tools/g16_files.hpp for tests/test_setup_cpu.py, built with
// -fsanitize=address,undefined: reads the file named on the command line and prints its shape and a checksum of the
// triplets.  A file the reader rejects ends the program with status 1 and the reader's message; a sanitizer report ends
// it with another status.
#define G16_TOOL_NAME "r1cs_reader"
#include "../../tools/g16_files.hpp"

int main(int argc, char** argv) {
  if (argc != 2) die("usage: r1cs_reader file.r1cs");
  R1csFile rf(argv[1]);
  uint64_t sum = 0;
  size_t nnz[3];
  for (int k = 0; k < 3; ++k) {
    nnz[k] = rf.row[k].size();
    if (rf.col[k].size() != nnz[k] || rf.val[k].size() != 32 * nnz[k]) die("inconsistent triplets");
    for (size_t i = 0; i < nnz[k]; ++i) {
      sum = sum * 1000003u + rf.row[k][i];
      sum = sum * 1000003u + rf.col[k][i];
      for (int b = 0; b < 32; ++b) sum = sum * 1000003u + rf.val[k][32 * i + b];
    }
  }
  printf("r1cs ok: wires %u pubout %u pubin %u privin %u constraints %u nnz %zu %zu %zu checksum %llu\n", rf.nwires,
         rf.npubout, rf.npubin, rf.nprivin, rf.nconstraints, nnz[0], nnz[1], nnz[2], (unsigned long long)sum);
  return 0;
}
