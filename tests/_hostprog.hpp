// TEST INFRASTRUCTURE ONLY -- the one call-record protocol of the stand-alone host programs (tests/*_host/*_host.cpp).
//
// A program reads calls of its unit's entry points from a binary file, hands each to the unit's dispatch() and writes the
// output arrays, so the CPU tests can hold the SAME source the GPU executes against the numpy statements of the definitions --
// also in an AddressSanitizer + UBSan build, which needs nothing loaded into python.  Every array is allocated at exactly its
// stated size, so a read or write past an end is a finding.  tests/_hostbuild.py (HostUnit.run_calls) writes the records.
// Never built or used by the product.
//
// File format (native endianness).  Input: int32 n_calls, then per call
//   int32 operation, n_ints, n_doubles, n_arrays; int32 ints[n_ints]; fp64 doubles[n_doubles]; then per array
//   int32 element size, kind (0 input, 1 output, 2 input and output, 3 absent: a null pointer), int64 length in elements,
//   and its data when it is an input.
// Output: per call its output arrays in order.  An output-only array starts as all-ones bytes (NaN): it is written, not added to.
// Exit status: 1 usage or open, 2 short read or bad record, 3 write, 4 a call the unit does not know or refuses.
#ifndef LGAR_TESTS_HOSTPROG_HPP
#define LGAR_TESTS_HOSTPROG_HPP
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

namespace hostprog {

struct Array {
  std::unique_ptr<char[]> mem;
  size_t bytes = 0;
  int kind = 3;
  template <typename T> T *as() const { return (T *)mem.get(); }
  void blank(size_t n) {  // an output-only array of n bytes
    kind = 1, bytes = n;
    mem.reset(new char[n]);
    memset(mem.get(), 0xFF, n);
  }
};

using Ints = std::vector<int32_t>;
using Doubles = std::vector<double>;
using Arrays = std::vector<Array>;

}  // namespace hostprog

// The unit's part: the operation's scalars (i, d) and arrays (a), in the order of its argument list, to its entry point.  Returns
// the entry point's status (non-zero: a refusal), or 4 for a call the unit does not know.
int dispatch(int op, const hostprog::Ints &i, const hostprog::Doubles &d, const hostprog::Arrays &a);

namespace hostprog {

inline int run_call(FILE *in, FILE *out) {
  int32_t h[4];
  if (fread(h, 4, 4, in) != 4 || h[1] < 0 || h[2] < 0 || h[3] < 0) return 2;
  Ints ints((size_t)h[1]);
  Doubles doubles((size_t)h[2]);
  if (h[1] && fread(ints.data(), 4, ints.size(), in) != ints.size()) return 2;
  if (h[2] && fread(doubles.data(), 8, doubles.size(), in) != doubles.size()) return 2;
  Arrays arrays((size_t)h[3]);
  for (Array &a : arrays) {
    int32_t eh[2];
    int64_t length;
    if (fread(eh, 4, 2, in) != 2 || fread(&length, 8, 1, in) != 1 || eh[0] < 1 || eh[1] < 0 || eh[1] > 3 || length < 0) return 2;
    if (eh[1] == 3) continue;
    a.blank((size_t)eh[0] * (size_t)length);
    a.kind = eh[1];
    if (a.kind != 1 && a.bytes && fread(a.mem.get(), 1, a.bytes, in) != a.bytes) return 2;
  }
  if (dispatch(h[0], ints, doubles, arrays) != 0) return 4;  // (a refusal of the launcher included)
  for (const Array &a : arrays)
    if ((a.kind == 1 || a.kind == 2) && a.bytes && fwrite(a.mem.get(), 1, a.bytes, out) != a.bytes) return 3;
  return 0;
}

}  // namespace hostprog

int main(int argc, char **argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s <input> <output>\n", argv[0]);
    return 1;
  }
  FILE *in = fopen(argv[1], "rb");
  FILE *out = fopen(argv[2], "wb");
  if (!in || !out) return 1;
  int32_t n_calls = 0;
  if (fread(&n_calls, 4, 1, in) != 1) return 2;
  for (int k = 0; k < n_calls; k++) {
    const int rc = hostprog::run_call(in, out);
    if (rc) return rc;
  }
  fclose(in);
  return fclose(out) == 0 ? 0 : 3;
}
#endif
