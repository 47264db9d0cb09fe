// TEST INFRASTRUCTURE ONLY -- stand-alone host program around post_host.hpp.
//
// Reads calls of the six post-processing entry points from a binary file, runs each through its host-side launcher and writes
// the output arrays, so the CPU tests (tests/test_moisture_host.py, test_catchment_host.py, test_route_host.py) can hold the SAME
// source the GPU executes against the reference's own data and the numpy statements of the definitions -- also in an
// AddressSanitizer + UBSan build, which needs nothing loaded into python.  Every array is allocated at exactly its stated size,
// so a read past an end is a finding.  Never built or used by the product.
//
// File format (native endianness).  Input: int32 n_calls, then per call
//   int32 operation (the order of `run` below), n_scalars, n_arrays; int32 scalars[n_scalars]; then per array
//   int32 element size, kind (0 input, 1 output, 2 input and output, 3 absent: a null pointer), int64 length in elements,
//   and its data when it is an input.
// Output: per call its output arrays in order.  An output-only array starts as all-ones bytes (NaN): it is written, not added to.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "post_host.hpp"

namespace {

struct Array {
  std::unique_ptr<char[]> mem;
  size_t bytes = 0;
  int kind = 3;
  template <typename T> T *as() const { return (T *)mem.get(); }
};

// the operation's scalars (s) and arrays (a), in the order of its argument list; 4 = not a call this program knows
int dispatch(int op, const std::vector<int32_t> &s, const std::vector<Array> &a) {
  const size_t ns = s.size(), na = a.size();
  LgarDims d;
  memset(&d, 0, sizeof d);
  if (op == 0 && ns == 6 && na == 7 && s[2] >= 1) {  // dtype, n_layers, front_slots, n_columns, n_bins, what
    LgarParams p;
    LgarState st;
    memset(&p, 0, sizeof p);
    memset(&st, 0, sizeof st);
    d.n_layers = s[1], d.front_slots = s[2], d.n_columns = s[3];
    p.thickness = a[0].as<void>();
    st.depth = a[1].as<void>(), st.theta = a[2].as<void>(), st.flags = a[3].as<uint8_t>(), st.n_fronts = a[4].as<int32_t>();
    return posthost_soil_moisture(&d, &p, &st, a[5].as<double>(), s[4], s[5], a[6].as<void>(), s[0]);
  }
  if (op == 1 && ns == 3 && na == 8) {  // dtype, n_columns, n_rows; the seven summed series, running
    LgarStepOut so;
    memset(&so, 0, sizeof so);
    for (int j = 0; j < 7; j++) so.series[j] = a[j].as<void>();
    d.n_columns = s[1];
    return posthost_totals_replay(&d, &so, s[2], a[7].as<void>(), s[0]);
  }
  if (op == 2 && ns == 6 && na == 7)  // dtype, n_rows, n_columns, n_catchments, n_order, rows_per_wave
    return posthost_catchment_sums(a[0].as<void>(), s[1], s[2], a[1].as<int32_t>(), s[3], a[2].as<int32_t>(), s[4], a[3].as<void>(),
                                   a[4].as<int32_t>(), a[5].as<double>(), a[6].as<double>(), s[0], s[5]);
  if (op == 3 && ns == 4 && na == 5)  // dtype, n_rows, n_catchments, n_columns
    return posthost_catchment_spread(a[0].as<double>(), s[1], s[2], a[1].as<int32_t>(), s[3], a[2].as<void>(), a[3].as<int32_t>(),
                                     a[4].as<void>(), s[0]);
  if (op == 4 && ns == 5 && na == 5)  // n_rows, n_catchments, n_ordinates, per_catchment, reverse
    return posthost_catchment_route(a[0].as<double>(), s[0], s[1], a[1].as<double>(), s[2], s[3], a[2].as<double>(), a[3].as<double>(),
                                    a[4].as<double>(), s[4]);
  if (op == 5 && ns == 3 && na == 3)  // n_rows, n_catchments, n_ordinates
    return posthost_catchment_route_grad(a[0].as<double>(), a[1].as<double>(), s[0], s[1], s[2], a[2].as<double>());
  return 4;
}

int run_call(FILE *in, FILE *out) {
  int32_t h[3];
  if (fread(h, 4, 3, in) != 3 || h[1] < 0 || h[2] < 0) return 2;
  std::vector<int32_t> scalars((size_t)h[1]);
  if (h[1] && fread(scalars.data(), 4, scalars.size(), in) != scalars.size()) return 2;
  std::vector<Array> arrays((size_t)h[2]);
  for (Array &a : arrays) {
    int32_t eh[2];
    int64_t length;
    if (fread(eh, 4, 2, in) != 2 || fread(&length, 8, 1, in) != 1 || eh[0] < 1 || eh[1] < 0 || eh[1] > 3 || length < 0) return 2;
    a.kind = eh[1];
    if (a.kind == 3) continue;
    a.bytes = (size_t)eh[0] * (size_t)length;
    a.mem.reset(new char[a.bytes]);
    if (a.kind == 1) memset(a.mem.get(), 0xFF, a.bytes);
    else if (a.bytes && fread(a.mem.get(), 1, a.bytes, in) != a.bytes) return 2;
  }
  if (dispatch(h[0], scalars, arrays) != 0) return 4;  // (a refusal of the launcher included)
  for (const Array &a : arrays)
    if ((a.kind == 1 || a.kind == 2) && a.bytes && fwrite(a.mem.get(), 1, a.bytes, out) != a.bytes) return 3;
  return 0;
}

}  // namespace

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
    const int rc = run_call(in, out);
    if (rc) return rc;
  }
  fclose(in);
  return fclose(out) == 0 ? 0 : 3;
}
