// TEST INFRASTRUCTURE ONLY -- stand-alone host program around snow_host.hpp.
//
// Reads calls of the two catchment-snowpack entry points from a binary file, runs each through its host-side launcher and writes
// the output arrays, so tests/test_snow_host.py can hold the SAME source the GPU executes against the numpy statement of the
// definition -- also in an AddressSanitizer + UBSan build, which needs nothing loaded into python.  Every array is allocated at
// exactly its stated size (an array of no elements is a null pointer), so a read or write past an end is a finding.  Never built
// or used by the product.
//
// File format (native endianness).  Input: int32 n_calls, then per call eight int32 and one fp64 (dt_h)
//   forward (0):  0, T, B, has_state_in, wants_pack, wants_state_out, 0, 0;  par [7 B], p [T B], ta [T B], state_in [2 B] if
//                 has_state_in
//   adjoint (1):  1, T, B, has_state_in, has_gpack, wants_gta, wants_gpar, wants_gstate;  par [7 B], gw [T B], gice [T B] and
//                 gliq [T B] if has_gpack, p [T B], ta [T B], ice [T B], liq [T B], state_in [2 B] if has_state_in
// Output: per call w [T B] (+ ice [T B], liq [T B]) (+ state_out [2 B]), or gp [T B] (+ gta [T B]) (+ gpar [7 B]) (+ gstate [2 B]).
// An output starts as all-ones bytes (NaN): it is written, not added to.
#include <cstdio>
#include <cstring>
#include <memory>

#include "snow_host.hpp"

namespace {

struct Array {
  std::unique_ptr<double[]> mem;
  size_t n = 0;
  double *get() const { return n ? mem.get() : nullptr; }
  void size(size_t count) {
    n = count;
    if (n) mem.reset(new double[n]);
  }
  bool read(FILE *in, size_t count) {
    size(count);
    return n == 0 || fread(mem.get(), sizeof(double), n, in) == n;
  }
  void blank(size_t count) {
    size(count);
    if (n) memset(mem.get(), 0xFF, n * sizeof(double));
  }
  bool write(FILE *out) const { return n == 0 || fwrite(mem.get(), sizeof(double), n, out) == n; }
};

int run_call(FILE *in, FILE *out) {
  int32_t h[8];
  double dt_h = 0.0;
  if (fread(h, 4, 8, in) != 8 || fread(&dt_h, 8, 1, in) != 1 || h[1] < 0 || h[2] < 0) return 2;
  const int32_t op = h[0], T = h[1], B = h[2];
  const size_t TB = (size_t)T * (size_t)B, nB = (size_t)B;
  Array par, p, ta, ice, liq, gw, gice, gliq, state_in, o0, o1, o2, o3;
  if (op == 0) {
    if (!par.read(in, 7 * nB) || !p.read(in, TB) || !ta.read(in, TB) || (h[3] && !state_in.read(in, 2 * nB))) return 2;
    o0.blank(TB);
    if (h[4]) o1.blank(TB), o2.blank(TB);
    if (h[5]) o3.blank(2 * nB);
    // (an array of no elements is a null pointer: with T = 0 or B = 0 a wanted pack is "neither", which the entry point takes)
    if (snowhost_catchment_snow(p.get(), ta.get(), T, B, par.get(), dt_h, state_in.get(), o3.get(), o0.get(), o1.get(), o2.get()) != 0)
      return 4;
  } else if (op == 1) {
    if (!par.read(in, 7 * nB) || !gw.read(in, TB) || (h[4] && (!gice.read(in, TB) || !gliq.read(in, TB))) || !p.read(in, TB) ||
        !ta.read(in, TB) || !ice.read(in, TB) || !liq.read(in, TB) || (h[3] && !state_in.read(in, 2 * nB)))
      return 2;
    o0.blank(TB);
    if (h[5]) o1.blank(TB);
    if (h[6]) o2.blank(7 * nB);
    if (h[7]) o3.blank(2 * nB);
    if (snowhost_catchment_snow_grad(gw.get(), gice.get(), gliq.get(), p.get(), ta.get(), ice.get(), liq.get(), T, B, par.get(), dt_h,
                                     state_in.get(), o0.get(), o1.get(), o2.get(), o3.get()) != 0)
      return 4;
  } else {
    return 4;
  }
  return o0.write(out) && o1.write(out) && o2.write(out) && o3.write(out) ? 0 : 3;
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
