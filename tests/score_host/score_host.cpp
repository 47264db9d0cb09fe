// TEST INFRASTRUCTURE ONLY -- stand-alone host program around score_host.hpp.
//
// Reads calls of the two catchment-score entry points from a binary file, runs each through its host-side launcher and writes
// the output array, so tests/test_score_host.py can hold the SAME source the GPU executes against the numpy statement of the
// definition -- also in an AddressSanitizer + UBSan build, which needs nothing loaded into python.  Every array, the workspace
// included, is allocated at exactly its stated size, so a read or write past an end is a finding.  Never built or used by the
// product.
//
// File format (native endianness).  Input: int32 n_calls, then per call
//   int32 operation (0 moments, 1 gradient), n_obs_rows, n_catchments, window; then the fp64 input arrays in the order of the
//   argument list: sim [To * window * B], obs [To * B] and, for the gradient, moments [7 * B] and coef [4 * B].
// Output: per call its output array, moments [7 * B] or grad_sim [To * window * B].  An output starts as all-ones bytes (NaN): it
// is written, not added to.
#include <cstdio>
#include <cstring>
#include <memory>

#include "score_host.hpp"

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
};

int run_call(FILE *in, FILE *out) {
  int32_t h[4];
  if (fread(h, 4, 4, in) != 4 || h[1] < 0 || h[2] < 0 || h[3] < 1) return 2;
  const int32_t op = h[0], To = h[1], B = h[2], r = h[3];
  const size_t nsim = (size_t)To * (size_t)r * (size_t)B, nobs = (size_t)To * (size_t)B;
  Array sim, obs, result;
  if (!sim.read(in, nsim) || !obs.read(in, nobs)) return 2;
  if (op == 0) {
    Array ws;
    const int64_t bytes = scorehost_catchment_moments_workspace(To, B);
    if (bytes < 0) return 4;
    ws.blank((size_t)bytes / sizeof(double));
    result.blank((size_t)LGAR_SCORE_NMOM * (size_t)B);
    if (scorehost_catchment_moments(sim.get(), obs.get(), To, B, r, result.get(), ws.get()) != 0) return 4;
  } else if (op == 1) {
    Array moments, coef;
    if (!moments.read(in, (size_t)LGAR_SCORE_NMOM * (size_t)B) || !coef.read(in, 4 * (size_t)B)) return 2;
    result.blank(nsim);
    if (scorehost_catchment_moments_grad(sim.get(), obs.get(), To, B, r, moments.get(), coef.get(), result.get()) != 0) return 4;
  } else {
    return 4;
  }
  if (result.n && fwrite(result.get(), sizeof(double), result.n, out) != result.n) return 3;
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
