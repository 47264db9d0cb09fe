// TEST INFRASTRUCTURE ONLY -- stand-alone host program around lgar_py_amd/csrc/lgar_route.hpp.
//
// The per-output fold, the queue hand-over and the ordinate-gradient accumulation of the catchment-routing kernels are plain
// C++; with -DLGAR_DEVSIM they compile for the host (one lane after the other).  This program reads routing cases from a binary
// file, runs route_all / route_grad_all and writes the results, so the CPU tests (tests/test_route_host.py) can hold the SAME
// source the GPU executes against the reference's recorded queue and against the numpy statement of the recurrence -- also in an
// AddressSanitizer + UBSan build, which needs nothing loaded into python.  Every array is allocated at exactly its stated size,
// so a read past an end is a finding.  Never built or used by the product.
//
// File format (native endianness).  Input: int32 n_cases, then per case
//   int32 mode (0 route forward, 1 route reverse, 2 ordinate gradient), n_rows T, n_catchments B, n_ordinates K,
//         per_catchment, has_queue_in
//   double x[T][B]; modes 0, 1: double g[K][B] (per_catchment) or g[K]; mode 0 with has_queue_in: double queue_in[K][B];
//   mode 2: double gy[T][B]
// Output per case: mode 0: double y[T][B], queue_out[K][B]; mode 1: double y[T][B]; mode 2: double g_out[K][B].
#define LGAR_DEVSIM 1
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../lgar_py_amd/csrc/lgar_route.hpp"

namespace {

bool read_vec(FILE *f, std::vector<double> &v, size_t n) {
  v.resize(n);
  v.shrink_to_fit();
  return n == 0 || fread(v.data(), sizeof(double), n, f) == n;
}

bool write_vec(FILE *f, const std::vector<double> &v) { return v.empty() || fwrite(v.data(), sizeof(double), v.size(), f) == v.size(); }

int run_case(FILE *in, FILE *outf, const int32_t *h) {
  const int mode = h[0];
  const size_t T = (size_t)h[1], B = (size_t)h[2], K = (size_t)h[3];
  const bool per = h[4] != 0, has_q = h[5] != 0;
  std::vector<double> x, g, q_in, gy;
  if (!read_vec(in, x, T * B)) return 2;
  if (mode == 2) {
    if (!read_vec(in, gy, T * B)) return 2;
    std::vector<double> g_out(K * B, 777.0);  // (written, not added to)
    lgar::route_grad_all(x.data(), gy.data(), (long long)T, (long long)B, (int)K, g_out.data());
    return write_vec(outf, g_out) ? 0 : 3;
  }
  if (!read_vec(in, g, per ? K * B : K) || !read_vec(in, q_in, has_q ? K * B : 0)) return 2;
  std::vector<double> y(T * B, 777.0), q_out(mode == 0 ? K * B : 0, 777.0);
  const lgar::RouteArgs a = lgar::route_args(x.data(), (long long)T, (long long)B, g.data(), (int)K, per, has_q ? q_in.data() : nullptr,
                                             mode == 0 ? q_out.data() : nullptr, y.data(), mode == 1);
  lgar::route_all(a);
  return write_vec(outf, y) && write_vec(outf, q_out) ? 0 : 3;
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
  int32_t n_cases = 0;
  if (fread(&n_cases, 4, 1, in) != 1) return 2;
  for (int k = 0; k < n_cases; k++) {
    int32_t h[6];
    if (fread(h, 4, 6, in) != 6) return 2;
    // what the C-ABI wrappers themselves refuse (lgar_route.hip)
    if (h[0] < 0 || h[0] > 2 || h[1] < 0 || h[2] < 0 || h[3] < 1 || h[3] > LGAR_ROUTE_KMAX || (h[0] != 0 && h[5])) return 4;
    const int rc = run_case(in, out, h);
    if (rc) return rc;
  }
  fclose(in);
  return fclose(out) == 0 ? 0 : 3;
}
