// TEST INFRASTRUCTURE ONLY -- stand-alone host program around lgar_py_amd/csrc/lgar_moisture.hpp.
//
// The per-column soil-moisture function the GPU kernel runs is a plain C++ template; with -DLGAR_DEVSIM it compiles for the
// host.  This program reads front tables from a binary file, runs the function over every column and writes the results, so the
// CPU tests (tests/test_moisture_host.py) can hold the SAME source the GPU executes against the reference's own front tables --
// also in an AddressSanitizer + UBSan build, which needs nothing loaded into python.  Never built or used by the product.
//
// File format (native endianness).  Input: int32 n_cases, then per case
//   int32 dtype (0 fp32, 1 fp64), n_layers, front_slots, n_columns, n_bins, layer_bins (0/1), what (0 theta, 1 storage)
//   R thickness[n_layers][n_columns], R depth[front_slots][n_columns], R theta[front_slots][n_columns]
//   uint8 flags[front_slots][n_columns], int32 n_fronts[n_columns], double edges[n_bins + 1] (absent when layer_bins)
// Output: per case R out[n_bins][n_columns].
#define LGAR_DEVSIM 1
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../lgar_py_amd/csrc/lgar_moisture.hpp"

namespace {

template <typename T> bool read_vec(FILE *f, std::vector<T> &v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

template <typename R> int run_case(FILE *in, FILE *outf, int L, int F, int N, int nb, int layer_bins, int what) {
  std::vector<R> thick, depth, theta, out((size_t)nb * N);
  std::vector<uint8_t> flags;
  std::vector<int32_t> nf;
  std::vector<double> edges;
  const size_t n = (size_t)N;
  if (!read_vec(in, thick, L * n) || !read_vec(in, depth, F * n) || !read_vec(in, theta, F * n) || !read_vec(in, flags, F * n) ||
      !read_vec(in, nf, n))
    return 2;
  if (!layer_bins && !read_vec(in, edges, (size_t)nb + 1)) return 2;
  for (size_t c = 0; c < n; c++) {
    // the kernel's dispatch (lgar_moisture.hip): layer bins, or the smallest compiled bin capacity that fits
    if (layer_bins)
      lgar::moist_column<R, 8, true>(depth.data(), theta.data(), flags.data(), nf.data(), thick.data(), nullptr, n, c, L, F, nb, what, out.data());
    else if (nb <= 8)
      lgar::moist_column<R, 8, false>(depth.data(), theta.data(), flags.data(), nf.data(), thick.data(), edges.data(), n, c, L, F, nb, what, out.data());
    else if (nb <= 16)
      lgar::moist_column<R, 16, false>(depth.data(), theta.data(), flags.data(), nf.data(), thick.data(), edges.data(), n, c, L, F, nb, what, out.data());
    else
      lgar::moist_column<R, LGAR_MOIST_BINS, false>(depth.data(), theta.data(), flags.data(), nf.data(), thick.data(), edges.data(), n, c, L, F, nb, what, out.data());
  }
  return fwrite(out.data(), sizeof(R), out.size(), outf) == out.size() ? 0 : 3;
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
    int32_t h[7];
    if (fread(h, 4, 7, in) != 7) return 2;
    const int dtype = h[0], L = h[1], F = h[2], N = h[3], nb = h[4], layer_bins = h[5], what = h[6];
    // what lgar_soil_moisture itself refuses (lgar_kernels.hip): the function is only ever called inside these bounds
    if (L < LGAR_LMIN || L > LGAR_LMAX || F < 1 || F > LGAR_FMAX || N < 1 || nb < 1 || nb > LGAR_MOIST_BINS ||
        (layer_bins && nb != L) || (what != 0 && what != 1) || (dtype != 0 && dtype != 1))
      return 4;
    const int rc = dtype == 1 ? run_case<double>(in, out, L, F, N, nb, layer_bins, what)
                              : run_case<float>(in, out, L, F, N, nb, layer_bins, what);
    if (rc) return rc;
  }
  fclose(in);
  return fclose(out) == 0 ? 0 : 3;
}
