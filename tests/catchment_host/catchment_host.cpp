// TEST INFRASTRUCTURE ONLY -- stand-alone host program around lgar_py_amd/csrc/lgar_catchment.hpp.
//
// The per-lane accumulation and the combine order of the catchment-sums kernel are plain C++ templates; with -DLGAR_DEVSIM they
// compile for the host (the 64 lanes one after the other).  This program reads catchment maps and series from a binary file,
// runs catch_sum over every (row, catchment) and catch_spread over every (row, column) and writes the results, so the CPU tests
// (tests/test_catchment_host.py) can hold the SAME source the GPU executes against the numpy statement of the definition -- also
// in an AddressSanitizer + UBSan build, which needs nothing loaded into python.  Every array is allocated at exactly its stated
// size, so a read past a corrupt map's end is a finding.  Never built or used by the product.
//
// File format (native endianness).  Input: int32 n_cases, then per case
//   int32 dtype (0 fp32, 1 fp64), n_rows, n_columns, n_catchments, n_order (-1: no order array), has_weights, has_status,
//         n_grad_rows (0: no spread), rows_per_wave (1 or 4: how many rows a simulated wave carries its catchment through)
//   R series[n_rows][n_columns], int32 offsets[n_catchments + 1], int32 order[n_order], R weights[n_columns],
//   int32 status[n_columns], and for the spread int32 catchment_of[n_columns], double grad[n_grad_rows][n_catchments]
// Output: per case double sums[n_rows][n_catchments], double weight_sums[n_catchments], R spread[n_grad_rows][n_columns].
#define LGAR_DEVSIM 1
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../lgar_py_amd/csrc/lgar_catchment.hpp"

namespace {

template <typename T> bool read_vec(FILE *f, std::vector<T> &v, size_t n) {
  v.resize(n);
  v.shrink_to_fit();
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

template <typename T> bool write_vec(FILE *f, const std::vector<T> &v) {
  return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
}

template <typename R> int run_case(FILE *in, FILE *outf, const int32_t *h) {
  const size_t T = (size_t)h[1], N = (size_t)h[2], B = (size_t)h[3];
  const bool has_order = h[4] >= 0;
  const size_t n_order = has_order ? (size_t)h[4] : 0, TG = (size_t)h[7];
  std::vector<R> series, weights;
  std::vector<int32_t> offsets, order, status, cat;
  std::vector<double> grad;
  if (!read_vec(in, series, T * N) || !read_vec(in, offsets, B + 1) || !read_vec(in, order, n_order) ||
      !read_vec(in, weights, h[5] ? N : 0) || !read_vec(in, status, h[6] ? N : 0))
    return 2;
  if (TG && (!read_vec(in, cat, N) || !read_vec(in, grad, TG * B))) return 2;
  const R *w = h[5] ? weights.data() : nullptr;
  const int32_t *st = h[6] ? status.data() : nullptr;
  const int32_t *ord = has_order ? order.data() : nullptr;
  std::vector<double> sums(T * B), wsum(B);
  // rows_per_wave 1: one wave per (row, catchment); 4: the kernel's row groups of four (the last one ragged)
  const size_t NR = (size_t)h[8];
  for (size_t t = 0; t < T; t += NR) {
    const int rows = (int)(T - t < NR ? T - t : NR);
    const lgar::CatchRow<R> a = lgar::catch_row<R>(series.data() + t * N, rows, w, st, ord, (long long)n_order, (long long)N);
    for (size_t b = 0; b < B; b++) {
      double q[4];
      if (NR == 4) lgar::catch_sum<R, 4>(a, offsets.data(), (long long)b, q);
      else lgar::catch_sum<R, 1>(a, offsets.data(), (long long)b, q);
      for (int r = 0; r < rows; r++) sums[(t + r) * B + b] = q[r];
    }
  }
  const lgar::CatchRow<R> ones = lgar::catch_row<R>(nullptr, 1, w, st, ord, (long long)n_order, (long long)N);  // the weight sums
  for (size_t b = 0; b < B; b++) lgar::catch_sum<R, 1>(ones, offsets.data(), (long long)b, &wsum[b]);
  std::vector<R> spread(TG * N);
  for (size_t t = 0; t < TG; t++)
    for (size_t c = 0; c < N; c++)
      spread[t * N + c] = lgar::catch_spread<R>(grad.data() + t * B, (long long)B, cat[c], st ? st[c] : 0, w ? (double)w[c] : 1.0);
  return write_vec(outf, sums) && write_vec(outf, wsum) && write_vec(outf, spread) ? 0 : 3;
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
    int32_t h[9];
    if (fread(h, 4, 9, in) != 9) return 2;
    // what the C-ABI wrappers themselves refuse (lgar_kernels.hip)
    if ((h[0] != 0 && h[0] != 1) || h[1] < 0 || h[2] < 0 || h[3] < 0 || h[4] < -1 || h[7] < 0 || (h[8] != 1 && h[8] != 4)) return 4;
    const int rc = h[0] == 1 ? run_case<double>(in, out, h) : run_case<float>(in, out, h);
    if (rc) return rc;
  }
  fclose(in);
  return fclose(out) == 0 ? 0 : 3;
}
