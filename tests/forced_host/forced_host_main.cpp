// forced_host_main.cpp -- TEST INFRASTRUCTURE ONLY: a stand-alone program around forced_host.cpp (also built with AddressSanitizer
// + UBSan).  window_host_main.cpp's job -- three columns of the Phillipsburg soil under two storms, every one-hot direction over
// (alpha, n, Ksat) x layer -- with a forcing direction beside each (a multiplier on the rain, another on the PET; either array
// NULL in turn): ONE call over T rows against the same rows cut at (0, 1), (1, 8), (8, T / 2), (T / 2, T - 1), (T - 1, T) with the
// end state of a chunk carried into the next.  Gradient, tangent series, status and both end states must agree bit for bit, and
// the forcing direction must move the gradient; in double and single precision, with and without the front-capacity chain.
// Prints "ok" and exits 0, or says what differed.
#include <cstdio>

#include "forced_host.cpp"

namespace {

constexpr int N = 3, L = 3, T = 24, F = LGAR_FMAX;

template <typename R> struct HostState {
  std::vector<R> depth, theta, psi, k, dzdt, scalars;
  std::vector<uint8_t> flags;
  std::vector<int32_t> nf;
  HostState() : depth(F * N), theta(F * N), psi(F * N), k(F * N), dzdt(F * N), scalars(LGAR_NSCAL * N), flags(F * N), nf(N) {}
  LgarState view() {
    LgarState s;
    std::memset(&s, 0, sizeof(s));
    s.depth = depth.data(); s.theta = theta.data(); s.psi = psi.data(); s.k = k.data(); s.dzdt = dzdt.data();
    s.flags = flags.data(); s.n_fronts = nf.data(); s.scalars = scalars.data();
    return s;
  }
  bool same(const HostState &o) const {
    return depth == o.depth && theta == o.theta && psi == o.psi && k == o.k && dzdt == o.dzdt && scalars == o.scalars &&
           flags == o.flags && nf == o.nf;
  }
};

template <typename V> bool same_bits(const V &a, const V &b) {
  return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(a[0])) == 0;
}

template <typename R> int run_case(int dtype, int search_mode) {
  const double soil[6][L] = {{0.0031297, 0.0083272, 0.0037454}, {1.6858, 1.299, 1.6151}, {0.45, 0.07, 0.45},
                             {0.4513, 0.4773, 0.4617},          {0.0648, 0.0831, 0.0668}, {44.0, 131.0, 25.0}};
  const double scale[N] = {1.0, 0.5, 1.3};
  std::vector<R> par[6];
  for (int j = 0; j < 6; j++) {
    par[j].resize(L * N);
    for (int l = 0; l < L; l++)
      for (int c = 0; c < N; c++) par[j][l * N + c] = (R)soil[j][l];
  }
  std::vector<R> precip(T * N), pet(T * N), wr(T * N), wp(T * N), dprecip(T * N), dpet(T * N);
  for (int t = 0; t < T; t++)
    for (int c = 0; c < N; c++) {
      const bool rain = (t >= 2 && t < 7) || (t >= 13 && t < 16);
      precip[t * N + c] = (R)(rain ? 2.0 * scale[c] : 0.0);
      pet[t * N + c] = (R)(rain ? 0.0 : 0.02);
      wr[t * N + c] = wp[t * N + c] = (R)(0.5 + (double)t / (T - 1));
      dprecip[t * N + c] = precip[t * N + c] * (R)(1.0 + 0.1 * c);
      dpet[t * N + c] = pet[t * N + c] * (R)(1.0 - 0.1 * c);
    }
  LgarDims d;
  std::memset(&d, 0, sizeof(d));
  d.n_columns = N; d.n_layers = L; d.num_subcycles = 1; d.nint = 120; d.n_giuh = 5; d.search_mode = search_mode;
  d.front_slots = F; d.dt_h = 1.0; d.initial_psi = 2000.0; d.ponded_depth_max = 0.0; d.wilting_point_psi = 15495.0;
  d.frozen_factor = 1.0;
  const double giuh[5] = {0.06, 0.51, 0.28, 0.12, 0.03};
  for (int i = 0; i < 5; i++) d.giuh[i] = giuh[i];
  const LgarParams p = {par[0].data(), par[1].data(), par[2].data(), par[3].data(), par[4].data(), par[5].data()};
  const int cuts[6] = {0, 1, 8, T / 2, T - 1, T};
  double moved = 0.0, forced = 0.0;
  for (int kind = 0; kind < 3; kind++)
    for (int layer = 0; layer < L; layer++) {
      std::vector<R> dir(L * N, R(0));
      for (int c = 0; c < N; c++) dir[layer * N + c] = R(1);
      LgarParams dp;
      std::memset(&dp, 0, sizeof(dp));
      (kind == 0 ? dp.alpha : kind == 1 ? dp.n : dp.ksat) = dir.data();
      // which of the two tangents this direction has: both, precipitation only, PET only
      const bool has_p = (kind + layer) % 3 != 2, has_e = (kind + layer) % 3 != 1;
      // one call
      HostState<R> v1, d1;
      std::vector<R> g1(N), s1(T * N);
      std::vector<int32_t> st1(N);
      {
        LgarState vo = v1.view(), to = d1.view();
        const LgarTangentWindow w = {nullptr, nullptr, &vo, &to, nullptr};
        const LgarForcing f = {precip.data(), pet.data(), nullptr};
        const LgarForcing df = {has_p ? dprecip.data() : nullptr, has_e ? dpet.data() : nullptr, nullptr};
        d.n_steps = T;
        if (forcedhost_forward_tangent_forced(&d, &p, &dp, &f, &df, wr.data(), wp.data(), &w, g1.data(), s1.data(), st1.data(), dtype) != 0) {
          std::printf("one call refused\n");
          return 1;
        }
        // the same call without the forcing direction: another gradient
        const LgarForcing none = {nullptr, nullptr, nullptr};
        const LgarTangentWindow w0 = {nullptr, nullptr, nullptr, nullptr, nullptr};
        std::vector<R> g0(N), s0(T * N);
        std::vector<int32_t> st0(N);
        if (forcedhost_forward_tangent_forced(&d, &p, &dp, &f, &none, wr.data(), wp.data(), &w0, g0.data(), s0.data(), st0.data(), dtype) != 0) {
          std::printf("the call without a forcing direction refused\n");
          return 1;
        }
        for (int c = 0; c < N; c++) forced += std::fabs((double)g1[c] - (double)g0[c]);
      }
      // the same rows in chunks
      HostState<R> v[2], t[2];
      std::vector<R> g[2] = {std::vector<R>(N), std::vector<R>(N)}, s2(T * N);
      std::vector<int32_t> st2(N);
      int cur = 0;
      for (int i = 0; i < 5; i++) {
        const int lo = cuts[i], hi = cuts[i + 1], nxt = 1 - cur;
        v[nxt] = HostState<R>();
        t[nxt] = HostState<R>();
        LgarState vi = v[cur].view(), ti = t[cur].view(), vo = v[nxt].view(), to = t[nxt].view();
        const LgarTangentWindow w = {i ? &vi : nullptr, i ? &ti : nullptr, &vo, &to, i ? g[cur].data() : nullptr};
        const LgarForcing f = {precip.data() + lo * N, pet.data() + lo * N, nullptr};
        const LgarForcing df = {has_p ? dprecip.data() + lo * N : nullptr, has_e ? dpet.data() + lo * N : nullptr, nullptr};
        d.n_steps = hi - lo;
        if (forcedhost_forward_tangent_forced(&d, &p, &dp, &f, &df, wr.data() + lo * N, wp.data() + lo * N, &w, g[nxt].data(),
                                              s2.data() + lo * N, st2.data(), dtype) != 0) {
          std::printf("chunk %d refused\n", i);
          return 1;
        }
        cur = nxt;
      }
      if (!same_bits(g1, g[cur]) || !same_bits(s1, s2) || !same_bits(st1, st2) || !v1.same(v[cur]) || !d1.same(t[cur])) {
        std::printf("dtype %d search_mode %d kind %d layer %d: the chunked run differs from one call\n", dtype, search_mode, kind, layer);
        return 1;
      }
      for (int c = 0; c < N; c++) moved += std::fabs((double)g1[c]);
    }
  if (!(moved > 0.0) || !(forced > 0.0)) {
    std::printf("dtype %d search_mode %d: the gradients are zero or the forcing direction does not move them, the case checks nothing\n",
                dtype, search_mode);
    return 1;
  }
  return 0;
}

}  // namespace

int main() {
  for (int mode = 1; mode <= 2; mode++) {
    if (run_case<double>(LGAR_F64, mode)) return 1;
    if (run_case<float>(LGAR_F32, mode)) return 1;
  }
  std::printf("ok\n");
  return 0;
}
