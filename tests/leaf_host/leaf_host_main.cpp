// leaf_host_main.cpp -- TEST INFRASTRUCTURE ONLY: a stand-alone program around the leaf dispatchers' host build (leaf_host.cpp),
// for the AddressSanitizer + UBSan leg (tests/test_leaf_tangent_host.py): every op of leafhost_batch and of
// leafhost_tangent_batch, both precisions, both policies, every unit seed, over the edge points of the leaf grids -- the floats
// either side of the 0.1 cm cut, a zero and a huge head, Se = 1, 1 - 2^-52 and beyond 1, theta_e itself, a negative pow base.
// Prints "ok <items evaluated>".  Never built, loaded or referenced by the product package.
#include <cmath>
#include <cstdio>
#include <vector>

#include "leaf_host.cpp"

// operand sets by what an op promises to handle: 0 the leaves and the checked primitives (anything, their own domain's outside
// included), 1 the trapezoids (water contents of the domain, theta_e itself, and theta > theta_e: the NaN path), 2 the select-free
// log2 / exp2 cores (positive, finite, moderate: lgar_scalar.hpp)
static int operand_set(int op, bool tangent) {
  if (op == 4 || op == 6 || (!tangent && (op == 10 || op == 22))) return 1;
  if (op == 7 || op == 8 || (!tangent && (op == 13 || op == 14))) return 2;
  return 0;
}

template <typename R> static long sweep(int dtype) {
  const R te = R(0.43), tr = R(0.045), cut = R(0.1);
  const std::vector<R> xs[3] = {
      {R(0), std::nextafter(cut, R(0)), cut, std::nextafter(cut, R(1)), R(1e-30), R(37.5), R(1e6), R(3e38), R(1),
       R(1) - R(std::ldexp(1.0, -52)), R(1) - R(1e-9), R(0.5), R(1e-6), R(1.0000001), R(-0.25), te, R(0.2)},
      {tr + R(0.02) * (te - tr), R(0.2), tr + R(0.98) * (te - tr), te, R(0.5)},
      {R(1e-6), cut, R(0.5), R(1), R(37.5)}};
  const std::vector<R> ys[3] = {{te, R(0.3), R(2.0), R(0), R(-1.5)}, {te, R(0.3), R(2.0)}, {R(1)}};
  const R soils[3][3] = {{R(0.02), R(1.09), R(0.1)}, {R(0.04), R(3.5), R(20.0)}, {R(0.0075), R(1.56), R(1.04)}};
  long done = 0;
  for (const auto &s : soils)
    for (int set = 0; set < 3; set++)
      for (R yv : ys[set]) {
        const int n = (int)xs[set].size();
        std::vector<R> x(xs[set]), y(n, yv), alpha(n, s[0]), nn(n, s[1]), ksat(n, s[2]), e(n, te), r(n, tr), one(n, R(1)), out(n), tan(n);
        for (int op = 0; op <= LEAF_OP_LAST; op++) {
          if (operand_set(op, false) != set) continue;
          const int rc = leafhost_batch(op, n, x.data(), y.data(), 1.0, alpha.data(), nn.data(), ksat.data(), e.data(), r.data(), 120,
                                        15495.0, out.data(), dtype);
          if (rc != 0 && !(op >= LEAF_OP_F32_FIRST && dtype == LGAR_F64)) return -1;
          done += n;
        }
        for (int op = 0; op <= LEAF_TOP_LAST; op++) {
          if (!leaf_tangent_op_exists(op) || operand_set(op, true) != set) continue;
          for (int pol = 0; pol < 2; pol++)
            for (int sd = 0; sd < LEAF_NSEED; sd++) {
              const void *d[LEAF_NSEED] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
              d[sd] = one.data();
              if (leafhost_tangent_batch(op, pol, 0, n, x.data(), y.data(), 1.0, alpha.data(), nn.data(), ksat.data(), e.data(),
                                         r.data(), d[0], d[1], d[2], d[3], d[4], d[5], d[6], 120, 15495.0, out.data(), tan.data(),
                                         dtype) != 0)
                return -1;
              done += n;
            }
        }
      }
  return done;
}

// the argument checks in the form the HIP library runs them (leaf_tangent_check<false>: the shared trapezoid exists there)
static bool library_checks() {
  const double v = 0.0;
  auto rc = [&](int op, int pol, int share, int n, const void *y, const void *out, int dtype) {
    return leaf_tangent_check<false>(op, pol, share, n, &v, y, &v, &v, &v, &v, &v, out, out, dtype);
  };
  bool ok = rc(4, 0, 0, 1, &v, &v, LGAR_F64) == 0 && rc(4, 0, 0, 1, &v, &v, LGAR_F32) == 0;
  for (int share = 2; share <= 32; share++) ok = ok && rc(4, 0, share, 1, &v, &v, LGAR_F64) == 0;
  for (int share : {-1, 1, 33, 64}) ok = ok && rc(4, 0, share, 1, &v, &v, LGAR_F64) == LGAR_E_ARG;
  ok = ok && rc(4, 0, 9, 1, &v, &v, LGAR_F32) == LGAR_E_ARG;   // the shared trapezoid is double precision only
  ok = ok && rc(6, 0, 9, 1, &v, &v, LGAR_F64) == LGAR_E_ARG;   // ... and the fused trapezoid only
  ok = ok && rc(0, 0, 9, 1, &v, &v, LGAR_F64) == LGAR_E_ARG;
  for (int op : {-1, 10, 12, 15, 22, 33}) ok = ok && rc(op, 0, 0, 1, &v, &v, LGAR_F64) == LGAR_E_ARG;
  ok = ok && rc(4, 0, 0, 1, &v, nullptr, LGAR_F64) == LGAR_E_ARG && rc(4, 0, 0, 1, nullptr, &v, LGAR_F64) == LGAR_E_ARG;
  ok = ok && rc(4, 0, 0, 0, &v, &v, LGAR_F64) == LGAR_E_ARG && rc(4, 2, 0, 1, &v, &v, LGAR_F64) == LGAR_E_ARG;
  ok = ok && rc(4, 0, 0, 1, &v, &v, 7) == LGAR_E_ARG;
  return ok;
}

int main() {
  if (!library_checks()) {
    std::printf("an argument check failed\n");
    return 1;
  }
  const long a = sweep<double>(LGAR_F64), b = sweep<float>(LGAR_F32);
  if (a < 0 || b < 0) {
    std::printf("a call failed\n");
    return 1;
  }
  std::printf("ok %ld\n", a + b);
  return 0;
}
