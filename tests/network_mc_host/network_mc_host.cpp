// TEST INFRASTRUCTURE ONLY -- stand-alone host program around network_mc_host.hpp: the two Muskingum-Cunge network entry points
// and mc_ln under the call records of tests/_hostprog.hpp (tests/test_network_mc_host.py; tests/network_mc_host writes the records
// and passes an array of no elements as a null pointer).  The topology is taken as the file gives it, so a read or write past an
// end under a corrupt topology is a finding.  Never built or used by the product.
//
// Calls (ints; doubles; arrays: fp64, the topology int32)
//   0 forward:  T, B, E, n_levels; dt_h, rmin, rmax;  x [T B], par [4 B], up_ptr [B + 1], up_idx [E], order [B],
//               level_ptr [n_levels + 1], state_in [2 B] or absent, state_out [2 B], y [T B]
//   1 adjoint:  T, B, E, n_levels; dt_h, rmin, rmax;  gy [T B], par, down [B], order, level_ptr, gx [T B], x, y [T B], up_ptr,
//               up_idx, state_in, gpar [3 B], gstate [2 B]
//   2 mc_ln:    n;  x [n], out [n]
#include "network_mc_host.hpp"

#include "../_hostprog.hpp"

int dispatch(int op, const hostprog::Ints &i, const hostprog::Doubles &d, const hostprog::Arrays &a) {
  const size_t ni = i.size(), nd = d.size(), na = a.size();
  auto f = [&a](int k) { return a[k].as<double>(); };
  auto n = [&a](int k) { return a[k].as<int32_t>(); };
  if (op == 0 && ni == 4 && nd == 3 && na == 9)
    return networkmchost_network_route_mc(f(0), i[0], i[1], f(1), d[0], d[1], d[2], n(2), n(3), i[2], n(4), n(5), i[3], f(6), f(7), f(8));
  if (op == 1 && ni == 4 && nd == 3 && na == 13)
    return networkmchost_network_route_mc_grad(f(0), i[0], i[1], f(1), d[0], d[1], d[2], n(2), n(3), n(4), i[3], f(5), f(6), f(7), n(8), n(9),
                                               i[2], f(10), f(11), f(12));
  if (op == 2 && ni == 1 && nd == 0 && na == 2) return networkmchost_mc_ln(f(0), i[0], f(1)), 0;
  return 4;
}
