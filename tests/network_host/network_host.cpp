// TEST INFRASTRUCTURE ONLY -- stand-alone host program around network_host.hpp: the two catchment-network entry points under the
// call records of tests/_hostprog.hpp (tests/test_network_host.py; tests/network_host writes the records and passes an array of
// no elements as a null pointer).  The topology is taken as the file gives it, so a read or write past an end under a corrupt
// topology is a finding.  Never built or used by the product.
//
// Calls (ints; arrays: fp64, the topology int32)
//   0 forward:  T, B, E, n_levels;  x [T B], coef [3 B], up_ptr [B + 1], up_idx [E], order [B], level_ptr [n_levels + 1],
//               state_in [2 B] or absent, state_out [2 B], y [T B]
//   1 adjoint:  T, B, E, n_levels;  gy [T B], coef, down [B], order, level_ptr, gx [T B] and, absent without the coefficient
//               gradient, x, y [T B], up_ptr, up_idx, state_in, gc [3 B]
#include "network_host.hpp"

#include "../_hostprog.hpp"

int dispatch(int op, const hostprog::Ints &i, const hostprog::Doubles &d, const hostprog::Arrays &a) {
  const size_t na = a.size();
  auto f = [&a](int k) { return a[k].as<double>(); };
  auto n = [&a](int k) { return a[k].as<int32_t>(); };
  if (i.size() != 4 || d.size() != 0) return 4;
  if (op == 0 && na == 9) return networkhost_network_route(f(0), i[0], i[1], f(1), n(2), n(3), i[2], n(4), n(5), i[3], f(6), f(7), f(8));
  if (op == 1 && na == 12)
    return networkhost_network_route_grad(f(0), i[0], i[1], f(1), n(2), n(3), n(4), i[3], f(5), f(6), f(7), n(8), n(9), i[2], f(10), f(11));
  return 4;
}
