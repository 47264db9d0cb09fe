// TEST INFRASTRUCTURE ONLY -- stand-alone host program around network_pool_host.hpp: the two reach-and-pool network entry points
// and the release law under the call records of tests/_hostprog.hpp (tests/test_network_pool_host.py; tests/network_pool_host
// writes the records and passes an array of no elements as a null pointer).  The topology, pool_ptr and pool_slot are taken as
// the file gives them, so a read or write past an end under a corrupt topology is a finding.  Never built or used by the product.
//
// Calls (ints; doubles; arrays: fp64, the topology int32)
//   0 forward:  T, B, E, n_levels, P; dt_h, rmin, rmax, prmin, prmax;  x [T B], par_mc [4 B], par_pool [5 P], up_ptr [B + 1],
//               up_idx [E], order [B], level_ptr [n_levels + 1], pool_ptr [n_levels], pool_slot [B] (absent without pools),
//               state_in [2 B] or absent, state_out [2 B], y [T B], storage [T P]
//   1 adjoint:  T, B, E, n_levels, P; the same doubles;  gy [T B], par_mc, par_pool, down [B], order, level_ptr, pool_ptr,
//               pool_slot, gx [T B], x, y [T B], storage [T P], up_ptr, up_idx, state_in, gpar_mc [3 B], gpool [4 P], gstate [2 B]
//               (a gpool of no elements is absent and still "wanted": the entry point only asks for the pointer where P > 0)
//   2 release:  n; prmin, prmax;  rc [n], m [n], out [n]
#include "network_pool_host.hpp"

#include "../_hostprog.hpp"

int dispatch(int op, const hostprog::Ints &i, const hostprog::Doubles &d, const hostprog::Arrays &a) {
  const size_t ni = i.size(), nd = d.size(), na = a.size();
  auto f = [&a](int k) { return a[k].as<double>(); };
  auto n = [&a](int k) { return a[k].as<int32_t>(); };
  if (op == 0 && ni == 5 && nd == 5 && na == 13)
    return networkpoolhost_network_route_pool(f(0), i[0], i[1], f(1), f(2), i[4], d[0], d[1], d[2], d[3], d[4], n(3), n(4), i[2], n(5), n(6),
                                              n(7), i[3], n(8), f(9), f(10), f(11), f(12));
  if (op == 1 && ni == 5 && nd == 5 && na == 18)
    return networkpoolhost_network_route_pool_grad(f(0), i[0], i[1], f(1), f(2), i[4], d[0], d[1], d[2], d[3], d[4], n(3), n(4), n(5), n(6),
                                                   i[3], n(7), f(8), f(9), f(10), f(11), n(12), n(13), i[2], f(14), f(15), f(16), f(17));
  if (op == 2 && ni == 1 && nd == 2 && na == 3) return networkpoolhost_release(f(0), f(1), i[0], d[0], d[1], f(2)), 0;
  return 4;
}
