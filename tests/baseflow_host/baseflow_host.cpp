// TEST INFRASTRUCTURE ONLY -- stand-alone host program around baseflow_host.hpp: the two catchment-baseflow entry points and
// gw_exp under the call records of tests/_hostprog.hpp (tests/test_baseflow_host.py; tests/baseflow_host writes the records and
// passes an array of no elements as a null pointer).  Never built or used by the product.
//
// Calls (ints; doubles; arrays, all fp64)
//   0 forward:  T, B; dt_h;  r [T B], par [3 B], state_in [B] or absent, state_out [B], q [T B], s [T B]
//   1 adjoint:  T, B; dt_h;  gq [T B], gs [T B] or absent, r, s [T B], par [3 B], state_in, gr [T B], gpar [3 B], gstate [B]
//   2 gw_exp:   n;  z [n], out [n]
#include "baseflow_host.hpp"

#include "../_hostprog.hpp"

int dispatch(int op, const hostprog::Ints &i, const hostprog::Doubles &d, const hostprog::Arrays &a) {
  const size_t ni = i.size(), nd = d.size(), na = a.size();
  auto f = [&a](int k) { return a[k].as<double>(); };
  if (op == 0 && ni == 2 && nd == 1 && na == 6) return baseflowhost_catchment_baseflow(f(0), i[0], i[1], f(1), d[0], f(2), f(3), f(4), f(5));
  if (op == 1 && ni == 2 && nd == 1 && na == 9)
    return baseflowhost_catchment_baseflow_grad(f(0), f(1), f(2), f(3), i[0], i[1], f(4), d[0], f(5), f(6), f(7), f(8));
  if (op == 2 && ni == 1 && nd == 0 && na == 2) return baseflowhost_gw_exp(f(0), i[0], f(1)), 0;
  return 4;
}
