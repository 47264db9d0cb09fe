// TEST INFRASTRUCTURE ONLY -- stand-alone host program around snow_host.hpp: the two catchment-snowpack entry points under the
// call records of tests/_hostprog.hpp (tests/test_snow_host.py; tests/snow_host writes the records and passes an array of no
// elements as a null pointer).  Never built or used by the product.
//
// Calls (ints; doubles; arrays, all fp64)
//   0 forward:  T, B; dt_h;  p, ta [T B], par [7 B], state_in [2 B] or absent, state_out [2 B], w, ice, liq [T B]
//   1 adjoint:  T, B; dt_h;  gw, gice, gliq (the two absent together), p, ta, ice, liq [T B], par [7 B], state_in, gp, gta [T B],
//               gpar [7 B], gstate [2 B]
#include "snow_host.hpp"

#include "../_hostprog.hpp"

int dispatch(int op, const hostprog::Ints &i, const hostprog::Doubles &d, const hostprog::Arrays &a) {
  const size_t ni = i.size(), nd = d.size(), na = a.size();
  auto f = [&a](int k) { return a[k].as<double>(); };
  if (op == 0 && ni == 2 && nd == 1 && na == 8) return snowhost_catchment_snow(f(0), f(1), i[0], i[1], f(2), d[0], f(3), f(4), f(5), f(6), f(7));
  if (op == 1 && ni == 2 && nd == 1 && na == 13)
    return snowhost_catchment_snow_grad(f(0), f(1), f(2), f(3), f(4), f(5), f(6), i[0], i[1], f(7), d[0], f(8), f(9), f(10), f(11), f(12));
  return 4;
}
