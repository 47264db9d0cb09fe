// TEST INFRASTRUCTURE ONLY -- stand-alone host program around snow_tangent_host.hpp under the call records of tests/_hostprog.hpp
// (tests/test_snow_tangent_host.py; an array of no elements is a null pointer).  Never built or used by the product.
//
// Call 0 (ints; doubles; arrays, all fp64):  T, B, D, ld, k0; dt_h;  p, ta [T B], par [7 B], state_in [2 B], dp, dta [D T B],
//   dpar [D 7 B], dstate_in [D 2 B] (each of the last five may be absent), dw [T B ld], dice, dliq [D T B], dstate_out [D 2 B]
#include "snow_tangent_host.hpp"

#include "../_hostprog.hpp"

int dispatch(int op, const hostprog::Ints &i, const hostprog::Doubles &d, const hostprog::Arrays &a) {
  auto f = [&a](int k) { return a[k].as<double>(); };
  if (op == 0 && i.size() == 5 && d.size() == 1 && a.size() == 12)
    return snowtanhost_catchment_snow_tangent(f(0), f(1), i[0], i[1], f(2), d[0], f(3), i[2], f(4), f(5), f(6), f(7), f(8), i[3], i[4], f(9),
                                              f(10), f(11));
  return 4;
}
