// TEST INFRASTRUCTURE ONLY -- stand-alone host program around canopy_host.hpp: the three catchment-canopy entry points under the
// call records of tests/_hostprog.hpp (tests/test_canopy_host.py; tests/canopy_host writes the records and passes an array of no
// elements as a null pointer).  Never built or used by the product.
//
// Calls (ints; doubles; arrays, all fp64)
//   0 forward:  T, B; dt_h;  p, e, lai (or absent) [T B], par [3 B], state_in [1 B] or absent, state_out [1 B], w, pet_out, store,
//               evap [T B]
//   1 adjoint:  T, B; dt_h;  gw, gpet, gstore, gevap (each of the last two may be absent), p, e, lai (or absent), store [T B],
//               par [3 B], state_in, gp, ge, glai [T B], gpar [3 B], gstate [1 B]
//   2 tangent:  T, B, D, ld, k0; dt_h;  p, e, lai [T B], par [3 B], state_in [1 B], dp, de, dlai [D T B], dpar [D 3 B],
//               dstate_in [D B] (each of the last five, lai and state_in may be absent), dw, dpet [T B ld], dstore, devap [D T B],
//               dstate_out [D B]
#include "canopy_host.hpp"

#include "../_hostprog.hpp"

int dispatch(int op, const hostprog::Ints &i, const hostprog::Doubles &d, const hostprog::Arrays &a) {
  const size_t ni = i.size(), nd = d.size(), na = a.size();
  auto f = [&a](int k) { return a[k].as<double>(); };
  if (op == 0 && ni == 2 && nd == 1 && na == 10)
    return canopyhost_catchment_canopy(f(0), f(1), f(2), i[0], i[1], f(3), d[0], f(4), f(5), f(6), f(7), f(8), f(9));
  if (op == 1 && ni == 2 && nd == 1 && na == 15)
    return canopyhost_catchment_canopy_grad(f(0), f(1), f(2), f(3), f(4), f(5), f(6), f(7), i[0], i[1], f(8), d[0], f(9), f(10), f(11), f(12),
                                            f(13), f(14));
  if (op == 2 && ni == 5 && nd == 1 && na == 15)
    return canopyhost_catchment_canopy_tangent(f(0), f(1), f(2), i[0], i[1], f(3), d[0], f(4), i[2], f(5), f(6), f(7), f(8), f(9), f(10), f(11),
                                               i[3], i[4], f(12), f(13), f(14));
  return 4;
}
