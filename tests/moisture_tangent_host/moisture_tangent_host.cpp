// TEST INFRASTRUCTURE ONLY -- stand-alone host program around moisture_tangent_host.hpp: lgar_soil_moisture_tangent under the call
// records of tests/_hostprog.hpp (tests/test_moisture_tangent_host.py; tests/moisture_tangent_host writes the records and passes an
// array of no elements as a null pointer).  Never built or used by the product.
//
// Call 0 (ints; arrays):  dtype, L, F, M, n_bins, what, group;
//   thickness [L M], depth, theta [F M] (dtype), flags uint8 [F M], n_fronts int32 [M], ddepth, dtheta [F M] (dtype),
//   edges fp64 [n_bins + 1] or absent, out [n_bins M] (dtype) or absent, cot fp64 [n_bins M / group] or absent, grad [M] (dtype,
//   input and output) or absent
#include "moisture_tangent_host.hpp"

#include <cstring>

#include "../_hostprog.hpp"

int dispatch(int op, const hostprog::Ints &i, const hostprog::Doubles &d, const hostprog::Arrays &a) {
  if (op != 0 || i.size() != 7 || d.size() != 0 || a.size() != 11) return 4;
  LgarDims dims;
  std::memset(&dims, 0, sizeof(dims));
  dims.n_layers = i[1], dims.front_slots = i[2], dims.n_columns = i[3];
  LgarParams p;
  std::memset(&p, 0, sizeof(p));
  p.thickness = a[0].as<void>();
  LgarState s, ds;
  std::memset(&s, 0, sizeof(s));
  std::memset(&ds, 0, sizeof(ds));
  s.depth = a[1].as<void>(), s.theta = a[2].as<void>(), s.flags = a[3].as<uint8_t>(), s.n_fronts = a[4].as<int32_t>();
  ds.depth = a[5].as<void>(), ds.theta = a[6].as<void>();
  return mthost_soil_moisture_tangent(&dims, &p, &s, &ds, a[7].as<double>(), i[4], i[5], a[8].as<void>(), a[9].as<double>(), i[6],
                                      a[10].as<void>(), i[0]);
}
