// TEST INFRASTRUCTURE ONLY -- stand-alone host program around post_host.hpp: the six post-processing entry points under the
// call records of tests/_hostprog.hpp (tests/test_moisture_host.py, test_catchment_host.py, test_route_host.py hold the SAME source
// the GPU executes against the reference's own data and the numpy statements of the definitions; tests/post_host writes the
// records).  Never built or used by the product.
#include "post_host.hpp"

#include "../_hostprog.hpp"

// the operation's scalars (s) and arrays (a), in the order of its argument list; 4 = not a call this program knows
int dispatch(int op, const hostprog::Ints &s, const hostprog::Doubles &f, const hostprog::Arrays &a) {
  const size_t ns = s.size(), na = a.size();
  if (f.size()) return 4;  // (no call here takes fp64 scalars)
  LgarDims d;
  memset(&d, 0, sizeof d);
  if (op == 0 && ns == 6 && na == 7 && s[2] >= 1) {  // dtype, n_layers, front_slots, n_columns, n_bins, what
    LgarParams p;
    LgarState st;
    memset(&p, 0, sizeof p);
    memset(&st, 0, sizeof st);
    d.n_layers = s[1], d.front_slots = s[2], d.n_columns = s[3];
    p.thickness = a[0].as<void>();
    st.depth = a[1].as<void>(), st.theta = a[2].as<void>(), st.flags = a[3].as<uint8_t>(), st.n_fronts = a[4].as<int32_t>();
    return posthost_soil_moisture(&d, &p, &st, a[5].as<double>(), s[4], s[5], a[6].as<void>(), s[0]);
  }
  if (op == 1 && ns == 3 && na == 8) {  // dtype, n_columns, n_rows; the seven summed series, running
    LgarStepOut so;
    memset(&so, 0, sizeof so);
    for (int j = 0; j < 7; j++) so.series[j] = a[j].as<void>();
    d.n_columns = s[1];
    return posthost_totals_replay(&d, &so, s[2], a[7].as<void>(), s[0]);
  }
  if (op == 2 && ns == 6 && na == 7)  // dtype, n_rows, n_columns, n_catchments, n_order, rows_per_wave
    return posthost_catchment_sums(a[0].as<void>(), s[1], s[2], a[1].as<int32_t>(), s[3], a[2].as<int32_t>(), s[4], a[3].as<void>(),
                                   a[4].as<int32_t>(), a[5].as<double>(), a[6].as<double>(), s[0], s[5]);
  if (op == 3 && ns == 4 && na == 5)  // dtype, n_rows, n_catchments, n_columns
    return posthost_catchment_spread(a[0].as<double>(), s[1], s[2], a[1].as<int32_t>(), s[3], a[2].as<void>(), a[3].as<int32_t>(),
                                     a[4].as<void>(), s[0]);
  if (op == 4 && ns == 5 && na == 5)  // n_rows, n_catchments, n_ordinates, per_catchment, reverse
    return posthost_catchment_route(a[0].as<double>(), s[0], s[1], a[1].as<double>(), s[2], s[3], a[2].as<double>(), a[3].as<double>(),
                                    a[4].as<double>(), s[4]);
  if (op == 5 && ns == 3 && na == 3)  // n_rows, n_catchments, n_ordinates
    return posthost_catchment_route_grad(a[0].as<double>(), a[1].as<double>(), s[0], s[1], s[2], a[2].as<double>());
  return 4;
}
