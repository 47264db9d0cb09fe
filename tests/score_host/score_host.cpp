// TEST INFRASTRUCTURE ONLY -- stand-alone host program around score_host.hpp: the two catchment-score entry points under the
// call records of tests/_hostprog.hpp (tests/test_score_host.py; tests/score_host writes the records and passes an array of no
// elements as a null pointer).  The workspace of the moments is allocated here, at exactly the size the library states, so a
// write past its end is a finding too.  Never built or used by the product.
//
// Calls (ints; arrays, all fp64)
//   0 moments:   To, B, window;  sim [To * window * B], obs [To * B], moments [7 * B]
//   1 gradient:  To, B, window;  sim, obs, moments [7 * B], coef [4 * B], grad_sim [To * window * B]
#include "score_host.hpp"

#include "../_hostprog.hpp"

int dispatch(int op, const hostprog::Ints &i, const hostprog::Doubles &d, const hostprog::Arrays &a) {
  const size_t ni = i.size(), na = a.size();
  auto f = [&a](int k) { return a[k].as<double>(); };
  if (ni != 3 || d.size() != 0 || i[2] < 1) return 4;
  if (op == 0 && na == 3) {
    hostprog::Array ws;
    const int64_t bytes = scorehost_catchment_moments_workspace(i[0], i[1]);
    if (bytes < 0) return 4;
    if (bytes > 0) ws.blank((size_t)bytes);
    return scorehost_catchment_moments(f(0), f(1), i[0], i[1], i[2], f(2), ws.as<double>());
  }
  if (op == 1 && na == 5) return scorehost_catchment_moments_grad(f(0), f(1), i[0], i[1], i[2], f(2), f(3), f(4));
  return 4;
}
