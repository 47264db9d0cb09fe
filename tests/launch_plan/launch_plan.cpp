// TEST INFRASTRUCTURE ONLY -- stand-alone host program around lgar_py_amd/csrc/lgar_plan.hpp.
//
// What a lgar_forward / lgar_forward_tangent call launches is decided by plain host C++ (forward_plan, tangent_plan, chain_step)
// that the library and the device-code simulator share; with -DLGAR_DEVSIM the header compiles without HIP.  This program prints
// the plans of the cases handed to it, so tests/test_launch_plan.py can pin them -- also in an AddressSanitizer + UBSan build,
// which needs nothing loaded into python.  Never built or used by the product.
//
// One case per argument, comma-separated integers after the kind:
//   f,<fp64>,<n_columns>,<n_layers>,<num_subcycles>,<nint>,<front_slots>,<search_mode>,<geff_mode>,<use_closed_form_G>,<forward_lanes>,<simds>
//   t,<n_columns>,<n_layers>,<num_subcycles>,<front_slots>,<search_mode>,<tangent_share>
// One JSON object per case and line.  "steps": per kernel of the chain [chain_first, chain_last, pending_in, pending_out, work
// counter], the pointers as indices into the tickets array (-1: null).
#define LGAR_DEVSIM 1
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#define __device__
#define __host__
#define __global__
#define __forceinline__ inline __attribute__((always_inline))

#include "../../lgar_py_amd/csrc/lgar_plan.hpp"

using namespace lgar;

namespace {

void print_chain(const int *caps, int n) {
  unsigned tickets[LGAR_NTICKETS] = {0};
  auto at = [&](const unsigned *p) { return p ? (int)(p - tickets) : -1; };
  printf("\"caps\": [");
  for (int i = 0; i < n; i++) printf("%s%d", i ? ", " : "", caps[i]);
  printf("], \"steps\": [");
  KArgs<float> a = KArgs<float>();
  for (int i = 0; i < n; i++) {
    const unsigned *tk = chain_step(a, i, n, tickets);
    printf("%s[%d, %d, %d, %d, %d]", i ? ", " : "", a.chain_first, a.chain_last, at(a.pending_in), at(a.pending_out), at(tk));
  }
  printf("]}\n");
}

}  // namespace

int main(int argc, char **argv) {
  for (int k = 1; k < argc; k++) {
    long v[16] = {0};
    int nv = 0;
    char kind = argv[k][0];
    for (const char *s = strchr(argv[k], ','); s && nv < 16; s = strchr(s + 1, ',')) v[nv++] = strtol(s + 1, nullptr, 10);
    LgarDims d;
    memset(&d, 0, sizeof d);
    d.dt_h = 1.0;
    if (kind == 'f' && nv == 11) {
      d.n_columns = (int32_t)v[1]; d.n_layers = (int32_t)v[2]; d.num_subcycles = (int32_t)v[3]; d.nint = (int32_t)v[4];
      d.front_slots = (int32_t)v[5]; d.search_mode = (int32_t)v[6]; d.geff_mode = (int32_t)v[7];
      d.use_closed_form_G = (int32_t)v[8]; d.forward_lanes = (int32_t)v[9];
      if (check_dims(&d) != 0) return 4;
      const ForwardPlan p = v[0] ? forward_plan<double>(&d, d.n_layers, (unsigned)v[10]) : forward_plan<float>(&d, d.n_layers, (unsigned)v[10]);
      printf("{\"literal\": %d, \"mixed\": %d, \"coop\": %d, ", (int)p.literal, (int)p.mixed, p.coop);
      print_chain(p.caps, p.n);
    } else if (kind == 't' && nv == 6) {
      d.n_columns = (int32_t)v[0]; d.n_layers = (int32_t)v[1]; d.num_subcycles = (int32_t)v[2]; d.nint = 120;
      d.front_slots = (int32_t)v[3]; d.search_mode = (int32_t)v[4]; d.tangent_share = (int32_t)v[5];
      if (check_dims(&d) != 0) return 4;
      const TangentPlan p = tangent_plan(&d, d.n_layers);
      printf("{\"literal\": %d, \"columns_per_block\": %u, ", (int)p.literal, p.columns_per_block);
      print_chain(p.caps, p.n);
    } else {
      fprintf(stderr, "bad case: %s\n", argv[k]);
      return 1;
    }
  }
  return 0;
}
