// TEST INFRASTRUCTURE ONLY -- stand-alone host program around network_pool_host.hpp.
//
// Reads calls of the two reach-and-pool network entry points (and of the release law) from a binary file, runs each through its
// host-side launcher and writes the output arrays, so tests/test_network_pool_host.py can hold the SAME source the GPU executes
// against the numpy statement of the definition -- also in an AddressSanitizer + UBSan build, which needs nothing loaded into
// python.  Every array is allocated at exactly its stated size (an array of no elements is a null pointer), and the topology,
// pool_ptr and pool_slot are taken as the file gives them, so a read or write past an end under a corrupt topology is a finding.
// Never built or used by the product.
//
// File format (native endianness).  Input: int32 n_calls, then per call ten int32
//   operation (0 forward, 1 adjoint, 2 release law), T, B, E, n_levels, P, has_state_in, wants (forward: 1 = state_out,
//   2 = storage; adjoint: 1 = gpar_mc, 2 = gpool, 4 = gstate), 0, 0
// then fp64 dt_h, rmin, rmax, prmin, prmax and
//   forward:  par_mc [4 B], par_pool [5 P], x [T B], state_in [2 B] if has_state_in, up_ptr [B + 1], up_idx [E], order [B],
//             level_ptr [n_levels + 1], pool_ptr [n_levels], pool_slot [B] if P > 0
//   adjoint:  par_mc [4 B], par_pool [5 P], gy [T B], x [T B], y [T B], storage [T P], state_in [2 B] if has_state_in, down [B],
//             order [B], level_ptr [n_levels + 1], pool_ptr [n_levels], pool_slot [B] if P > 0, up_ptr [B + 1], up_idx [E]
//   release:  rc [T], m [T]
// Output: per call y [T B] (+ state_out [2 B]) (+ storage [T P]), or gx [T B] (+ gpar_mc [3 B]) (+ gpool [4 P]) (+ gstate [2 B]), or
// the release [T].  An output starts as all-ones bytes (NaN): it is written, not added to.  A refused call ends the program with
// status 4.
#include <cstdio>
#include <cstring>
#include <memory>

#include "network_pool_host.hpp"

namespace {

template <typename V> struct Array {
  std::unique_ptr<V[]> mem;
  size_t n = 0;
  V *get() const { return n ? mem.get() : nullptr; }
  void size(size_t count) {
    n = count;
    if (n) mem.reset(new V[n]);
  }
  bool read(FILE *in, size_t count) {
    size(count);
    return n == 0 || fread(mem.get(), sizeof(V), n, in) == n;
  }
  void blank(size_t count) {
    size(count);
    if (n) memset(mem.get(), 0xFF, n * sizeof(V));
  }
  bool write(FILE *out) const { return n == 0 || fwrite(mem.get(), sizeof(V), n, out) == n; }
};

int run_call(FILE *in, FILE *out) {
  int32_t h[10];
  double sc[5];
  if (fread(h, 4, 10, in) != 10 || h[1] < 0 || h[2] < 0 || h[3] < 0 || h[4] < 0 || h[5] < 0 || fread(sc, 8, 5, in) != 5) return 2;
  const int32_t op = h[0], T = h[1], B = h[2], E = h[3], L = h[4], P = h[5];
  const bool has_state = h[6] != 0;
  const int32_t wants = h[7];
  const size_t TB = (size_t)T * (size_t)B, TP = (size_t)T * (size_t)P;
  Array<double> par_mc, par_pool, x, y, gy, storage, state_in, result, extra, extra2, extra3;
  Array<int32_t> up_ptr, up_idx, order, level_ptr, pool_ptr, pool_slot, down;
  if (op == 2) {
    if (!x.read(in, T) || !y.read(in, T)) return 2;
    result.blank(T);
    networkpoolhost_release(x.get(), y.get(), T, sc[3], sc[4], result.get());
    return result.write(out) ? 0 : 3;
  }
  if (!par_mc.read(in, 4 * (size_t)B) || !par_pool.read(in, 5 * (size_t)P)) return 2;
  if (op == 0) {
    if (!x.read(in, TB) || (has_state && !state_in.read(in, 2 * (size_t)B)) || !up_ptr.read(in, (size_t)B + 1) || !up_idx.read(in, E) ||
        !order.read(in, B) || !level_ptr.read(in, (size_t)L + 1) || !pool_ptr.read(in, L) || !pool_slot.read(in, P > 0 ? B : 0))
      return 2;
    result.blank(TB);
    if (wants & 1) extra.blank(2 * (size_t)B);
    if (wants & 2) extra2.blank(TP);
    if (networkpoolhost_network_route_pool(x.get(), T, B, par_mc.get(), par_pool.get(), P, sc[0], sc[1], sc[2], sc[3], sc[4], up_ptr.get(),
                                           up_idx.get(), E, order.get(), level_ptr.get(), pool_ptr.get(), L, pool_slot.get(), state_in.get(),
                                           extra.get(), result.get(), extra2.get()) != 0)
      return 4;
  } else if (op == 1) {
    if (!gy.read(in, TB) || !x.read(in, TB) || !y.read(in, TB) || !storage.read(in, TP) || (has_state && !state_in.read(in, 2 * (size_t)B)) ||
        !down.read(in, B) || !order.read(in, B) || !level_ptr.read(in, (size_t)L + 1) || !pool_ptr.read(in, L) ||
        !pool_slot.read(in, P > 0 ? B : 0) || !up_ptr.read(in, (size_t)B + 1) || !up_idx.read(in, E))
      return 2;
    result.blank(TB);
    if (wants & 1) extra.blank(3 * (size_t)B);
    if (wants & 2) extra2.blank(4 * (size_t)P);
    if (wants & 4) extra3.blank(2 * (size_t)B);
    // (a gpool of no elements is still "wanted": the entry point only asks whether the pointer is null where P > 0)
    if (networkpoolhost_network_route_pool_grad(gy.get(), T, B, par_mc.get(), par_pool.get(), P, sc[0], sc[1], sc[2], sc[3], sc[4], down.get(),
                                                order.get(), level_ptr.get(), pool_ptr.get(), L, pool_slot.get(), result.get(), x.get(),
                                                y.get(), storage.get(), up_ptr.get(), up_idx.get(), E, state_in.get(), extra.get(),
                                                extra2.get(), extra3.get()) != 0)
      return 4;
  } else {
    return 4;
  }
  return result.write(out) && extra.write(out) && extra2.write(out) && extra3.write(out) ? 0 : 3;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s <input> <output>\n", argv[0]);
    return 1;
  }
  FILE *in = fopen(argv[1], "rb");
  FILE *out = fopen(argv[2], "wb");
  if (!in || !out) return 1;
  int32_t n_calls = 0;
  if (fread(&n_calls, 4, 1, in) != 1) return 2;
  for (int k = 0; k < n_calls; k++) {
    const int rc = run_call(in, out);
    if (rc) return rc;
  }
  fclose(in);
  return fclose(out) == 0 ? 0 : 3;
}
