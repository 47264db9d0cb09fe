// lgar_forward_wave.hpp -- the body of a forward kernel (lgar_kernels_nl.hip), included once per kernel with
// LGAR_FORWARD_MAPPED defined: 0 = the forcing column comes from the layout, 1 = from LgarForcing.column_map (forward_lane's
// MAPPED).  Text, not a function: the kernel without a map has to stay, instruction for instruction, the kernel it was before
// the map existed, and these kernels' register allocation changes with one more level of inlining (compared in the ISA).
// In scope: R, NL, CAP, MODE, and the wave's `lds` and `coop_lds`.
  const int lane = threadIdx.x;
  // the argument block is read in place (kernarg segment), see LGAR_KARG in lgar_scalar.hpp
  const LGAR_KARG KArgs<R> *ap = (const LGAR_KARG KArgs<R> *)__builtin_amdgcn_kernarg_segment_ptr();
  const size_t N = (size_t)ap->N;
  unsigned *ticket = ap->ticket;
  if (ap->pending_in != nullptr && *ap->pending_in == 0u) return;  // no column was handed over to this kernel
  // With a ticket counter: persistent waves.  The grid is one wave per wave slot of the chip; each pulls 64-column blocks
  // from the counter until none is left, so no round of the grid is partially filled whatever the column count.
  // Without: one workgroup per block.
  // cooperating lanes: `coop` adjacent lanes per column (4..64; 1 = every lane its own column), 64 / coop columns per wave
  const int coop = CoopLDS<R, MODE>::on ? ap->coop : 1;
  const unsigned cpb = (unsigned)(WAVE / coop);
  const unsigned nblocks = (unsigned)((N + cpb - 1) / cpb);
  for (bool first = true;; first = false) {
    unsigned blk = blockIdx.x;
    if (ticket != nullptr) {
      if (lane == 0) blk = atomicAdd(ticket, 1u);
      blk = __builtin_amdgcn_readfirstlane(blk);
      if (blk >= nblocks) break;
    } else if (!first) {
      break;
    }
    if constexpr (CoopLDS<R, MODE>::on) {
      if (coop > 1) {
        // my group and my place in it; the lanes left over when coop does not divide 64 join the last group
        int group = lane / coop;
        group = group < (int)cpb ? group : (int)cpb - 1;
        const int rank = lane - group * coop;
        const size_t c0 = (size_t)blk * cpb + group;
        const bool live = c0 < N;
        // (a wave of at most 8 columns leaves every group two rows of the exchange table: Column::calc_dzdt_pairs)
        const int rows = (cpb <= LGAR_COOP_GROUPS / 2) ? 2 : 1;
        forward_lane<R, NL, CAP, MODE, LGAR_FORWARD_MAPPED>(ap, live ? c0 : N - 1, live, lane, lds, rank == 0, &coop_lds.tab[group * rows][0], group, rank);
        continue;
      }
    }
    const size_t c0 = (size_t)blk * WAVE + lane;
    const bool live = c0 < N;
    forward_lane<R, NL, CAP, MODE, LGAR_FORWARD_MAPPED>(ap, live ? c0 : N - 1, live, lane, lds);
  }
