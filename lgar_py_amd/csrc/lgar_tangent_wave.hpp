// lgar_tangent_wave.hpp -- the body of a tangent kernel (lgar_tangent_nl.hip, lgar_tangent_forced_nl.hip), included once per kernel
// with LGAR_TANGENT_WINDOW defined: 0 = lgar_tangent_kernel (argument block TArgs, fresh state), 1 = lgar_tangent_window_kernel
// (TWArgs: the TArgs, then the window block that tangent_lane<..., WINDOW = true> starts from and stores to), 2 =
// lgar_tangent_forced_kernel (TFArgs: those two, then the forcing tangents of tangent_lane<..., FORCED = true>).  Text, not a
// function, as lgar_forward_wave.hpp is: through a shared __device__ __forceinline__ wave function every one of the twelve
// kernels came out different (about 36 instructions shorter, two LDS flag loops gone, another register further down), and a
// kernel that changes needs its parity sweeps and timings again.  As text, each kernel is, instruction for instruction, what
// it was when the two families had a translation unit each (compared in the ISA, profiles/r13).
// In scope: R, NL, CAP, MODE.
  __shared__ WaveLDS<Dual<R>, CAP, 1> lds;
  __shared__ R xchg[LGAR_XCHG_WORDS];  // tangent_share: the lanes of a column exchange trapezoid nodes through it (lgar_dual.hpp)
  const int lane = threadIdx.x;
  // the argument block is read in place (kernarg segment), see LGAR_KARG in lgar_scalar.hpp
#if LGAR_TANGENT_WINDOW == 2
  const LGAR_KARG TFArgs<R> *fa = (const LGAR_KARG TFArgs<R> *)__builtin_amdgcn_kernarg_segment_ptr();
  const LGAR_KARG TArgs<R> *ap = &fa->a;
#elif LGAR_TANGENT_WINDOW
  const LGAR_KARG TWArgs<R> *wa = (const LGAR_KARG TWArgs<R> *)__builtin_amdgcn_kernarg_segment_ptr();
  const LGAR_KARG TArgs<R> *ap = &wa->a;
#else
  const LGAR_KARG TArgs<R> *ap = (const LGAR_KARG TArgs<R> *)__builtin_amdgcn_kernarg_segment_ptr();
#endif
  if (ap->pending_in != nullptr && *ap->pending_in == 0u) return;  // no column was handed over to this kernel
  const size_t N = (size_t)ap->N;
  unsigned *ticket = ap->ticket;
  // A block = the columns of one wavefront (columns_per_block).  With a ticket counter: persistent waves, as in the forward
  // kernels.
  const unsigned cpb = columns_per_block(ap->share);
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
    const size_t c = (size_t)blk * cpb + lane;
    // (c < N bounds every access of the lane: the window's state arrays are [rows][N] with rows <= front_slots, read and
    // written at [i * N + c], i < min(n_fronts, front_slots))
#if LGAR_TANGENT_WINDOW == 2
    if ((unsigned)lane < cpb && c < N) tangent_lane<R, NL, CAP, MODE, true, true>(ap, c, lane, lds, &xchg[0], &fa->w, &fa->f);
#elif LGAR_TANGENT_WINDOW
    if ((unsigned)lane < cpb && c < N) tangent_lane<R, NL, CAP, MODE, true>(ap, c, lane, lds, &xchg[0], &wa->w);
#else
    if ((unsigned)lane < cpb && c < N) tangent_lane<R, NL, CAP, MODE>(ap, c, lane, lds, &xchg[0]);
#endif
  }
