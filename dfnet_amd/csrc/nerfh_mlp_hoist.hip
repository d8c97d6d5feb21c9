// nerfh_mlp_hoist.hip — kernel variant 10: variant 9's plain fused fine kernel (split-f16 16x16x32, resident layers, claimed tiles, kept
// encoding) with two kinds of per-tile work that the result does not need taken out of the tile loop (nerfh_fine_hoist_kernel) and its
// launcher launch_mlp_hoist, as a translation unit (= a code object) of their own, in the pattern of nerfh_mlp_pe.hip: the kernels of
// the other units are compiled, laid out and loaded exactly as before.
//   1. The per-ray seeds arrive at the accumulators' scale.  ray_bias_kernel<true> writes the table of this route multiplied by the
//      fine network's in_scale, once per pass; the RAYBIAS layers (dir_encoding.0 and transient_encoding.0 on h8) seed their
//      accumulators with the loaded values as they are instead of multiplying 2 x 16 loaded registers by in_scale on every tile
//      (nerfh_mlp_core.h: layer()).  The same fp32 product by a power of two on the same values: the bits are unchanged.
//   2. Uniform values are formed where they are used.  As invariants of the tile loop LLVM hoists them into the prologue, where the
//      scalar file cannot hold them all; variant 9's fine kernel parks 79 SGPRs in VGPR lanes and reads them back with 231
//      v_readlane_b32 per tile, on the vector pipe.  Here the weight DMA's per-wave condition and first piece (stage_issue_at: 88 of
//      those reads), the LDS addresses of the input-prefetch slots (wave_here) and the argument pointers used once per tile (args_here:
//      one s_load from the kernarg segment at the use) are no loop invariants: 39 parked SGPRs, 54 + 8 lane reads (the 8 are the
//      compositing's own).  Scalar arithmetic on the same values: the bits are unchanged.
// The unit holds no coarse kernel: the coarse network has no per-ray seeds and parks nothing, and variant 10 runs variant 9's.
// Replaces (reference, /root/reference/script/): models/nerfw.py:297-354 (NeRFW.forward: the dir / appearance / transient columns of
// dir_encoding.0 and transient_encoding.0, constant along a ray).
#define DFN_MLP_FOLD_TU 1
#define DFN_MLP_HALF_TU 1
#define DFN_MLP_RES_TU 1
#define DFN_MLP_DYN_TU 1
#define DFN_MLP_PE_TU 1
#define DFN_MLP_HOIST_TU 1
#include "nerfh_mlp.hip"
