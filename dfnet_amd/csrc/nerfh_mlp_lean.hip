// nerfh_mlp_lean.hip — kernel variant 12, the lean unit: variant 7's split-f16 16x16x32 coarse kernel and plain fused fine kernel
// (resident layers in LDS, nerfh_mlp_res.hip) with per-tile work that the result does not need taken out (nerfh_fine_lean_kernel,
// nerfh_coarse_lean_kernel) and their launcher launch_mlp_lean, as a translation unit (= a code object) of their own, in the pattern of
// nerfh_mlp_res.hip: the kernels of the other units are compiled, laid out and loaded exactly as before.  One flag, DFN_MLP_LEAN_TU,
// turns on all of the following (nerfh_layout.h "Kernel variants" has a paragraph on each; variants 8 to 11 were the steps by which
// they were added one at a time, each measured against the one before, and are retired):
//   claimed tiles    both: a workgroup takes its next tile from a device counter instead of blockIdx.x, + gridDim.x, ...
//                    (nerfh_mlp_core.h: Stager::claim / next, mid_sync).  Scheduling only: every tile is computed by the same code on
//                    the same inputs and written to the same place
//   kept encoding    both: the 63-wide positional encoding of a tile's points is formed ONCE and kept in registers for the skip concat
//                    in front of layer 5, instead of formed a second time there (nerfh_mlp_core.h: trunk(), kEncodingKept).  The kept
//                    operand is the value the second evaluation computes from the same inputs with the same code
//   scaled seeds     fine: ray_bias_kernel<true> writes the per-ray table of this route multiplied by the fine network's in_scale, once
//                    per pass; the RAYBIAS layers (dir_encoding.0 and transient_encoding.0 on h8) seed their accumulators with the
//                    loaded values as they are instead of multiplying 2 x 16 loaded registers by in_scale on every tile
//                    (nerfh_mlp_core.h: layer()).  The same fp32 product by a power of two on the same values
//   uniform values   fine: formed where they are used.  As invariants of the tile loop LLVM hoists them into the prologue, where the
//                    scalar file cannot hold them all; without this the fine kernel parks 79 SGPRs in VGPR lanes and reads them back
//                    with 231 v_readlane_b32 per tile, on the vector pipe.  The weight DMA's per-wave condition and first piece
//                    (stage_issue_at: 88 of those reads), the LDS addresses of the input-prefetch slots (wave_here) and the argument
//                    pointers used once per tile (args_here: one s_load from the kernarg segment at the use) are no loop invariants
//                    here.  Scalar arithmetic on the same values
//   one select       both: a PrecX3M16 head block leaves value c of the lane's sample in one of two accumulator registers, by lane
//                    group (nerfh_mlp_core.h: layer()).  LLVM folds the select of two extracted elements into one extract with a
//                    lane-dependent index, which on a vector held in VGPRs is a chain of 15 v_cmp_eq_u32 and 16 v_cndmask_b32 per
//                    index register, with the 15 masks kept in SGPR pairs: about 170 vector instructions per fine tile that no MFMA
//                    covers, and the scalar pressure behind the parked SGPRs above (with this: none).  The two candidates go through an
//                    opaque copy and the select stays one v_cndmask_b32: the same value on the same lane
//   packed heads     fine: the eight head activations evaluated as four.  Lanes 32..63 carry no sample in the head epilogue, so the
//                    static pre-activations are kept across the transient layers and moved onto those lanes by v_permlane32_swap_b32:
//                    one sigmoid covers a colour pair, one softplus the two densities (nerfh_mlp.hip: the transient branch's end)
//   magic division   both: point -> ray by a multiply-high and a shift (nerfh_raydiv.h) instead of a 32-bit division per lane and point
//   maximum3 guard   both: the range guard of the ReLU conversions as one v_pk_maximum3_f16 per two pieces (nerfh_mlp_core.h: X3Piece::C)
// Each computes the same value on the same lane by the same arithmetic: variant 7's outputs and range flag bit for bit, on its packed
// networks and resident blob.  (One more part, the coarse kernel's rays prefetched by LDS-DMA, was built, was bit-exact and measured
// no gain: LABBOOK R29.1.)
// Replaces (reference, script/): models/rendering.py:269-292 (ray -> points), models/nerfw.py:105-133 (Embedder.embed), :297-354
// (NeRFW.forward: the skip concat, the dir / appearance / transient columns constant along a ray, the head rows and activations, the
// order in which its chunks of points are evaluated).
#define DFN_MLP_FOLD_TU 1
#define DFN_MLP_HALF_TU 1
#define DFN_MLP_RES_TU 1
#define DFN_MLP_LEAN_TU 1
#include "nerfh_mlp.hip"
