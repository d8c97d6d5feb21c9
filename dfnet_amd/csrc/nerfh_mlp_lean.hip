// nerfh_mlp_lean.hip — kernel variant 12: variant 11's two kernels (split-f16 16x16x32, resident layers, claimed tiles, kept encoding,
// scaled seeds, uniform values formed at their use, one select per head value) with vector work the result does not need taken out of
// the tile seam and the range guard (nerfh_fine_lean_kernel, nerfh_coarse_lean_kernel) and their launcher launch_mlp_lean, as a
// translation unit (= a code object) of their own, in the pattern of nerfh_mlp_sel.hip: the kernels of the other units are compiled,
// laid out and loaded exactly as before.  Three parts, each behind a switch of this file so that it can be built and measured alone
// (-DDFN_LEAN_x=0); the library is built with all three:
//   DFN_LEAN_ACT4   fine: the eight head activations evaluated as four.  Lanes 32..63 carry no sample in the head epilogue, so the
//                   static pre-activations are kept across the transient layers and moved onto those lanes by v_permlane32_swap_b32:
//                   one sigmoid covers a colour pair, one softplus the two densities (nerfh_mlp.hip: the transient branch's end)
//   DFN_LEAN_MAGIC  both: point -> ray by a multiply-high and a shift (nerfh_raydiv.h) instead of a 32-bit division per lane and point
//   DFN_LEAN_MAX3   both: the range guard of the ReLU conversions as one v_pk_maximum3_f16 per two pieces (nerfh_mlp_core.h: X3Piece::C)
// Each computes the same value on the same lane by the same arithmetic: variant 11's outputs and range flag bit for bit, on its packed
// networks, resident blob, scaled table and counters.  (A fourth part, the coarse kernel's rays prefetched by LDS-DMA, was built,
// was bit-exact and measured no gain: LABBOOK R29.1.)
// Replaces (reference, script/): models/rendering.py:269-292 (ray -> points), models/nerfw.py:297-354 (NeRFW.forward: the head
// activations).
#define DFN_MLP_FOLD_TU 1
#define DFN_MLP_HALF_TU 1
#define DFN_MLP_RES_TU 1
#define DFN_MLP_DYN_TU 1
#define DFN_MLP_PE_TU 1
#define DFN_MLP_HOIST_TU 1
#define DFN_MLP_SEL_TU 1
#define DFN_MLP_LEAN_TU 1
#ifndef DFN_LEAN_ACT4
#define DFN_LEAN_ACT4 1
#endif
#ifndef DFN_LEAN_MAGIC
#define DFN_LEAN_MAGIC 1
#endif
#ifndef DFN_LEAN_MAX3
#define DFN_LEAN_MAX3 1
#endif
#include "nerfh_mlp.hip"
