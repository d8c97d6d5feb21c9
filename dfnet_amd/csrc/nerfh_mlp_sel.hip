// nerfh_mlp_sel.hip — kernel variant 11: variant 10's plain fused fine kernel and variant 9's coarse kernel (split-f16 16x16x32,
// resident layers, claimed tiles, kept encoding, scaled seeds, uniform values formed at their use) with ONE SELECT per head value
// (nerfh_fine_sel_kernel, nerfh_coarse_sel_kernel) and their launcher launch_mlp_sel, as a translation unit (= a code object) of
// their own, in the pattern of nerfh_mlp_hoist.hip: the kernels of the other units are compiled, laid out and loaded exactly as before.
// A PrecX3M16 head block leaves value c of the lane's sample in one of two accumulator registers, by lane group (nerfh_mlp_core.h:
// layer()).  LLVM folds the select of two extracted elements into one extract with a lane-dependent index, which on a vector held in
// VGPRs is a chain of 15 v_cmp_eq_u32 and 16 v_cndmask_b32 per index register, with the 15 masks kept in SGPR pairs: about 170 vector
// instructions per fine tile that no MFMA covers, and the scalar pressure that made variant 9 park 79 SGPRs in VGPR lanes (variant 10:
// 39; here none).  Under DFN_MLP_SEL_TU the two candidates go through an opaque copy and the select stays one v_cndmask_b32: the same
// value on the same lane, so the outputs are variant 10's bit for bit.
// Replaces (reference, /root/reference/script/): models/nerfw.py:297-354 (NeRFW.forward: the static_sigma, static_rgb and transient
// head rows as they leave their Linear layers).
#define DFN_MLP_FOLD_TU 1
#define DFN_MLP_HALF_TU 1
#define DFN_MLP_RES_TU 1
#define DFN_MLP_DYN_TU 1
#define DFN_MLP_PE_TU 1
#define DFN_MLP_HOIST_TU 1
#define DFN_MLP_SEL_TU 1
#include "nerfh_mlp.hip"
