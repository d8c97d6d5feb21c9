// nerfh_mlp_pe.hip — kernel variant 9: variant 8's split-f16 16x16x32 coarse kernel and plain fused fine kernel (resident layers in LDS,
// tiles claimed from a device counter) with the 63-wide positional encoding of a tile's points formed ONCE and kept in registers for
// the skip concat in front of layer 5, instead of formed a second time there (nerfh_coarse_pe_kernel, nerfh_fine_pe_kernel;
// nerfh_mlp_core.h: trunk(), kEncodingKept) and their launcher launch_mlp_pe, as a translation unit (= a code object) of their own, in
// the pattern of nerfh_mlp_dyn.hip: the kernels of the other units are compiled, laid out and loaded exactly as before.  The kept
// operand is the value the second evaluation computes from the same inputs with the same code: every output keeps its bits.
// Replaces (reference, /root/reference/script/): models/nerfw.py:105-133 (Embedder.embed), :297-354 (NeRFW.forward: the skip concat
// torch.cat([input_xyz, xyz_], 1) reads the encoding formed once).
#define DFN_MLP_FOLD_TU 1
#define DFN_MLP_HALF_TU 1
#define DFN_MLP_RES_TU 1
#define DFN_MLP_DYN_TU 1
#define DFN_MLP_PE_TU 1
#include "nerfh_mlp.hip"
