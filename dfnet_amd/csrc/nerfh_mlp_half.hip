// nerfh_mlp_half.hip — kernel variant 6: variant 5's split-f16 16x16x32 render kernels with half-height head M-blocks
// (nerfh_coarse_half_kernel, nerfh_fine_half_kernel plain and render-maps flavour; nerfh_mlp_core.h: layer<..., HALF>) and their
// launcher launch_mlp_half, as a translation unit (= a code object) of their own, in the pattern of nerfh_mlp_fold.hip: the kernels of
// nerfh_mlp.hip, nerfh_mlp_maps.hip and nerfh_mlp_fold.hip are compiled, laid out and loaded exactly as before.  Replaces (reference,
// /root/reference/script/): models/nerfw.py:297-354 (NeRFW.forward), whose padded head rows the matrix cores need not multiply.
#define DFN_MLP_FOLD_TU 1
#define DFN_MLP_HALF_TU 1
#include "nerfh_mlp.hip"
