// nerfh_mlp_fold.hip — kernel variant 5: the split-f16 16x16x32 fine render kernel with xyz_encoding_final folded into the two layers
// it feeds (nerfh_fine_fold_kernel, plain and render-maps flavour) and its launcher launch_mlp_fold, as a translation unit (= a code
// object) of their own, in the pattern of nerfh_mlp_maps.hip: the kernels of nerfh_mlp.hip and nerfh_mlp_maps.hip are compiled, laid
// out and loaded exactly as before.  Replaces (reference, /root/reference/script/): models/nerfw.py:297-354 (NeRFW.forward), whose
// xyz_encoding_final output the folded weights of dfn_nerfh_commit make unnecessary at test time.
#define DFN_MLP_FOLD_TU 1
#include "nerfh_mlp.hip"
