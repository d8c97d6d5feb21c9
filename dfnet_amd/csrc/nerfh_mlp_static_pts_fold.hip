// nerfh_mlp_static_pts_fold.hip — the coarse network's training query (nerfh_mlp_static_pts.hip) in split-f16 at netwidth 128: the
// 16x16x32 kernel of the fine point query (nerfh_mlp_pts_fold.hip: PrecX3M16, xyz_encoding_final folded into dir_encoding.0 at commit,
// static_sigma a head block of its own on h8) cut off behind static_rgb, on the coarse network packed along kCoarseStaticFoldSeq:
// nerfh_coarse_static_fold_pts_kernel and its launcher launch_mlp_static_pts_fold.  A translation unit (= a code object) of its own.
// Replaces (reference, /root/reference/script/): models/nerfw.py:47-60, :326-343.
#define DFN_MLP_PTS_TU 1
#define DFN_MLP_FOLD_TU 1
#define DFN_MLP_STATIC_TU 1
#include "nerfh_mlp.hip"
