// nerfh_mlp_pts_fold.hip — the points flavour (nerfh_mlp_pts.hip) of kernel variant 5's split-f16 16x16x32 fine kernel with
// xyz_encoding_final folded at commit (nerfh_mlp_fold.hip): nerfh_fine_fold_pts_kernel and its launcher launch_mlp_pts_fold, the raw
// route of dfn_mlp_fine_points in split-f16 at netwidth 128.  A translation unit (= a code object) of its own.  Replaces (reference,
// /root/reference/script/): models/nerfw.py:62-95 (the fine query of run_network_NeRFW), :297-354 (NeRFW.forward).
#define DFN_MLP_PTS_TU 1
#define DFN_MLP_FOLD_TU 1
#include "nerfh_mlp.hip"
