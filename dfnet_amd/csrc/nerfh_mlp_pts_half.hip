// nerfh_mlp_pts_half.hip — the points flavour (nerfh_mlp_pts.hip) of kernel variant 6's split-f16 16x16x32 coarse kernel with
// half-height head M-blocks (nerfh_mlp_half.hip): nerfh_coarse_half_pts_kernel and its launcher launch_mlp_pts_half, what
// dfn_mlp_coarse_points runs in split-f16 at netwidth 128.  A translation unit (= a code object) of its own.  Replaces (reference,
// /root/reference/script/): models/nerfw.py:37-46 (the test-time coarse query of run_network_NeRFW: static_sigma alone).
#define DFN_MLP_PTS_TU 1
#define DFN_MLP_FOLD_TU 1
#define DFN_MLP_HALF_TU 1
#include "nerfh_mlp.hip"
