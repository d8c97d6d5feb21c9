// nerfh_bwd_coarse_static_pts.hip — the input-gradient kernel of the coarse network's TRAINING query, points flavour
// (dfn_mlp_coarse_static_points_backward): nerfh_coarse_static_backward_pts_kernel is the one-pass kernel of nerfh_bwd.hip without its
// transient branch, on the coarse network's weights — the forward recompute of trunk, xyz_encoding_final + static_sigma, dir_encoding.0
// with the per-row seed and static_rgb with their ReLU signs, the head derivatives g y (1 - y) (rgb) and g sigmoid(pre) (sigma), then
// BW_RGB, BW_DIRCAT, BW_FIN, BW_L8 .. BW_L1 and the two positional-encoding Jacobians — with its launcher
// launch_mlp_coarse_static_backward_pts.  pts [n_rows, N, 3], view directions [n_rows, 3] and d L / d raw4 [n_rows, N, 4] in,
// [d L / d point (3), d L / d viewdir through that point (3)] [n_rows, N, 6] out.  A translation unit (= a code object) of its own: the
// kernels of nerfh_bwd.hip, nerfh_bwd_pts.hip and nerfh_bwd_coarse_pts.hip are compiled, laid out and loaded exactly as before.
// Replaces (reference): autograd through models/nerfw.py:47-60, 326-343 (the training coarse query of run_network_NeRFW) into its
// points and view directions.
#define DFN_BWD_PTS_TU 1
#define DFN_BWD_CSTATIC_TU 1
#include "nerfh_bwd.hip"
