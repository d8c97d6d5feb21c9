// nerfh_bwd_coarse_pts.hip — the input-gradient kernel of the COARSE network, points flavour (dfn_mlp_coarse_points_backward):
// nerfh_coarse_backward_pts_kernel is the one-pass kernel of nerfh_bwd.hip reduced to what sigma = softplus(static_sigma(h8)) computes —
// the trunk's forward recompute with its ReLU signs, static_sigma as a head block of its own, the seed d sigma_pre = g sigmoid(pre) spread
// over d h8 by BW_SIG, then BW_L8 .. BW_L1 and the two positional-encoding Jacobians — with its launcher launch_mlp_coarse_backward_pts.
// pts [n_rows, N, 3] and d L / d sigma [n_rows, N] in, d L / d point [n_rows, N, 3] out.  A translation unit (= a code object) of its own:
// the kernels of nerfh_bwd.hip and nerfh_bwd_pts.hip are compiled, laid out and loaded exactly as before.  Replaces (reference):
// autograd through models/nerfw.py:37-46, 315-334 (the test-time coarse query of run_network_NeRFW) into its points.
#define DFN_BWD_PTS_TU 1
#define DFN_BWD_COARSE_TU 1
#include "nerfh_bwd.hip"
