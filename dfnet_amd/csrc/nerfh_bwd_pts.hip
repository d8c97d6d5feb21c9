// nerfh_bwd_pts.hip — the points flavour of the fine network's input-gradient kernel (dfn_mlp_fine_points_backward):
// nerfh_fine_backward_pts_kernel loads the sample positions from pts [n_rows, N, 3] instead of forming o + d z and is otherwise the
// one-pass kernel of nerfh_bwd.hip, with its launcher launch_mlp_fine_backward_pts.  A translation unit (= a code object) of its own: the
// kernels of nerfh_bwd.hip are compiled, laid out and loaded exactly as before.  Replaces (reference, /root/reference/script/): autograd
// through models/nerfw.py:62-95 (the fine query of run_network_NeRFW) into its inputs and view directions.
#define DFN_BWD_PTS_TU 1
#include "nerfh_bwd.hip"
