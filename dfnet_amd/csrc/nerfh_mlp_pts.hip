// nerfh_mlp_pts.hip — the points flavour of the NeRF-H network kernels (dfn_mlp_coarse_points, dfn_mlp_fine_points): the MLP inputs are
// loaded from pts [n_rows, N, 3] instead of being formed as o + d z (nerfh_coarse_pts_kernel, nerfh_fine_pts_kernel) and the fine
// kernel's next-tile prefetch fetches pts by LDS-DMA; everything behind the inputs is the code of nerfh_mlp.hip.  A translation unit
// (= a code object) of its own with its launcher launch_mlp_pts, in the pattern of nerfh_mlp_maps.hip: the kernels of the other units
// are compiled, laid out and loaded exactly as before.  This unit holds f16 and exact fp32 at netwidth 128 and the three arithmetic
// modes at netwidth 256; split-f16 at netwidth 128 is nerfh_mlp_pts_half.hip (coarse) and nerfh_mlp_pts_fold.hip (fine).  Replaces
// (reference, /root/reference/script/): models/nerfw.py:15-95 (run_network_NeRFW on pre-sampled points), :425-434 (network_query_fn).
#define DFN_MLP_PTS_TU 1
#include "nerfh_mlp.hip"
