// nerfh_mlp_static_pts.hip — the coarse network's TRAINING query on the caller's points (dfn_mlp_coarse_static_points): the points
// flavour of the fine kernel (nerfh_mlp_pts.hip) cut off behind static_rgb, evaluated on the coarse network's weights packed along
// kCoarseStaticSeq: trunk, xyz_encoding_final + static_sigma, dir_encoding.0 with a per-row seed, static_rgb; 4 floats per point
// (nerfh_coarse_static_pts_kernel, launch_mlp_static_pts).  A translation unit (= a code object) of its own: the kernels of the other
// units are compiled, laid out and loaded exactly as before.  This unit holds f16 and exact fp32 at netwidth 128 and the three
// arithmetic modes at netwidth 256; split-f16 at netwidth 128 is nerfh_mlp_static_pts_fold.hip.  Replaces (reference,
// /root/reference/script/): models/nerfw.py:47-60 (the training coarse query of run_network_NeRFW), :326-343 (NeRFW.forward, output_transient=False).
#define DFN_MLP_PTS_TU 1
#define DFN_MLP_STATIC_TU 1
#include "nerfh_mlp.hip"
