// nerfh_mlp_dyn.hip — kernel variant 8: variant 7's split-f16 16x16x32 coarse kernel and plain fused fine kernel (resident layers in LDS)
// with their tiles CLAIMED from a device counter instead of dealt blockIdx.x, + gridDim.x, ... (nerfh_coarse_dyn_kernel,
// nerfh_fine_dyn_kernel; nerfh_mlp_core.h: Stager::claim / next, mid_sync) and their launcher launch_mlp_dyn, as a translation unit
// (= a code object) of their own, in the pattern of nerfh_mlp_res.hip: the kernels of the other units are compiled, laid out and loaded
// exactly as before.  Scheduling only: every tile is computed by the same code on the same inputs and written to the same place.
// Replaces (reference, /root/reference/script/): models/nerfw.py:297-354 (NeRFW.forward), the order in which its chunks of points are
// evaluated.
#define DFN_MLP_FOLD_TU 1
#define DFN_MLP_HALF_TU 1
#define DFN_MLP_RES_TU 1
#define DFN_MLP_DYN_TU 1
#include "nerfh_mlp.hip"
