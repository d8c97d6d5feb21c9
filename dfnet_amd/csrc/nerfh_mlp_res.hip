// nerfh_mlp_res.hip — kernel variant 7: variant 6's split-f16 16x16x32 coarse kernel and plain fused fine kernel with a fixed set of
// small layers resident in LDS (nerfh_coarse_res_kernel, nerfh_fine_res_kernel; nerfh_layout.h: kCoarseResident / kFineResident;
// nerfh_mlp_core.h: stage_resident, layer<..., RES>) and their launcher launch_mlp_res, as a translation unit (= a code object) of
// their own, in the pattern of nerfh_mlp_half.hip: the kernels of the other units are compiled, laid out and loaded exactly as before.
// Replaces (reference, /root/reference/script/): models/nerfw.py:297-354 (NeRFW.forward), whose small tail layers need not be fetched
// again for every tile of points.
#define DFN_MLP_FOLD_TU 1
#define DFN_MLP_HALF_TU 1
#define DFN_MLP_RES_TU 1
#include "nerfh_mlp.hip"
