// nerfh_mlp_maps.hip — the render-maps flavour of the fused fine kernels (nerfh_fine_kernel<..., MAPS = true>) and its launcher
// launch_mlp_maps, as a translation unit (= a code object) of their own: the kernels of nerfh_mlp.hip that run when no map is asked
// for are compiled, laid out and loaded exactly as before.  Replaces (reference, /root/reference/script/): the quantities of
// models/rendering.py:196-241 that raw2outputs_NeRFW forms and render() drops at test time.
#define DFN_MLP_MAPS_TU 1
#include "nerfh_mlp.hip"
