// nerfh_fused_chain_pts.hip — the training chains of nerfh_fused_chain.hip, POINTS flavour (dfn_nerfh_points_train_forward /
// dfn_nerfh_points_train_backward: one network of NeRF-H evaluated on given points with every layer input kept, and its weight gradients
// from d L / d raw).  train_fwd_chain_pts_kernel<FINE, PL> is train_fwd_chain_kernel reading the point from pts [P, 3] instead of forming
// o + d z; train_bwd_chain_pts_kernel<FINE, PL> is train_bwd_chain_kernel seeded from d L / d raw and the post-activation raw (a point
// query has no compositor to hand it pre-activation gradients): g y (1 - y) on the sigmoid channels, g (1 - e^-y) on the softplus ones,
// zero on padded lanes.  Row index, per-row bias table, stored X / G arrays, sign-bit masks, wave scales and the raw store are the
// step's, so the weight-gradient stream of nerfh_fused_wgrad.hip reads these arrays as it reads the step's.  Launchers:
// launch_points_forward_chain / launch_points_backward_chain (nerfh_fused_train.h).  A translation unit (= a code object) of its own:
// the kernels of nerfh_fused_chain.hip are compiled, laid out and loaded exactly as before.
// Replaces (reference): models/nerfw.py:47-95 (run_network_NeRFW, test_time=False), :297-354 (NeRFW.forward) under autograd with
// respect to the networks' parameters.
#define DFN_CHAIN_PTS_TU 1
#include "nerfh_fused_chain.hip"
