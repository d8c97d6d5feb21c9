// nerfh_handle.h — the NeRF-H handle behind dfn_nerfh_t, shared by nerfh_pack.hip (its life and the host packer behind
// dfn_nerfh_commit), nerfh_api.hip (test-time render path) and nerfh_train_api.hip (training path, generic-width path).
#pragma once
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../include/dfnet_hip.h"
#include "nerfh_kernels.h"
#include "nerfh_layout.h"

struct PackedNet {
  char* blob = nullptr;
  uint32_t* tab = nullptr;
  int n_units = 0;
  int n_fwd_units = 0;   // gradient nets: the forward units come first in the table
  float in_scale = 1.f;  // split-f16: weight scale x activation scale carried by the accumulators
  char* res_blob = nullptr;   // kernel variant 7: the LDS-resident layers (blob / tab then hold the streamed units only)
  uint32_t res_bytes = 0;
};

// One device buffer of the last dfn_nerfh_commit, in commit order (dfn_nerfh_packed_buffer, dfn_nerfh_recommit_device).
// net: index of its PackedNet (nerfh_net_at; -1: extra, gen_blob); scale: dfn::recommit scale class of a split-f16 buffer, else -1.
struct PackedBufInfo {
  std::string name;
  void* ptr = nullptr;
  size_t bytes = 0;
  int net = -1;
  int scale = -1;
};

struct dfn_nerfh_s {
  dfn_nerfh_desc desc;
  std::map<std::string, std::vector<float>> params;
  bool committed = false;
  PackedNet net[2][3][dfn::kVariants];  // [coarse/fine][prec][kernel variant]
  PackedNet half_maps;             // kernel variant 6: the split-f16 fine network of the maps flavour (transient head at full height)
  PackedNet bwd[3];                // [prec] fine forward units + backward (W^T) units of the gradient kernel
                                   // (prec 2: split-f16 forward and backward units)
  PackedNet bwd_coarse[3];         // [prec] coarse forward units + the backward units of kBwdCoarseSeq (dfn_mlp_coarse_points_backward);
                                   // DFN_PREC_F32 and DFN_PREC_F16X3 only (plain f16 differentiates nothing: stays empty)
  PackedNet cstatic[3];            // [prec] the coarse network along kCoarseStaticSeq (split-f16 at netwidth 128: kCoarseStaticFoldSeq, PrecX3M16):
                                   // dfn_mlp_coarse_static_points
  PackedNet bwd_cstatic[3];        // [prec] its forward units (plain sequence) + the backward units of kBwdCoarseStaticSeq
                                   // (dfn_mlp_coarse_static_points_backward); netwidth 128, DFN_PREC_F32 and DFN_PREC_F16X3 only
  float* extra = nullptr;  // w_dir^T | b_dir | w_tr^T | b_tr | emb_a | emb_t | b_dir + W_dir[:, :W] b_final | b_tr + W_tr[:, :W] b_final
                           // | coarse w_dir^T [27][W/2] | coarse b_dir | coarse b_dir + W_dir[:, :W] b_final
  dfn::RayBiasWeights rb{};
  dfn::RayBiasWeights rb_fold{};   // rb with the two folded bias vectors: the table of kernel variant 5's fine kernel, and of it alone
  // the COARSE dir_encoding.0's seeds (the training query): 27 direction columns, no appearance columns (hist_bin = 0), no transient
  // table (b_tr = b_dir: table 1 is written and never read); _fold: with the folded bias, the table of the split-f16 kernel at netwidth 128
  dfn::RayBiasWeights rb_cstatic{}, rb_cstatic_fold{};
  bool fast = false;       // the register-resident MFMA kernels are packed (netwidth == dfn::kWidth)
  // Generic-width path (nerfh_train_api.hip): every parameter as a plain row-major fp32 device tensor, in the canonical
  // order of dfn_nerfh_train_param_name(); one allocation.
  float* gen_blob = nullptr;
  std::vector<const float*> gen_params;
  // Training step: the coarse network's backward runs beside the fine one's on this stream (created on first use), fenced by the
  // two events (nerfh_train_api.hip: dfn_nerfh_train_backward).
  int render_flags = 0;    // DFN_RENDER_* options of every render entry point (dfn_nerfh_set_render_options)
  int* range_flag = nullptr;   // device int the MLP kernels OR their range-guard bits into (dfn_nerfh_range_status)
  uint32_t* tile_counter = nullptr;   // kernel variant 12: two device words, the tile heads of the coarse [0] and the fine [1] kernel of the
                                      // pass in flight (zeroed on the render stream in front of each pass: one render per handle at a time)
  void* fused = nullptr;       // dfn::fused::State: staging-unit / destination tables of the fused training step (nerfh_fused_api.hip)
  bool train_forward_exact = false;   // which implementation the last dfn_nerfh_train_forward ran (dfn_nerfh_train_backward_rays needs the exact one)
  bool train_split_fine = false;   // DFN_TRAIN_FUSED_SPLIT: the fused step stores the fine network's operands as hi | lo planes too (nerfh_fused_train.h)
  bool train_forward_split = false; // ... as the last dfn_nerfh_train_forward laid the workspace out
  bool train_exact = false;    // dfn_nerfh_set_train_mode: run the training step on the layer-by-layer exact-fp32 products even at netwidth 128
  hipStream_t side_stream = nullptr;
  hipEvent_t side_ev[2] = {nullptr, nullptr};
  std::vector<PackedBufInfo> bufs;     // the buffers the last commit produced
  std::set<std::string> stale_params;  // host copies (params) a device re-commit left behind: dfn_nerfh_commit waits for all of them to be set again
  void* recommit = nullptr;            // dfn::recommit::State: the uploaded plan of dfn_nerfh_recommit_device (built on its first call)
};

// Every PackedNet of a handle under one index: net[f][prec][var], half_maps, bwd, bwd_coarse, cstatic, bwd_cstatic.
constexpr int kNerfhNets = 2 * 3 * dfn::kVariants + 1 + 4 * 3;
inline PackedNet* nerfh_net_at(dfn_nerfh_s* h, int i) {
  constexpr int nv = 2 * 3 * dfn::kVariants;
  if (i < 0 || i >= kNerfhNets) return nullptr;
  if (i < nv) return &h->net[0][0][0] + i;
  i -= nv;
  if (i == 0) return &h->half_maps;
  i -= 1;
  PackedNet* groups[4] = {h->bwd, h->bwd_coarse, h->cstatic, h->bwd_cstatic};
  return groups[i / 3] + i % 3;
}
inline int nerfh_net_index(dfn_nerfh_s* h, const PackedNet* n) {
  for (int i = 0; i < kNerfhNets; ++i)
    if (nerfh_net_at(h, i) == n) return i;
  return -1;
}

