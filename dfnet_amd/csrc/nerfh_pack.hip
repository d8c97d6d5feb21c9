// nerfh_pack.hip — the NeRF-H handle's life and its host packer: dfn_nerfh_create / set_param / commit / destroy, the packing of the
// reference's state_dict tensors into MFMA A-fragments (Packer), the table of a handle's packed networks (commit_core), and the plan
// build and host selfcheck of the device re-commit (nerfh_recommit.h).  No kernel is defined or launched here.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <map>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/dfnet_hip.h"
#include "dfn_common.h"
#include "nerfh_fused_train.h"
#include "nerfh_handle.h"
#include "nerfh_kernels.h"
#include "nerfh_layout.h"
#include "nerfh_recommit.h"

using namespace dfn;

// ------------------------------------------------------------------------------------------ handle (nerfh_handle.h)
static std::map<std::string, std::vector<size_t>> expected_shapes(const dfn_nerfh_desc& d) {
  std::map<std::string, std::vector<size_t>> m;
  const size_t W = d.width, na = size_t(d.hist_bin) * d.dim_a, nt = size_t(d.hist_bin) * d.dim_t;
  for (int f = 0; f < 2; ++f) {
    const std::string pre = f ? "fine." : "coarse.";
    for (int i = 0; i < d.depth; ++i) {
      const size_t k = i == 0 ? kChXyz : (i == 4 ? W + kChXyz : W);
      m[pre + "xyz_encoding_" + std::to_string(i + 1) + ".0.weight"] = {W, k};
      m[pre + "xyz_encoding_" + std::to_string(i + 1) + ".0.bias"] = {W};
    }
    m[pre + "xyz_encoding_final.weight"] = {W, W};
    m[pre + "xyz_encoding_final.bias"] = {W};
    m[pre + "dir_encoding.0.weight"] = {W / 2, W + kChDir + (f ? na : 0)};
    m[pre + "dir_encoding.0.bias"] = {W / 2};
    m[pre + "static_sigma.0.weight"] = {1, W};
    m[pre + "static_sigma.0.bias"] = {1};
    m[pre + "static_rgb.0.weight"] = {3, W / 2};
    m[pre + "static_rgb.0.bias"] = {3};
    if (f) {
      const size_t ks[4] = {W + nt, W / 2, W / 2, W / 2};
      for (int j = 0; j < 4; ++j) {
        m[pre + "transient_encoding." + std::to_string(2 * j) + ".weight"] = {W / 2, ks[j]};
        m[pre + "transient_encoding." + std::to_string(2 * j) + ".bias"] = {W / 2};
      }
      m[pre + "transient_sigma.0.weight"] = {1, W / 2};
      m[pre + "transient_sigma.0.bias"] = {1};
      m[pre + "transient_rgb.0.weight"] = {3, W / 2};
      m[pre + "transient_rgb.0.bias"] = {3};
      m[pre + "transient_beta.0.weight"] = {1, W / 2};
      m[pre + "transient_beta.0.bias"] = {1};
    }
  }
  m["embedding_a.weight"] = {size_t(d.n_vocab), size_t(d.dim_a)};
  m["embedding_t.weight"] = {size_t(d.n_vocab), size_t(d.dim_t)};
  return m;
}

extern "C" int dfn_nerfh_create(const dfn_nerfh_desc* desc, dfn_nerfh_t* out) {
  if (!desc || !out) return set_error(DFN_ERR_ARG, "dfn_nerfh_create: null argument");
  if (desc->depth != 8 || desc->multires != kLxyz || desc->multires_views != kLdir)
    return set_error(DFN_ERR_UNSUPPORTED,
                     "dfn_nerfh_create: kernels are specialised for netdepth=8 multires=%d multires_views=%d (got %d/%d/%d)",
                     kLxyz, kLdir, desc->depth, desc->multires, desc->multires_views);
  // netwidth: %d runs on the register-resident MFMA kernels; any other even width runs on the generic layer-by-layer
  // fp32-MFMA path (nerfh_train_api.hip), which is also the training path.
  if (desc->width < 2 || desc->width > 1024 || (desc->width & 1))
    return set_error(DFN_ERR_UNSUPPORTED, "dfn_nerfh_create: netwidth must be even and in [2, 1024] (got %d)", desc->width);
  if (desc->hist_bin <= 0 || desc->dim_a <= 0 || desc->dim_t <= 0 || desc->n_vocab <= 0 ||
      desc->hist_bin * (desc->dim_a + desc->dim_t) > 1024)
    return set_error(DFN_ERR_ARG, "dfn_nerfh_create: bad embedding geometry");
  auto* h = new dfn_nerfh_s();
  h->desc = *desc;
  *out = h;
  return DFN_OK;
}

static void free_packed(dfn_nerfh_s* h) {
  for (int i = 0; i < kNerfhNets; ++i) {
    PackedNet* n = nerfh_net_at(h, i);
    if (n->blob) (void)hipFree(n->blob);
    if (n->tab) (void)hipFree(n->tab);
    if (n->res_blob) (void)hipFree(n->res_blob);
    *n = PackedNet();
  }
  if (h->extra) (void)hipFree(h->extra);
  h->extra = nullptr;
  if (h->gen_blob) (void)hipFree(h->gen_blob);
  h->gen_blob = nullptr;
  h->gen_params.clear();
  h->bufs.clear();
  h->fast = false;
}

extern "C" int dfn_nerfh_destroy(dfn_nerfh_t h) {
  if (!h) return DFN_OK;
  free_packed(h);
  dfn::fused::destroy_state(h);
  dfn::recommit::destroy_state(h);
  for (hipEvent_t e : h->side_ev) if (e) (void)hipEventDestroy(e);
  if (h->side_stream) (void)hipStreamDestroy(h->side_stream);
  if (h->range_flag) (void)hipFree(h->range_flag);
  if (h->tile_counter) (void)hipFree(h->tile_counter);
  delete h;
  return DFN_OK;
}

extern "C" int dfn_nerfh_set_param(dfn_nerfh_t h, const char* name, const float* host, size_t numel) {
  if (!h || !name || !host) return set_error(DFN_ERR_ARG, "dfn_nerfh_set_param: null argument");
  const auto shapes = expected_shapes(h->desc);
  const auto it = shapes.find(name);
  if (it == shapes.end()) return set_error(DFN_ERR_ARG, "dfn_nerfh_set_param: unknown parameter '%s'", name);
  size_t want = 1;
  for (size_t s : it->second) want *= s;
  if (want != numel)
    return set_error(DFN_ERR_ARG, "dfn_nerfh_set_param: '%s' has %zu elements, expected %zu", name, numel, want);
  h->params[name].assign(host, host + numel);
  h->stale_params.erase(name);
  h->committed = false;
  return DFN_OK;
}

// ------------------------------------------------------------------------------------------ packing
namespace {

struct Mat {  // a state_dict Linear
  const float* w = nullptr;
  const float* b = nullptr;
  int rows = 0, cols = 0;
  int wid = -1, bid = -1;   // plan mode: the sources behind w and b (canonical parameter index, or a pseudo-parameter of fold_final)
};

// index of a parameter in the canonical order of dfn_nerfh_train_param_name()
int param_index(const std::string& name) {
  static const std::map<std::string, int> ids = [] {
    std::map<std::string, int> m;
    for (int i = 0; i < dfn_nerfh_train_param_count(); ++i) m[dfn_nerfh_train_param_name(i)] = i;
    return m;
  }();
  const auto it = ids.find(name);
  return it == ids.end() ? -1 : it->second;
}

// What Packer::pack lays out: which layer sequence of nerfh_layout.h, in what staging units.
enum PackSeq { SEQ_COARSE, SEQ_FINE, SEQ_CSTATIC };   // kCoarseSeq, kFineSeq, the coarse training query's kCoarseStaticSeq ("coarse." weights)
struct PackOpts {
  PackSeq seq = SEQ_COARSE;
  bool fold = false;      // xyz_encoding_final folded into the layers it feeds: kFineFoldSeq / kCoarseStaticFoldSeq (Packer::fold_dir, fold_tr)
  int umb = 1;            // M-blocks per staging unit
  int l5_umb = -1;        // ... of layer 5 (< 0: as the other layers)
  bool merge = false;     // umb >= 8: a unit holds whole layers and the small layers of one group (kFineGroup / kCoarseGroup) share one
  // kernel variant 7 (plain units only): the layers of kFineResident / kCoarseResident go here instead, unit after unit in execution
  // order in the same fragment and bias-block format but without the rounding to pieces (nerfh_layout.h: resident_offset); blob and
  // tab then hold the streamed units alone.  The set is zero-padded once to whole pieces.
  std::vector<uint8_t>* res = nullptr;
};

struct Packer {
  const dfn_nerfh_s* h;
  std::string pre;
  int width() const { return h->desc.width; }
  mutable int fwd_units = 0;   // pack_bwd: number of forward units at the head of the table
  // kernel variant 5 (kFineFoldSeq): dir_encoding.0[:, :W] . xyz_encoding_final and transient_encoding.0[:, :W] . xyz_encoding_final,
  // row-major [W / 2][W] (fold_final)
  const float *fold_dir = nullptr, *fold_tr = nullptr;
  int fold_dir_id = -1, fold_tr_id = -1;   // plan mode: their pseudo-parameters
  // Plan mode (nerfh_recommit.h): every store of a parameter's value below goes through emit_w / emit_b, which then also records
  // where the value came from.  target() names the buffer the next pack_blocks / pack_bwd_blocks call writes into.
  recommit::HostPlan* plan = nullptr;
  int buf_main = -1, buf_res = -1;
  mutable const uint8_t* origin = nullptr;
  mutable int cur_buf = -1;
  void target(const std::vector<uint8_t>& v, int buf) const { origin = v.data(); cur_buf = buf; }
  template <bool kSplit, class Elem>
  void emit_w(Elem* dst, const Mat& m, ptrdiff_t idx) const {   // idx < 0: zero
    const float v = idx >= 0 ? m.w[idx] : 0.f;
    if constexpr (kSplit) {   // [hi plane][lo plane] of a 1024-half fragment
      const Elem hi = Elem(v * wscale);
      dst[0] = hi;
      dst[512] = Elem(v * wscale - float(hi));
    } else {
      dst[0] = Elem(v);
    }
    if (plan && idx >= 0)
      plan->add(cur_buf, kSplit ? recommit::K_SPLIT : (sizeof(Elem) == 2 ? recommit::K_F16 : recommit::K_F32),
                size_t(reinterpret_cast<const uint8_t*>(dst) - origin), m.wid, size_t(idx));
  }
  void emit_b(float* dst, const Mat& m, int row, bool split) const {   // row < 0: zero
    const float b = row >= 0 ? m.b[row] : 0.f;
    *dst = split ? b * wscale * kX3ActScale : b;
    if (plan && row >= 0)
      plan->add(cur_buf, split ? recommit::K_BIAS : recommit::K_F32, size_t(reinterpret_cast<const uint8_t*>(dst) - origin), m.bid, size_t(row));
  }
  // kernel variant 6 (PrecX3M16): head M-blocks packed half-height, the fragments of their 16-row half ms = 0 only (head_row_m16 puts
  // head values c = 0..3 there): static_sigma and static_rgb; the transient head too where transient_beta (c = 4) is not wanted
  bool half_heads = false, half_thead = false;
  bool half_block(int layer) const { return half_heads && (layer == LY_SIG || layer == LY_RGB || (layer == LY_THEAD && half_thead)); }
  Mat mat(const std::string& key) const {
    Mat m;
    const auto& w = h->params.at(pre + key + ".weight");
    const auto& b = h->params.at(pre + key + ".bias");
    m.w = w.data();
    m.b = b.data();
    m.rows = int(b.size());
    m.cols = int(w.size() / b.size());
    if (plan) {
      m.wid = param_index(pre + key + ".weight");
      m.bid = param_index(pre + key + ".bias");
    }
    return m;
  }
  // Source (matrix, row) of row i of M-block mb of a layer; row < 0 = zero row.
  void row_source(int layer, int mb, int i, Mat& m, int& row) const {
    row = 32 * mb + i;
    switch (layer) {
      case LY_L1: case LY_L2: case LY_L3: case LY_L4: case LY_L5: case LY_L6: case LY_L7: case LY_L8:
        m = mat("xyz_encoding_" + std::to_string(layer - LY_L1 + 1) + ".0");
        break;
      case LY_FIN:
        if (mb < width() / 32) m = mat("xyz_encoding_final");
        else { m = mat("static_sigma.0"); row = i == 0 ? 0 : -1; }
        break;
      case LY_DIR: m = mat("dir_encoding.0"); break;
      case LY_RGB: m = mat("static_rgb.0"); row = i < 3 ? i : -1; break;
      case LY_TE0: m = mat("transient_encoding.0"); break;
      case LY_TE1: m = mat("transient_encoding.2"); break;
      case LY_TE2: m = mat("transient_encoding.4"); break;
      case LY_TE3: m = mat("transient_encoding.6"); break;
      case LY_THEAD:
        if (i < 3) { m = mat("transient_rgb.0"); row = i; }
        else if (i == 3) { m = mat("transient_sigma.0"); row = 0; }
        else if (i == 8) { m = mat("transient_beta.0"); row = 0; }
        else { m = mat("transient_beta.0"); row = -1; }
        break;
      case LY_SIG: m = mat("static_sigma.0"); row = i == 0 ? 0 : -1; break;
      case LY_DIRF: case LY_TE0F:   // no bias of their own (unit_has_bias): it is folded per ray
        m = Mat();
        m.w = layer == LY_DIRF ? fold_dir : fold_tr;
        m.wid = layer == LY_DIRF ? fold_dir_id : fold_tr_id;
        m.rows = width() / 2;
        m.cols = width();
        break;
    }
  }
  // Source column of slot s of half h; < 0 = zero.
  static int col_source(int layer, int hh, int s) {
    if (layer == LY_L1) return pe_xyz_feature(hh, s);
    if (layer == LY_L5) return s < 32 ? pe_xyz_feature(hh, s) : kChXyz + hidden_feature(hh, s - 32);
    return hidden_feature(hh, s);
  }
  // PrecX3M16: source column of slot s of lane group g (nerfh_layout.h: pe_xyz_feature_m16, hidden_feature_m16)
  static int col_source_m16(int layer, int g, int s) {
    if (layer == LY_L1) return pe_xyz_feature_m16(g, s);
    if (layer == LY_L5) return s < 16 ? pe_xyz_feature_m16(g, s) : kChXyz + hidden_feature_m16(g, s - 16);
    return hidden_feature_m16(g, s);
  }
  // M-blocks whose rows are heads (read back by the kernels) rather than the next layer's operand
  bool head_block(int layer, int mb) const {
    return layer == LY_RGB || layer == LY_THEAD || layer == LY_SIG || (layer == LY_FIN && mb == width() / 32);
  }
  // PrecX3M16: row of the 32-row M-block's weights behind packed row i (-1 = zero row), see head_row_m16
  int row_m16(int layer, int mb, int i) const { return head_block(layer, mb) ? head_row_m16(i) : i; }
  // The bias folded per ray (DIR, TE0) is NOT packed into the unit.
  static bool unit_has_bias(int layer) { return layer != LY_DIR && layer != LY_TE0 && layer != LY_DIRF && layer != LY_TE0F; }

  // One layer's M-blocks [mb0, mb0+group) as [A fragments][bias fragments], appended at `base`.
  // split-f16 (P::kSplit): a fragment is a hi plane then a lo plane of w * wscale; the bias is pre-multiplied by
  // wscale * kX3ActScale (what the accumulators carry).
  float wscale = 1.f;
  template <class P>
  void pack_blocks(int layer, int mb0, int group, uint8_t* base) const {
    using Elem = typename std::conditional<P::kSlotsPerChunk == 8, _Float16, float>::type;
    const LayerShape sh = layer_shape(layer, width());
    const int KC = sh.slots / P::kSlotsPerChunk;
    Elem* frag = reinterpret_cast<Elem*>(base);
    const bool half = P::kM16 && half_block(layer);   // KC / 2 fragments per M-block: kc = 0, 2, .. (ms = 0)
    const int KCP = half ? KC / 2 : KC;
    float* bias = reinterpret_cast<float*>(base + size_t(group) * KCP * 64 * P::kLaneBytes);
    for (int g = 0; g < group; ++g) {
      const int mb = mb0 + g;
      if constexpr (P::kM16) {
        // fragment kc = (32-K chunk kc >> 1, 16-row half kc & 1); lane l: row 16 (kc & 1) + (l & 15), slots 8 (kc >> 1) + j of group l >> 4
        auto source = [&](int i, Mat& m, int& row) {
          const int ri = row_m16(layer, mb, i);
          if (ri < 0) { m = Mat(); row = -1; return; }
          row_source(layer, mb, ri, m, row);
          if (row >= m.rows) row = -1;
        };
        for (int lane = 0; lane < 64; ++lane)
          for (int kc = 0; kc < KC; ++kc) {
            if (half && (kc & 1)) continue;
            Mat m;
            int row;
            source(16 * (kc & 1) + (lane & 15), m, row);
            for (int j = 0; j < 8; ++j) {
              const int col = col_source_m16(layer, lane >> 4, 8 * (kc >> 1) + j);
              Elem* fr = frag + (size_t(g) * KCP + (half ? kc >> 1 : kc)) * 64 * 16;
              emit_w<true>(fr + lane * 8 + j, m, (row >= 0 && col >= 0 && col < m.cols) ? ptrdiff_t(row) * m.cols + col : -1);
            }
          }
        for (int lg = 0; lg < 4; ++lg)   // bias block [g][ms][r] (load_bias_m16)
          for (int ms = 0; ms < 2; ++ms)
            for (int r = 0; r < 4; ++r) {
              Mat m;
              int row;
              source(16 * ms + 4 * lg + r, m, row);
              emit_b(&bias[g * 32 + lg * 8 + ms * 4 + r], m, unit_has_bias(layer) ? row : -1, true);
            }
        continue;
      }
      for (int lane = 0; lane < 64; ++lane) {
        const int i = lane & 31, hh = lane >> 5;
        Mat m;
        int row;
        row_source(layer, mb, i, m, row);
        if (row >= m.rows) row = -1;
        for (int kc = 0; kc < KC; ++kc)
          for (int j = 0; j < P::kSlotsPerChunk; ++j) {
            const int col = col_source(layer, hh, kc * P::kSlotsPerChunk + j);
            const ptrdiff_t idx = (row >= 0 && col >= 0 && col < m.cols) ? ptrdiff_t(row) * m.cols + col : -1;
            if constexpr (P::kSplit) emit_w<true>(frag + (size_t(g) * KC + kc) * 64 * 16 + lane * 8 + j, m, idx);   // 1024 halves per fragment
            else emit_w<false>(frag + ((size_t(g) * KC + kc) * 64 + lane) * P::kSlotsPerChunk + j, m, idx);
          }
      }
      for (int hh = 0; hh < 2; ++hh)
        for (int r = 0; r < 16; ++r) {
          Mat m;
          int row;
          row_source(layer, mb, mblock_row(hh, r), m, row);
          if (row >= m.rows) row = -1;
          emit_b(&bias[(g * 2 + hh) * 16 + r], m, unit_has_bias(layer) ? row : -1, P::kSplit);
        }
    }
  }
  // Element of the backward (W^T) layer `layer` at row i of M-block mb, contraction slot s of half hh
  // (nerfh_layout.h: BwdLayerId).  Rows are INPUT features of the forward Linear, slots its OUTPUT features.
  struct Ref { Mat m; ptrdiff_t idx = -1; };   // idx < 0: zero
  Ref bwd_elem(int layer, int mb, int i, int hh, int s) const {
    const int k = 32 * mb + i;
    auto W = [](const Mat& m, int row, int col) {
      return (row >= 0 && row < m.rows && col >= 0 && col < m.cols) ? Ref{m, ptrdiff_t(row) * m.cols + col} : Ref();
    };
    auto pe_col = [&](int blk) { return pe_xyz_feature(mblock_half_of_row(i), 16 * blk + mblock_reg_of_row(i)); };
    const int j = hidden_feature(hh, s);
    switch (layer) {
      case BW_THEAD:
        if (j < 3) return W(mat("transient_rgb.0"), j, k);
        if (j == 3) return W(mat("transient_sigma.0"), 0, k);
        if (j == 8) return W(mat("transient_beta.0"), 0, k);
        return Ref();
      case BW_TE3: return W(mat("transient_encoding.6"), j, k);
      case BW_TE2: return W(mat("transient_encoding.4"), j, k);
      case BW_TE1: return W(mat("transient_encoding.2"), j, k);
      case BW_RGB: return j < 3 ? W(mat("static_rgb.0"), j, k) : Ref();
      case BW_FINCAT: {
        const bool dirpart = s >= 32;
        const int jj = hidden_feature(hh, s & 31);
        if (mb < 4) return W(mat(dirpart ? "dir_encoding.0" : "transient_encoding.0"), jj, k);
        if (!dirpart) return Ref();
        const int c = pe_dir_feature(mblock_half_of_row(i), mblock_reg_of_row(i));
        return c >= 0 ? W(mat("dir_encoding.0"), jj, kWidth + c) : Ref();
      }
      case BW_FIN:
        if (s < 64) return W(mat("xyz_encoding_final"), j, k);
        return (s == 64 && hh == 0) ? W(mat("static_sigma.0"), 0, k) : Ref();
      case BW_L5:
        if (mb < 4) return W(mat("xyz_encoding_5.0"), j, kChXyz + k);
        return W(mat("xyz_encoding_5.0"), j, pe_col(mb - 4));
      case BW_L1: return W(mat("xyz_encoding_1.0"), j, pe_col(mb));
      case BW_SIG: return (s == 0 && hh == 0) ? W(mat("static_sigma.0"), 0, k) : Ref();   // the coarse chain's seed layer
      case BW_DIRCAT: {   // BW_FINCAT's dir_encoding.0 half: M-blocks 0..3 d final, the 5th d pe_dir (the columns behind the W of `final`)
        if (mb < 4) return W(mat("dir_encoding.0"), j, k);
        const int c = pe_dir_feature(mblock_half_of_row(i), mblock_reg_of_row(i));
        return c >= 0 ? W(mat("dir_encoding.0"), j, kWidth + c) : Ref();
      }
      default: {  // BW_L8..BW_L6, BW_L4..BW_L2: 128 -> 128
        const int n = 8 - (layer - BW_L8);
        return W(mat("xyz_encoding_" + std::to_string(n) + ".0"), j, k);
      }
    }
  }
  template <class P>
  void pack_bwd_blocks(int layer, int mb0, int group, uint8_t* base) const {
    using Elem = typename std::conditional<P::kSlotsPerChunk == 8, _Float16, float>::type;
    const LayerShape sh = bwd_layer_shape(layer);
    const int KC = sh.slots / P::kSlotsPerChunk;
    Elem* frag = reinterpret_cast<Elem*>(base);  // bias fragments after the A fragments stay zero
    for (int g = 0; g < group; ++g)
      for (int lane = 0; lane < 64; ++lane)
        for (int kc = 0; kc < KC; ++kc)
          for (int j = 0; j < P::kSlotsPerChunk; ++j) {
            const Ref v = bwd_elem(layer, mb0 + g, lane & 31, lane >> 5, kc * P::kSlotsPerChunk + j);
            if constexpr (P::kSplit) emit_w<true>(frag + (size_t(g) * KC + kc) * 64 * 16 + lane * 8 + j, v.m, v.idx);   // as pack_blocks
            else emit_w<false>(frag + ((size_t(g) * KC + kc) * 64 + lane) * P::kSlotsPerChunk + j, v.m, v.idx);
          }
  }
  // Blob of a gradient kernel: the forward layers of o.seq in plain units (one per layer in f16, per M-block in fp32), then its backward
  // layers the same way: all of BwdLayerId for the fine net, kBwdCoarseSeq for the coarse one, kBwdCoarseStaticSeq for its training query.
  // o gives the sequence alone: the unit sizes are the gradient kernels' (bwd_fwd_unit_mb, bwd_unit_mb).
  template <class P>
  void pack_bwd(PackOpts o, std::vector<uint8_t>& blob, std::vector<uint32_t>& tab) const {
    o.umb = bwd_fwd_unit_mb<P>();
    pack<P>(o, blob, tab);
    fwd_units = int(tab.size() / 2);
    const int umb = bwd_unit_mb<P>();
    const bool stat = o.seq == SEQ_CSTATIC, coarse = o.seq != SEQ_FINE;
    for (int li = 0; li < (stat ? kBwdCoarseStaticLayers : (coarse ? kBwdCoarseLayers : int(BW_COUNT))); ++li) {
      const int layer = stat ? kBwdCoarseStaticSeq[li] : (coarse ? kBwdCoarseSeq[li] : li);
      const LayerShape sh = bwd_layer_shape(layer);
      for (int u0 = 0; u0 < sh.mb; u0 += umb) {
        // units of one or two M-blocks: BW_L5's two d pe M-blocks (4, 5) are staged BEFORE its four d h4 M-blocks — the kernel
        // folds d pe to three floats while only the layer's input is live (nerfh_bwd.hip)
        const int mb0 = (umb <= 2 && layer == BW_L5) ? (u0 < 2 ? 4 + u0 : u0 - 2) : u0;
        const int group = sh.mb - mb0 < umb ? sh.mb - mb0 : umb;
        pack_bwd_blocks<P>(layer, mb0, group, add_unit(blob, tab, unit_bytes<P>(sh.slots, group)));
      }
    }
  }

  // A new staging unit of `bytes` zero bytes at the end of blob: entered in tab and made the target of the emit helpers.
  uint8_t* add_unit(std::vector<uint8_t>& blob, std::vector<uint32_t>& tab, uint32_t bytes) const {
    const uint32_t off = uint32_t(blob.size());
    blob.resize(off + bytes, 0);
    tab.push_back(off);
    tab.push_back(bytes);
    target(blob, buf_main);
    return blob.data() + off;
  }
  template <class P>
  uint32_t blocks_bytes(int layer, int group) const {
    const LayerShape sh = layer_shape(layer, width());
    const bool half = P::kM16 && half_block(layer);
    return uint32_t(group) * (sh.slots / P::kSlotsPerChunk / (half ? 2 : 1)) * 64 * P::kLaneBytes + uint32_t(group) * 128;
  }

  // The packed blob: staging units in execution order, merged (PackOpts::merge) or of <= umb M-blocks of a layer.
  // SEQ_CSTATIC with fold: fold_dir holds the coarse dir_encoding.0[:, :W] . xyz_encoding_final; its groups are kCoarseStaticGroup.
  template <class P>
  void pack(const PackOpts& o, std::vector<uint8_t>& blob, std::vector<uint32_t>& tab) const {
    const bool fine = o.seq == SEQ_FINE, stat = o.seq == SEQ_CSTATIC;
    const int* seq = stat ? (o.fold ? kCoarseStaticFoldSeq : kCoarseStaticSeq) : fine ? (o.fold ? kFineFoldSeq : kFineSeq) : kCoarseSeq;
    const int* grp = stat ? kCoarseStaticGroup : fine ? kFineGroup : kCoarseGroup;
    const int nl = stat ? kCoarseStaticLayers : fine ? kFineLayers : kCoarseLayers;
    if (o.merge) {
      for (int li = 0; li < nl;) {
        int lj = li;
        uint32_t bytes = 0;
        while (lj < nl && grp[lj] == grp[li]) bytes += blocks_bytes<P>(seq[lj], layer_shape(seq[lj], width()).mb), ++lj;
        if (seq[li] == LY_L5) {  // split so that three staging buffers fit in LDS (nerfh_layout.h: l5_unit_mb)
          const LayerShape sh = layer_shape(LY_L5, width());
          const int g = l5_unit_mb(o.umb);
          for (int mb0 = 0; mb0 < sh.mb; mb0 += g) pack_blocks<P>(LY_L5, mb0, g, add_unit(blob, tab, unit_bytes<P>(sh.slots, g)));
          li = lj;
          continue;
        }
        uint8_t* at = add_unit(blob, tab, align_piece(bytes));
        for (int l = li; l < lj; ++l) {
          pack_blocks<P>(seq[l], 0, layer_shape(seq[l], width()).mb, at);
          at += blocks_bytes<P>(seq[l], layer_shape(seq[l], width()).mb);
        }
        li = lj;
      }
      return;
    }
    for (int li = 0; li < nl; ++li) {
      const LayerShape sh = layer_shape(seq[li], width());
      const int lu = (seq[li] == LY_L5 && o.l5_umb > 0) ? o.l5_umb : o.umb;
      for (int mb0 = 0; mb0 < sh.mb; mb0 += lu) {
        const int group = sh.mb - mb0 < lu ? sh.mb - mb0 : lu;
        if (o.res && layer_resident(fine, seq[li])) {
          const size_t at = o.res->size();
          o.res->resize(at + blocks_bytes<P>(seq[li], group), 0);
          target(*o.res, buf_res);
          pack_blocks<P>(seq[li], mb0, group, o.res->data() + at);
          continue;
        }
        pack_blocks<P>(seq[li], mb0, group, add_unit(blob, tab, unit_bytes<P>(sh.slots, group, P::kM16 && half_block(seq[li]))));
      }
    }
    if (o.res) o.res->resize(align_piece(uint32_t(o.res->size())), 0);
  }
};

// xyz_encoding_final is a Linear without activation whose output feeds only the first W columns of dir_encoding.0 and
// transient_encoding.0:  A[:, :W] (F h + b_F) = (A[:, :W] F) h + A[:, :W] b_F.  Both products in double, rounded to float once.
// a: [rows][lda] row-major (its first W columns are used), F: [W][W], b_F: [W]  ->  af [rows][W], ab [rows].
void fold_final(const std::vector<float>& a, int rows, int lda, const std::vector<float>& F, const std::vector<float>& bF, int W,
                std::vector<float>& af, std::vector<float>& ab) {
  af.assign(size_t(rows) * W, 0.f);
  ab.assign(rows, 0.f);
  std::vector<double> acc(W);
  for (int r = 0; r < rows; ++r) {
    std::fill(acc.begin(), acc.end(), 0.0);
    double b = 0.0;
    for (int k = 0; k < W; ++k) {
      const double ark = a[size_t(r) * lda + k];
      const float* frow = &F[size_t(k) * W];
      for (int c = 0; c < W; ++c) acc[c] += ark * double(frow[c]);
      b += ark * double(bF[k]);
    }
    for (int c = 0; c < W; ++c) af[size_t(r) * W + c] = float(acc[c]);
    ab[r] = float(b);
  }
}

int upload(const void* src, size_t bytes, void** dst) {
  if (hipMalloc(dst, bytes ? bytes : 16) != hipSuccess) return set_error(DFN_ERR_HIP, "hipMalloc(%zu) failed", bytes);
  if (bytes && hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice) != hipSuccess)
    return set_error(DFN_ERR_HIP, "hipMemcpy H2D (%zu bytes) failed", bytes);
  return DFN_OK;
}

// ------------------------------------------------------------------------------------------ commit
enum { FIELD_BLOB = 0, FIELD_RES = 1, FIELD_EXTRA = 2, FIELD_GEN = 3 };

// Where the packed buffers of commit_core go: to the device (dfn_nerfh_commit) or into host vectors (the plan build of
// dfn_nerfh_recommit_device and dfn_nerfh_recommit_selfcheck: no device call).  A buffer's index is reserved BEFORE it is packed, so
// that the packer's plan entries can name it; the order of the reserve() calls is the order dfn_nerfh_packed_buffer enumerates.
struct CommitSink {
  dfn_nerfh_s* h;
  bool device;
  recommit::HostPlan* plan = nullptr;
  std::vector<recommit::BufShape> shapes;
  std::vector<void*> ptrs;                   // device mode
  std::vector<std::vector<uint8_t>> bytes;   // host mode
  std::vector<uint32_t> tabs[kNerfhNets];    // host mode: the unit table of each PackedNet (nerfh_net_at)
  int reserve() {
    shapes.emplace_back();
    ptrs.push_back(nullptr);
    bytes.emplace_back();
    return int(shapes.size()) - 1;
  }
  int put(int id, const std::string& name, PackedNet* n, int field, int scale, const void* data, size_t nbytes) {
    recommit::BufShape& b = shapes[id];
    b.name = name;
    b.bytes = nbytes;
    b.net = n ? nerfh_net_index(h, n) : -1;
    b.field = field;
    b.scale = scale;
    if (!device) {
      bytes[id].assign(static_cast<const uint8_t*>(data), static_cast<const uint8_t*>(data) + nbytes);
      return DFN_OK;
    }
    void* p = nullptr;
    if (int rc = upload(data, nbytes, &p)) return rc;
    ptrs[id] = p;
    if (field == FIELD_BLOB) n->blob = static_cast<char*>(p);
    else if (field == FIELD_RES) n->res_blob = static_cast<char*>(p);
    else if (field == FIELD_EXTRA) h->extra = static_cast<float*>(p);
    else h->gen_blob = static_cast<float*>(p);
    return DFN_OK;
  }
  int put_net(int id, const std::string& name, PackedNet& n, int scale, const std::vector<uint8_t>& blob, const std::vector<uint32_t>& tab) {
    if (int rc = put(id, name + ".blob", &n, FIELD_BLOB, scale, blob.data(), blob.size())) return rc;
    n.n_units = int(tab.size() / 2);
    if (device) return upload(tab.data(), tab.size() * 4, reinterpret_cast<void**>(&n.tab));
    tabs[shapes[id].net] = tab;
    return DFN_OK;
  }
  void publish() {   // device mode: the handle's buffer list
    h->bufs.clear();
    for (size_t i = 0; i < shapes.size(); ++i) h->bufs.push_back(PackedBufInfo{shapes[i].name, ptrs[i], shapes[i].bytes, shapes[i].net, shapes[i].scale});
  }
};

// ---- the table of packed networks: one NetRow per PackedNet of a handle, all of them packed by pack_net
const char* const kPrecNames[3] = {"f16", "f32", "f16x3"};
const char* const kNetPrefix[2] = {"coarse.", "fine."};
std::string net_name(int f, int prec, int var) { return std::string("net.") + kNetPrefix[f] + kPrecNames[prec] + ".v" + std::to_string(var); }

// The precision traits (nerfh_layout.h) a network's units are laid out for; kPlainTraits: those of a DFN_PREC_* on the plain kernels.
enum Traits { T_F16, T_F32, T_X3, T_X3M16 };
const Traits kPlainTraits[3] = {T_F16, T_F32, T_X3};
template <class F>
auto with_traits(Traits t, F&& f) {   // f(P()) for the traits type P behind t
  switch (t) {
    case T_F16: return f(PrecF16());
    case T_F32: return f(PrecF32());
    case T_X3: return f(PrecX3());
    default: return f(PrecX3M16());
  }
}

struct NetRow {
  PackedNet* net;        // receives the result
  std::string name;      // its buffers: "<name>.blob" and, resident, "<name>.res"
  const char* pre;       // prefix of the parameters it packs
  Traits traits;
  PackOpts opts;
  int scale = -1;        // split-f16 (T_X3, T_X3M16): its scale class (recommit::scales_from_max); in_scale stays 1 otherwise
  bool bwd = false;      // a gradient blob (Packer::pack_bwd): opts.seq alone counts, n_fwd_units is recorded
  bool half_heads = false, half_thead = false;   // Packer's: half-height head M-blocks (T_X3M16)
  bool resident = false;                         // the resident layers go to a buffer of their own (PackOpts::res)
  // A second network packed from the same weights: its buffer index follows this row's, its buffers are put before this row's
  const NetRow* sibling = nullptr;
};

// What every row of one commit shares.  fold / fold_b (netwidth 128, else empty): the matrices and bias vectors of fold_final for fine
// dir_encoding.0, fine transient_encoding.0 and coarse dir_encoding.0: pseudo-parameters np + k and np + 3 + k of the plan.
struct CommitCtx {
  CommitSink& sink;
  float in_scale[recommit::kScales], wscale[recommit::kScales];
  std::vector<float> fold[3], fold_b[3];
};

// One packed network: reserve its buffer indices, pack, put.  Buffer indices follow the order of the reserve() calls, which is the
// order dfn_nerfh_packed_buffer enumerates and the plan's entries name.
int pack_net(CommitCtx& c, const NetRow& r) {
  PackedNet& n = *r.net;
  Packer pk{c.sink.h, r.pre};
  pk.plan = c.sink.plan;
  pk.buf_main = c.sink.reserve();
  pk.half_heads = r.half_heads;
  pk.half_thead = r.half_thead;
  std::vector<uint8_t> blob, rblob;
  std::vector<uint32_t> tab;
  PackOpts o = r.opts;
  if (r.resident) {
    pk.buf_res = c.sink.reserve();
    o.res = &rblob;
  }
  if (o.fold) {
    const int np = dfn_nerfh_train_param_count(), k = o.seq == SEQ_FINE ? 0 : 2;
    pk.fold_dir = c.fold[k].data();
    pk.fold_dir_id = np + k;
    pk.fold_tr = c.fold[1].data();   // read by the fine sequence alone
    pk.fold_tr_id = np + 1;
  }
  if (r.scale >= 0) {
    n.in_scale = c.in_scale[r.scale];
    pk.wscale = c.wscale[r.scale];
  }
  with_traits(r.traits, [&](auto p) {
    using P = decltype(p);
    if (r.bwd) pk.template pack_bwd<P>(o, blob, tab);
    else pk.template pack<P>(o, blob, tab);
  });
  if (r.sibling)
    if (int rc = pack_net(c, *r.sibling)) return rc;
  if (int rc = c.sink.put_net(pk.buf_main, r.name, n, r.scale, blob, tab)) return rc;
  if (r.bwd) n.n_fwd_units = pk.fwd_units;
  if (!r.resident) return DFN_OK;
  const uint32_t want = resident_bytes<PrecX3M16>(o.seq == SEQ_FINE);
  if (rblob.size() != want)
    return set_error(DFN_ERR_STATE, "dfn_nerfh_commit: the resident layers pack to %zu bytes, the kernels expect %u", rblob.size(), want);
  n.res_bytes = want;
  return c.sink.put(pk.buf_res, r.name + ".res", &n, FIELD_RES, r.scale, rblob.data(), rblob.size());
}

// The packing of dfn_nerfh_commit: every buffer of the handle from h->params into `sink`.  h's PackedNets receive n_units, in_scale and
// (device mode) the pointers; plan mode (sink.plan) records the source of every packed element on the way.
int commit_core(dfn_nerfh_s* h, CommitSink& sink) {
  recommit::HostPlan* const plan = sink.plan;
  const int np = dfn_nerfh_train_param_count();
  {  // generic-width path: plain device copies in canonical order
    std::vector<float> all;
    std::vector<size_t> offs;
    for (int i = 0; i < np; ++i) {
      const auto& v = h->params.at(dfn_nerfh_train_param_name(i));
      offs.push_back(all.size());
      if (plan) plan->copies.push_back(recommit::CopySeg{i, uint32_t(v.size()), all.size()});
      all.insert(all.end(), v.begin(), v.end());
      all.resize((all.size() + 3) & ~size_t(3));
    }
    const int id = sink.reserve();
    if (plan) plan->gen_buf = id;
    int rc = sink.put(id, "gen_blob", nullptr, FIELD_GEN, -1, all.data(), all.size() * 4);
    if (rc) return rc;
    if (sink.device)
      for (size_t o : offs) h->gen_params.push_back(h->gen_blob + o);
  }
  const int Wd = h->desc.width;
  if (Wd != kWidth && Wd != kMaxWidth) return DFN_OK;   // generic-width path only
  CommitCtx c{sink};
  {  // the split-f16 scales: the largest |weight| of each network, scanned once
    float wmax[2] = {0.f, 0.f};
    for (const auto& kv : h->params)
      if (const int net = recommit::scan_net(kv.first); net >= 0)
        for (float v : kv.second) wmax[net] = std::fmax(wmax[net], std::fabs(v));
    recommit::scales_from_max(wmax, c.in_scale, c.wscale);
  }
  if (Wd == kWidth) {
    // the folded matrices stay out of the scan above: wscale is what every other layer's operands were scaled for.  Their entries may
    // exceed the largest weight (sums of W products); as hi + lo f16 pairs of w x wscale that is harmless.
    const auto& p = h->params;
    const auto &F = p.at("fine.xyz_encoding_final.weight"), &bF = p.at("fine.xyz_encoding_final.bias");
    fold_final(p.at("fine.dir_encoding.0.weight"), Wd / 2, Wd + kChDir + h->desc.hist_bin * h->desc.dim_a, F, bF, Wd, c.fold[0], c.fold_b[0]);
    fold_final(p.at("fine.transient_encoding.0.weight"), Wd / 2, Wd + h->desc.hist_bin * h->desc.dim_t, F, bF, Wd, c.fold[1], c.fold_b[1]);
    fold_final(p.at("coarse.dir_encoding.0.weight"), Wd / 2, Wd + kChDir, p.at("coarse.xyz_encoding_final.weight"),
               p.at("coarse.xyz_encoding_final.bias"), Wd, c.fold[2], c.fold_b[2]);
  }
  // A forward row: sequence `seq` on traits t, in the staging units of the kernels that read it (nerfh_layout.h):
  // unit_mb_w256 at netwidth 256; else kernel variant var's unit_mb, layer 5 by l5_unit_mb_p, merged units from 8 M-blocks on.
  // Split-f16: scale class 0 (coarse weights) or 1.
  auto fwd_row = [&](PackedNet& n, const std::string& name, PackSeq seq, Traits t, int var) {
    NetRow r{&n, name, kNetPrefix[seq == SEQ_FINE], t};
    PackOpts& o = r.opts;
    o.seq = seq;
    r.scale = t == T_X3 || t == T_X3M16 ? int(seq == SEQ_FINE) : -1;
    with_traits(t, [&](auto tr) {
      using P = decltype(tr);
      o.umb = Wd == kMaxWidth ? unit_mb_w256<P>() : unit_mb<P>(var);
      o.l5_umb = l5_unit_mb_p<P>(o.umb);
      o.merge = o.umb >= 8;
    });
    return r;
  };
  // A gradient row "<name><prec>" on the plain traits of `prec`: forward units of `seq`, then its backward units.  Scale class 2 or 3.
  auto bwd_row = [&](PackedNet* nets, const char* name, PackSeq seq, int prec) {
    NetRow r{&nets[prec], std::string(name) + kPrecNames[prec], kNetPrefix[seq == SEQ_FINE], kPlainTraits[prec]};
    r.opts.seq = seq;
    r.bwd = true;
    r.scale = prec == DFN_PREC_F16X3 ? 2 + int(seq == SEQ_FINE) : -1;
    return r;
  };
  const int grad_precs[2] = {DFN_PREC_F32, DFN_PREC_F16X3};   // plain f16 differentiates nothing
  if (Wd == kMaxWidth) {   // netwidth 256: one kernel variant per precision, plain staging units (nerfh_mlp.hip: launch_mlp)
    for (int f = 0; f < 2; ++f)
      for (int prec = 0; prec < 3; ++prec)
        if (int rc = pack_net(c, fwd_row(h->net[f][prec][0], net_name(f, prec, 0), f ? SEQ_FINE : SEQ_COARSE, kPlainTraits[prec], 0))) return rc;
    // the coarse network's training query (dfn_mlp_coarse_static_points), forward only: the plain sequence in the same staging units.
    // 1 245 184 B (f16, 40 units), 2 488 320 B (fp32, 78 units), 2 488 320 B (split-f16, 78 units)
    for (int prec = 0; prec < 3; ++prec)
      if (int rc = pack_net(c, fwd_row(h->cstatic[prec], std::string("cstatic.") + kPrecNames[prec], SEQ_CSTATIC, kPlainTraits[prec], 0))) return rc;
  } else {   // netwidth 128
    for (int f = 0; f < 2; ++f)
      for (int prec = 0; prec < 3; ++prec)
        for (int var = 0; var < kVariants; ++var) {
          // A variant with kernels of its own (kVariantFacts: base != var) packs the split-f16 networks they read and nothing else: the
          // fine one from the fold on, the coarse one from the half-height heads on; the rest of it is its base's (nerfh_route.h).
          // Half heads: also h->half_maps, the folded fine network with transient_beta's half (the maps flavour; variant 7 reads variant
          // 6's).  Resident: the resident layers leave the unit table for a blob of their own (res_blob).
          const VariantFacts vf = kVariantFacts[var];
          const bool x3 = prec == DFN_PREC_F16X3;
          if (vf.base != var && !(x3 && (f ? vf.fold : vf.half))) continue;
          NetRow r = fwd_row(h->net[f][prec][var], net_name(f, prec, var), f ? SEQ_FINE : SEQ_COARSE, x3 && vf.base == 4 ? T_X3M16 : kPlainTraits[prec], var);
          r.opts.fold = vf.fold && f == 1;
          r.half_heads = r.half_thead = vf.half;
          r.resident = vf.resident;
          NetRow maps = r;   // the maps flavour's network: the transient head at full height
          if (r.opts.fold && vf.half && !vf.resident) {
            maps.net = &h->half_maps;
            maps.name = "half_maps";
            maps.half_thead = false;
            r.sibling = &maps;
          }
          if (int rc = pack_net(c, r)) return rc;
        }
    // the fine network's gradient blob (nerfh_bwd.hip)
    for (int prec = 0; prec < 3; ++prec)
      if (int rc = pack_net(c, bwd_row(h->bwd, "bwd.", SEQ_FINE, prec))) return rc;
    // the coarse network's gradient blob (dfn_mlp_coarse_points_backward): 1 152 000 B + 552 B of unit table (fp32: 33 + 36 units) and
    // 1 117 184 B + 280 B (split-f16: 17 + 18 units), 2.27 MB per handle in all
    for (int prec : grad_precs)
      if (int rc = pack_net(c, bwd_row(h->bwd_coarse, "bwd_coarse.", SEQ_COARSE, prec))) return rc;
    // the coarse network's training query (dfn_mlp_coarse_static_points): the coarse weights along kCoarseStaticSeq in the staging units
    // of the fine point query's kernels (f16: merged, variant 0's; exact fp32: one M-block; split-f16: PrecX3M16 along
    // kCoarseStaticFoldSeq, the fold variant's units).  334 848 B + 88 B of unit table (f16, 11 units), 688 128 B + 320 B (fp32, 40
    // units), 603 136 B + 168 B (split-f16, 21 units)
    for (int prec = 0; prec < 3; ++prec) {
      const bool x3 = prec == DFN_PREC_F16X3;
      NetRow r = fwd_row(h->cstatic[prec], std::string("cstatic.") + kPrecNames[prec], SEQ_CSTATIC, x3 ? T_X3M16 : kPlainTraits[prec], x3 ? kFoldVariant : 0);
      r.opts.fold = x3;
      if (int rc = pack_net(c, r)) return rc;
    }
    // ... and its gradient blob (dfn_mlp_coarse_static_points_backward): the plain forward sequence followed by kBwdCoarseStaticSeq.
    // 1 387 520 B + 664 B (fp32: 40 + 43 units) and 1 346 560 B + 344 B (split-f16: 21 + 22 units), 2.73 MB per handle; with the three
    // forward networks above 4.36 MB in all
    for (int prec : grad_precs)
      if (int rc = pack_net(c, bwd_row(h->bwd_cstatic, "bwd_cstatic.", SEQ_CSTATIC, prec))) return rc;
  }
  // per-ray-bias weights: transposed tails of dir_encoding.0 / transient_encoding.0 + embeddings
  const dfn_nerfh_desc& d = h->desc;
  const int na = d.hist_bin * d.dim_a, nt = d.hist_bin * d.dim_t, kd = kChDir + na, NO = Wd / 2;
  const auto& wd = h->params.at("fine.dir_encoding.0.weight");
  const auto& bd = h->params.at("fine.dir_encoding.0.bias");
  const auto& wt = h->params.at("fine.transient_encoding.0.weight");
  const auto& bt = h->params.at("fine.transient_encoding.0.bias");
  const auto& ea = h->params.at("embedding_a.weight");
  const auto& et = h->params.at("embedding_t.weight");
  std::vector<float> ex;
  const size_t o_wd = 0, o_bd = o_wd + size_t(kd) * NO, o_wt = o_bd + NO, o_bt = o_wt + size_t(nt) * NO,
               o_ea = o_bt + NO, o_et = o_ea + ea.size(), o_bdf = o_et + et.size(), o_btf = o_bdf + NO,
               o_cwd = o_btf + NO, o_cbd = o_cwd + size_t(kChDir) * NO, o_cbdf = o_cbd + NO;
  ex.resize(o_cbdf + NO);
  const int ex_id = sink.reserve();
  // ex[at] = value, which is element idx of source src (a canonical parameter, or a pseudo-parameter of fold_final)
  auto put_extra = [&](size_t at, float value, int src, size_t idx) {
    ex[at] = value;
    if (plan) plan->add(ex_id, recommit::K_F32, at * 4, src, idx);
  };
  const int i_wd = param_index("fine.dir_encoding.0.weight"), i_bd = param_index("fine.dir_encoding.0.bias"),
            i_wt = param_index("fine.transient_encoding.0.weight"), i_bt = param_index("fine.transient_encoding.0.bias"),
            i_ea = param_index("embedding_a.weight"), i_et = param_index("embedding_t.weight"),
            i_cwd = param_index("coarse.dir_encoding.0.weight"), i_cbd = param_index("coarse.dir_encoding.0.bias");
  const int ld_d = Wd + kd, ld_t = Wd + nt;
  for (int j = 0; j < kd; ++j)
    for (int f = 0; f < NO; ++f) put_extra(o_wd + size_t(j) * NO + f, wd[size_t(f) * ld_d + Wd + j], i_wd, size_t(f) * ld_d + Wd + j);
  for (int j = 0; j < nt; ++j)
    for (int f = 0; f < NO; ++f) put_extra(o_wt + size_t(j) * NO + f, wt[size_t(f) * ld_t + Wd + j], i_wt, size_t(f) * ld_t + Wd + j);
  for (int f = 0; f < NO; ++f) put_extra(o_bd + f, bd[f], i_bd, f);
  for (int f = 0; f < NO; ++f) put_extra(o_bt + f, bt[f], i_bt, f);
  for (size_t i = 0; i < ea.size(); ++i) put_extra(o_ea + i, ea[i], i_ea, i);
  for (size_t i = 0; i < et.size(); ++i) put_extra(o_et + i, et[i], i_et, i);
  // variant 5's per-ray seeds: b + W[:, :W] b_final (netwidth 256 has no variant 5: the plain biases)
  for (int f = 0; f < NO; ++f) {
    if (c.fold_b[0].empty()) put_extra(o_bdf + f, bd[f], i_bd, f);
    else put_extra(o_bdf + f, bd[f] + c.fold_b[0][f], np + 3, f);
    if (c.fold_b[1].empty()) put_extra(o_btf + f, bt[f], i_bt, f);
    else put_extra(o_btf + f, bt[f] + c.fold_b[1][f], np + 4, f);
  }
  {  // the coarse dir_encoding.0 [W/2, W + 27]: its 27 direction columns transposed, its bias, and the bias of the folded kernel
    const auto& cwd = h->params.at("coarse.dir_encoding.0.weight");
    const auto& cbd = h->params.at("coarse.dir_encoding.0.bias");
    for (int j = 0; j < kChDir; ++j)
      for (int f = 0; f < NO; ++f)
        put_extra(o_cwd + size_t(j) * NO + f, cwd[size_t(f) * (Wd + kChDir) + Wd + j], i_cwd, size_t(f) * (Wd + kChDir) + Wd + j);
    for (int f = 0; f < NO; ++f) {
      put_extra(o_cbd + f, cbd[f], i_cbd, f);
      if (c.fold_b[2].empty()) put_extra(o_cbdf + f, cbd[f], i_cbd, f);
      else put_extra(o_cbdf + f, cbd[f] + c.fold_b[2][f], np + 5, f);
    }
  }
  int rc = sink.put(ex_id, "extra", nullptr, FIELD_EXTRA, -1, ex.data(), ex.size() * 4);
  if (rc) return rc;
  h->fast = true;
  if (!sink.device) return DFN_OK;
  h->rb.w_dir = h->extra + o_wd;
  h->rb.b_dir = h->extra + o_bd;
  h->rb.w_tr = h->extra + o_wt;
  h->rb.b_tr = h->extra + o_bt;
  h->rb.emb_a = h->extra + o_ea;
  h->rb.emb_t = h->extra + o_et;
  h->rb.hist_bin = d.hist_bin;
  h->rb.dim_a = d.dim_a;
  h->rb.dim_t = d.dim_t;
  h->rb.n_vocab = d.n_vocab;
  h->rb.nout = NO;
  h->rb_fold = h->rb;
  h->rb_fold.b_dir = h->extra + o_bdf;
  h->rb_fold.b_tr = h->extra + o_btf;
  h->rb_cstatic = dfn::RayBiasWeights{h->extra + o_cwd, h->extra + o_cbd, h->extra + o_cwd, h->extra + o_cbd, h->extra + o_ea,
                                      h->extra + o_et, 0, 1, 1, d.n_vocab, NO};
  h->rb_cstatic_fold = h->rb_cstatic;
  h->rb_cstatic_fold.b_dir = h->rb_cstatic_fold.b_tr = h->extra + o_cbdf;
  return DFN_OK;
}
}  // namespace

extern "C" int dfn_nerfh_commit(dfn_nerfh_t h) {
  if (!h) return set_error(DFN_ERR_ARG, "dfn_nerfh_commit: null handle");
  for (const auto& kv : expected_shapes(h->desc))
    if (!h->params.count(kv.first)) return set_error(DFN_ERR_STATE, "dfn_nerfh_commit: parameter '%s' not set", kv.first.c_str());
  if (!h->stale_params.empty())   // the host copies are older than what dfn_nerfh_recommit_device packed: never re-pack from them
    return set_error(DFN_ERR_STATE, "dfn_nerfh_commit: parameter '%s' (and %zu more) not set again since dfn_nerfh_recommit_device",
                     h->stale_params.begin()->c_str(), h->stale_params.size() - 1);
  free_packed(h);
  dfn::fused::destroy_state(h);   // its tables follow the handle's geometry and scales: rebuilt on the next training step
  if (!h->range_flag) {   // range guard of the narrow arithmetic modes: three device ints (flag, fetch slot, the training step's own word), cleared here
    if (hipMalloc(reinterpret_cast<void**>(&h->range_flag), 3 * sizeof(int)) != hipSuccess) {
      h->range_flag = nullptr;
      return set_error(DFN_ERR_HIP, "dfn_nerfh_commit: allocating the range-guard flag failed");
    }
    if (hipMemset(h->range_flag, 0, 3 * sizeof(int)) != hipSuccess) return set_error(DFN_ERR_HIP, "dfn_nerfh_commit: clearing the range-guard flag failed");
  }
  if (!h->tile_counter) {   // kernel variant 12: the tile heads of the coarse and the fine kernel (zeroed in front of every pass that claims from them)
    if (hipMalloc(reinterpret_cast<void**>(&h->tile_counter), 2 * sizeof(uint32_t)) != hipSuccess) {
      h->tile_counter = nullptr;
      return set_error(DFN_ERR_HIP, "dfn_nerfh_commit: allocating the tile counters failed");
    }
  }
  CommitSink sink{h, true};
  if (int rc = commit_core(h, sink)) return rc;
  sink.publish();
  h->committed = true;
  return DFN_OK;
}

// ------------------------------------------------------------------------------------------ device re-commit: plan, inspection, selfcheck
namespace {
void scratch_params(dfn_nerfh_s& t, uint32_t seed, float coarse_mul, float fine_mul) {   // seed 0: zeros
  for (const auto& kv : expected_shapes(t.desc)) {
    size_t n = 1;
    for (size_t s : kv.second) n *= s;
    std::vector<float>& v = t.params[kv.first];
    v.assign(n, 0.f);
    if (!seed) continue;
    uint32_t st = seed * 2654435761u;
    for (char c : kv.first) st = st * 31u + uint32_t(c);
    const float mul = kv.first.compare(0, 7, "coarse.") == 0 ? coarse_mul : (kv.first.compare(0, 5, "fine.") == 0 ? fine_mul : 1.f);
    for (float& x : v) {
      st = st * 1664525u + 1013904223u;
      x = (float(st >> 8) * (1.f / 16777216.f) - 0.5f) * mul;
    }
  }
}

// 64-bit FNV-1a over everything a host-mode sink holds of a packed parameter set, buffer by buffer in enumeration order: name, byte
// count, bytes, and for a PackedNet's buffer the net's unit table, n_units, n_fwd_units, res_bytes and the bits of in_scale (integers
// as little-endian words).  dfn_nerfh_recommit_selfcheck prints it: a change of the packer shows in it without a device.
uint64_t packed_digest(dfn_nerfh_s* h, const CommitSink& sink) {
  uint64_t d = 0xcbf29ce484222325ull;
  auto eat = [&d](const void* p, size_t n) {
    for (size_t i = 0; i < n; ++i) d = (d ^ static_cast<const uint8_t*>(p)[i]) * 0x100000001b3ull;
  };
  auto word = [&eat](uint64_t v, int n) {
    for (int i = 0; i < n; ++i) { const uint8_t b = uint8_t(v >> (8 * i)); eat(&b, 1); }
  };
  for (size_t i = 0; i < sink.shapes.size(); ++i) {
    const recommit::BufShape& b = sink.shapes[i];
    eat(b.name.data(), b.name.size());
    word(b.bytes, 8);
    eat(sink.bytes[i].data(), sink.bytes[i].size());
    if (b.net < 0) continue;
    const PackedNet& n = *nerfh_net_at(h, b.net);
    for (uint32_t v : sink.tabs[b.net]) word(v, 4);
    word(uint32_t(n.n_units), 4);
    word(uint32_t(n.n_fwd_units), 4);
    word(n.res_bytes, 4);
    uint32_t bits;
    std::memcpy(&bits, &n.in_scale, 4);
    word(bits, 4);
  }
  return d;
}
}  // namespace

void dfn::recommit::fold_specs(const dfn_nerfh_desc& d, FoldSpec out[3]) {
  const int W = d.width;
  const int fF = param_index("fine.xyz_encoding_final.weight"), fb = param_index("fine.xyz_encoding_final.bias");
  out[0] = FoldSpec{param_index("fine.dir_encoding.0.weight"), fF, fb, param_index("fine.dir_encoding.0.bias"), W + kChDir + d.hist_bin * d.dim_a};
  out[1] = FoldSpec{param_index("fine.transient_encoding.0.weight"), fF, fb, param_index("fine.transient_encoding.0.bias"), W + d.hist_bin * d.dim_t};
  out[2] = FoldSpec{param_index("coarse.dir_encoding.0.weight"), param_index("coarse.xyz_encoding_final.weight"),
                    param_index("coarse.xyz_encoding_final.bias"), param_index("coarse.dir_encoding.0.bias"), W + kChDir};
}

int dfn::recommit::build_plan(const dfn_nerfh_desc& desc, HostPlan& plan, std::vector<BufShape>& shapes) {
  dfn_nerfh_s t;
  t.desc = desc;
  scratch_params(t, 0, 1.f, 1.f);
  CommitSink sink{&t, false};
  sink.plan = &plan;
  if (int rc = commit_core(&t, sink)) return rc;
  if (plan.overflow || dfn_nerfh_train_param_count() + kPseudo > kMaxSrc || int(sink.shapes.size()) > kMaxBufs)
    return set_error(DFN_ERR_UNSUPPORTED, "dfn_nerfh_recommit_device: this geometry does not fit the plan's entry format");
  shapes = sink.shapes;
  return DFN_OK;
}

extern "C" int dfn_nerfh_packed_buffer(dfn_nerfh_t h, int index, const char** name, const void** device_ptr, size_t* bytes, float* in_scale) {
  if (!h) return set_error(DFN_ERR_ARG, "dfn_nerfh_packed_buffer: null handle");
  if (!h->committed) return set_error(DFN_ERR_STATE, "dfn_nerfh_packed_buffer: handle not committed");
  if (index < 0 || index >= int(h->bufs.size()))
    return set_error(DFN_ERR_ARG, "dfn_nerfh_packed_buffer: index %d outside the handle's %zu buffers", index, h->bufs.size());
  const PackedBufInfo& b = h->bufs[index];
  if (name) *name = b.name.c_str();
  if (device_ptr) *device_ptr = b.ptr;
  if (bytes) *bytes = b.bytes;
  if (in_scale) *in_scale = b.net >= 0 ? nerfh_net_at(h, b.net)->in_scale : 1.f;
  return DFN_OK;
}

// Host-only check of the plan (no device call): pack parameter set A with the plan recorded, pack another set B, then re-commit A's
// buffers to B's values the way the device does -- maxima, scales, fold arena, plan entries, gen_blob segments, through the functions
// the kernels call (nerfh_recommit.h) -- and compare every buffer with B's byte for byte.
extern "C" int dfn_nerfh_recommit_selfcheck(int width) {
  using namespace dfn::recommit;
  if (width < 2 || width > 1024 || (width & 1)) return set_error(DFN_ERR_ARG, "dfn_nerfh_recommit_selfcheck: netwidth must be even and in [2, 1024] (got %d)", width);
  const dfn_nerfh_desc desc{8, width, kLxyz, kLdir, 10, 5, 2, 32};
  dfn_nerfh_s A, B;
  A.desc = B.desc = desc;
  scratch_params(A, 1, 1.f, 1.f);
  scratch_params(B, 2, 1.f / 64.f, 3.f);   // both weight scales move
  HostPlan plan;
  CommitSink sa{&A, false}, sb{&B, false};
  sa.plan = &plan;
  if (int rc = commit_core(&A, sa)) return rc;
  if (int rc = commit_core(&B, sb)) return rc;
  const int np = dfn_nerfh_train_param_count();
  if (plan.overflow || np + kPseudo > kMaxSrc || int(sa.shapes.size()) > kMaxBufs) return set_error(DFN_ERR_STATE, "selfcheck: the plan overflows its entry format");
  if (sa.shapes.size() != sb.shapes.size()) return set_error(DFN_ERR_STATE, "selfcheck: buffer lists differ");
  std::vector<const float*> src(np + kPseudo, nullptr);
  float wmax[2] = {0.f, 0.f};
  for (int i = 0; i < np; ++i) {
    const std::string name = dfn_nerfh_train_param_name(i);
    const std::vector<float>& v = B.params.at(name);
    src[i] = v.data();
    const int net = scan_net(name);
    if (net >= 0)
      for (float x : v)
        if (x == x && std::fabs(x) > wmax[net]) wmax[net] = std::fabs(x);
  }
  float in_scale[kScales], wscale[kScales];
  scales_from_max(wmax, in_scale, wscale);
  std::vector<float> arena(arena_floats(width), 0.f);
  if (width == kWidth) {
    FoldSpec fs[3];
    fold_specs(desc, fs);
    for (int k = 0; k < 3; ++k)
      for (int r = 0; r < width / 2; ++r)
        for (int c = 0; c <= width; ++c)
          arena[c < width ? arena_off(k, width) + size_t(r) * width + c : arena_off(3 + k, width) + r] =
              fold_elem(src[fs[k].a], fs[k].lda, src[fs[k].F], src[fs[k].bF], src[fs[k].bA], width, r, c);
  }
  for (int k = 0; k < kPseudo; ++k) src[np + k] = arena.data() + arena_off(k, width);
  for (const PlanElem& e : plan.elems) {
    const int buf = int(e.dst >> 24), sc = sa.shapes[buf].scale;
    if (!elem_in_bounds(e, sa.bytes[buf].size())) return set_error(DFN_ERR_STATE, "selfcheck: an entry leaves buffer %s", sa.shapes[buf].name.c_str());
    store_elem(reinterpret_cast<char*>(sa.bytes[buf].data()), e, src[e.src >> kIdxBits], sc >= 0 ? wscale[sc] : 1.f);
  }
  for (const CopySeg& c : plan.copies) std::memcpy(sa.bytes[plan.gen_buf].data() + c.dst_off * 4, src[c.src], size_t(c.numel) * 4);
  for (size_t i = 0; i < sa.shapes.size(); ++i) {
    const BufShape& a = sa.shapes[i];
    const BufShape& b = sb.shapes[i];
    if (a.name != b.name || a.bytes != b.bytes || a.scale != b.scale || a.net != b.net) return set_error(DFN_ERR_STATE, "selfcheck: buffer %zu differs in shape", i);
    for (size_t o = 0; o < a.bytes; ++o)
      if (sa.bytes[i][o] != sb.bytes[i][o])
        return set_error(DFN_ERR_STATE, "selfcheck: netwidth %d, buffer %s: byte %zu of %zu is 0x%02x after the plan, 0x%02x from the packer", width,
                         a.name.c_str(), o, a.bytes, sa.bytes[i][o], sb.bytes[i][o]);
    if (a.scale >= 0 && nerfh_net_at(&B, a.net)->in_scale != in_scale[a.scale])
      return set_error(DFN_ERR_STATE, "selfcheck: buffer %s: in_scale %g from the maxima, %g from the packer", a.name.c_str(), in_scale[a.scale],
                       nerfh_net_at(&B, a.net)->in_scale);
  }
  // DFN_OK: dfn_last_error() holds the plan's figures
  size_t total = 0, written = 0;
  for (const BufShape& b : sa.shapes) total += b.bytes;
  for (const PlanElem& e : plan.elems) written += ((e.dst >> kOffBits) & 3u) == K_F16 ? 2 : 4;
  for (const CopySeg& c : plan.copies) written += size_t(c.numel) * 4;
  return set_error(DFN_OK, "netwidth %d: %zu buffers of %zu bytes; plan of %zu entries (%zu bytes) and %zu segments; %zu bytes written per re-commit; "
                   "packed digest %016llx", width, sa.shapes.size(), total, plan.elems.size(), plan.elems.size() * sizeof(PlanElem), plan.copies.size(),
                   written, static_cast<unsigned long long>(packed_digest(&B, sb)));
}

