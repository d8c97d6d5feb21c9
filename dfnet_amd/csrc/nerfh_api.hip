// nerfh_api.hip — the C ABI (include/dfnet_hip.h) of the NeRF-H render path: handle, host-side
// packing of the reference's state_dict tensors into MFMA A-fragments, stage entry points and
// the whole-path dfn_render_rays / dfn_render_image drivers.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
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
#include "nerfh_route.h"

using namespace dfn;
static_assert(kPrecF16 == DFN_PREC_F16 && kPrecF32 == DFN_PREC_F32 && kPrecF16X3 == DFN_PREC_F16X3, "nerfh_route.h names the ABI's precisions");

// ------------------------------------------------------------------------------------------ errors
namespace dfn {
static thread_local char g_err[512] = "";
int set_error(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return code;
}
int device_cu_count() {
  static int n = 0;
  if (!n) {
    int dev = 0;
    hipDeviceProp_t p;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&p, dev) == hipSuccess) n = p.multiProcessorCount;
    if (n <= 0) n = 256;
  }
  return n;
}
}  // namespace dfn

extern "C" const char* dfn_last_error(void) { return g_err; }
extern "C" int dfn_abi_version(void) { return 1; }

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
  for (auto& a : h->net)
    for (auto& b : a)
      for (auto& n : b) {
        if (n.blob) (void)hipFree(n.blob);
        if (n.tab) (void)hipFree(n.tab);
        if (n.res_blob) (void)hipFree(n.res_blob);
        n = PackedNet();
      }
  for (PackedNet* n : {&h->bwd[0], &h->bwd[1], &h->bwd[2], &h->half_maps, &h->bwd_coarse[0], &h->bwd_coarse[1], &h->bwd_coarse[2],
                       &h->cstatic[0], &h->cstatic[1], &h->cstatic[2], &h->bwd_cstatic[0], &h->bwd_cstatic[1], &h->bwd_cstatic[2]}) {
    if (n->blob) (void)hipFree(n->blob);
    if (n->tab) (void)hipFree(n->tab);
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

struct Packer {
  const dfn_nerfh_s* h;
  std::string pre;
  int width() const { return h->desc.width; }
  mutable int fwd_units = 0;   // pack_bwd: number of forward units at the head of the table
  // kernel variant 5 (kFineFoldSeq): dir_encoding.0[:, :W] . xyz_encoding_final and transient_encoding.0[:, :W] . xyz_encoding_final,
  // row-major [W / 2][W] (fold_final)
  std::vector<float> fold_dir, fold_tr;
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
        m.w = (layer == LY_DIRF ? fold_dir : fold_tr).data();
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
  // Blob of the gradient kernel: the fine net's forward layers, one unit per layer (f16) / per M-block (f32),
  // then the backward layers the same way.  coarse: the coarse net's forward layers (kCoarseSeq), then the layers of kBwdCoarseSeq.
  // stat (with coarse): the coarse net's training query, kCoarseStaticSeq then kBwdCoarseStaticSeq.
  template <class PF, class P>
  void pack_bwd(std::vector<uint8_t>& blob, std::vector<uint32_t>& tab, bool coarse = false, bool stat = false) const {
    pack<PF>(!coarse, bwd_fwd_unit_mb<PF>(), false, blob, tab, -1, false, nullptr, stat);
    fwd_units = int(tab.size() / 2);
    const int umb = bwd_unit_mb<P>();
    for (int li = 0; li < (stat ? kBwdCoarseStaticLayers : (coarse ? kBwdCoarseLayers : int(BW_COUNT))); ++li) {
      const int layer = stat ? kBwdCoarseStaticSeq[li] : (coarse ? kBwdCoarseSeq[li] : li);
      const LayerShape sh = bwd_layer_shape(layer);
      for (int u0 = 0; u0 < sh.mb; u0 += umb) {
        // units of one or two M-blocks: BW_L5's two d pe M-blocks (4, 5) are staged BEFORE its four d h4 M-blocks — the kernel
        // folds d pe to three floats while only the layer's input is live (nerfh_bwd.hip)
        const int mb0 = (umb <= 2 && layer == BW_L5) ? (u0 < 2 ? 4 + u0 : u0 - 2) : u0;
        const int group = sh.mb - mb0 < umb ? sh.mb - mb0 : umb;
        const uint32_t bytes = unit_bytes<P>(sh.slots, group);
        const uint32_t off = uint32_t(blob.size());
        blob.resize(off + bytes, 0);
        tab.push_back(off);
        tab.push_back(bytes);
        target(blob, buf_main);
        pack_bwd_blocks<P>(layer, mb0, group, blob.data() + off);
      }
    }
  }

  template <class P>
  uint32_t blocks_bytes(int layer, int group) const {
    const LayerShape sh = layer_shape(layer, width());
    const bool half = P::kM16 && half_block(layer);
    return uint32_t(group) * (sh.slots / P::kSlotsPerChunk / (half ? 2 : 1)) * 64 * P::kLaneBytes + uint32_t(group) * 128;
  }

  // The packed blob: staging units in execution order.  umb >= 8: a unit holds whole layers and the small
  // layers of one group (kFineGroup / kCoarseGroup) share a unit; otherwise a unit is <= umb M-blocks of a layer.
  // l5_umb: M-blocks per unit of layer 5 (< 0: the same as the other layers)
  // res (kernel variant 7, plain units only): the layers of kFineResident / kCoarseResident go there instead, unit after unit in
  // execution order in the same fragment and bias-block format but without the rounding to pieces (nerfh_layout.h: resident_offset);
  // blob and tab then hold the streamed units alone.  The set is zero-padded once to whole pieces.
  // stat (fine = false, the "coarse." prefix): the coarse network's training query, kCoarseStaticSeq / kCoarseStaticFoldSeq (fold: fold_dir
  // holds the coarse dir_encoding.0[:, :W] . xyz_encoding_final) with kCoarseStaticGroup.
  template <class P>
  void pack(bool fine, int umb, bool merge, std::vector<uint8_t>& blob, std::vector<uint32_t>& tab, int l5_umb = -1, bool fold = false,
            std::vector<uint8_t>* res = nullptr, bool stat = false) const {
    const int* seq = stat ? (fold ? kCoarseStaticFoldSeq : kCoarseStaticSeq) : fine ? (fold ? kFineFoldSeq : kFineSeq) : kCoarseSeq;
    const int* grp = stat ? kCoarseStaticGroup : fine ? kFineGroup : kCoarseGroup;
    const int nl = stat ? kCoarseStaticLayers : fine ? kFineLayers : kCoarseLayers;
    if (merge) {
      for (int li = 0; li < nl;) {
        int lj = li;
        uint32_t bytes = 0;
        while (lj < nl && grp[lj] == grp[li]) bytes += blocks_bytes<P>(seq[lj], layer_shape(seq[lj], width()).mb), ++lj;
        if (seq[li] == LY_L5) {  // split so that three staging buffers fit in LDS (nerfh_layout.h: l5_unit_mb)
          const LayerShape sh = layer_shape(LY_L5, width());
          const int g = l5_unit_mb(umb);
          for (int mb0 = 0; mb0 < sh.mb; mb0 += g) {
            const uint32_t ub = unit_bytes<P>(sh.slots, g), uo = uint32_t(blob.size());
            blob.resize(uo + ub, 0);
            tab.push_back(uo);
            tab.push_back(ub);
            target(blob, buf_main);
            pack_blocks<P>(LY_L5, mb0, g, blob.data() + uo);
          }
          li = lj;
          continue;
        }
        const uint32_t off = uint32_t(blob.size());
        blob.resize(off + align_piece(bytes), 0);
        tab.push_back(off);
        tab.push_back(align_piece(bytes));
        uint32_t at = off;
        target(blob, buf_main);
        for (int l = li; l < lj; ++l) {
          pack_blocks<P>(seq[l], 0, layer_shape(seq[l], width()).mb, blob.data() + at);
          at += blocks_bytes<P>(seq[l], layer_shape(seq[l], width()).mb);
        }
        li = lj;
      }
      return;
    }
    for (int li = 0; li < nl; ++li) {
      const LayerShape sh = layer_shape(seq[li], width());
      const int lu = (seq[li] == LY_L5 && l5_umb > 0) ? l5_umb : umb;
      for (int mb0 = 0; mb0 < sh.mb; mb0 += lu) {
        const int group = sh.mb - mb0 < lu ? sh.mb - mb0 : lu;
        if (res && layer_resident(fine, seq[li])) {
          const size_t at = res->size();
          res->resize(at + blocks_bytes<P>(seq[li], group), 0);
          target(*res, buf_res);
          pack_blocks<P>(seq[li], mb0, group, res->data() + at);
          continue;
        }
        const uint32_t bytes = unit_bytes<P>(sh.slots, group, P::kM16 && half_block(seq[li]));
        const uint32_t off = uint32_t(blob.size());
        blob.resize(off + bytes, 0);
        tab.push_back(off);
        tab.push_back(bytes);
        target(blob, buf_main);
        pack_blocks<P>(seq[li], mb0, group, blob.data() + off);
      }
    }
    if (res) res->resize(align_piece(uint32_t(res->size())), 0);
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

}  // namespace

__global__ void range_fetch_kernel(int* flag) { flag[1] = atomicExch(flag, 0); }

extern "C" int dfn_nerfh_set_render_options(dfn_nerfh_t h, int flags) {
  if (!h) return set_error(DFN_ERR_ARG, "dfn_nerfh_set_render_options: null handle");
  if (flags & ~(DFN_RENDER_LINDISP | DFN_RENDER_COARSE_F16)) return set_error(DFN_ERR_UNSUPPORTED, "dfn_nerfh_set_render_options: unknown option bits 0x%x", flags);
  h->render_flags = flags;
  return DFN_OK;
}

extern "C" int dfn_nerfh_range_status(dfn_nerfh_t h, int* flags, void* stream) {
  if (!h) return set_error(DFN_ERR_ARG, "dfn_nerfh_range_status: null handle");
  int v = 0;
  if (h->range_flag) {
    // read-and-clear in ONE atomic exchange on the device: bits raised by kernels of another stream between a copy and a
    // separate clear would be lost
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(range_fetch_kernel, dim3(1), dim3(1), 0, s, h->range_flag);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&v, h->range_flag + 1, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
      return set_error(DFN_ERR_HIP, "dfn_nerfh_range_status: reading the flag failed");
  }
  if (flags) { *flags = v; return DFN_OK; }
  if (v)
    return set_error(DFN_ERR_RANGE, "NeRF-H render: activations left the range of the %s arithmetic since the last check (%s); the frames rendered "
                     "since then are not the network's output: render them with DFN_PREC_F32",
                     (v & DFN_RANGE_F16_OVERFLOW) ? "f16" : "split-f16",
                     (v & DFN_RANGE_F16_OVERFLOW) ? "an f16 layer output overflowed to inf: |activation| > 65504"
                                                  : "a split-f16 hi half saturated: |activation| >= 4094 (hidden layers of the render kernels: "
                                                    ">= 4094 x the network's largest |weight|, the accumulators are narrowed before they are scaled)");
  return DFN_OK;
}

extern "C" int dfn_nerfh_range_status_async(dfn_nerfh_t h, int* host_flags, void* stream) {
  if (!h || !host_flags) return set_error(DFN_ERR_ARG, "dfn_nerfh_range_status_async: null handle / destination");
  if (!h->range_flag) { *host_flags = 0; return DFN_OK; }
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(range_fetch_kernel, dim3(1), dim3(1), 0, s, h->range_flag);   // read-and-clear, as dfn_nerfh_range_status
  if (hipGetLastError() != hipSuccess || hipMemcpyAsync(host_flags, h->range_flag + 1, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess)
    return set_error(DFN_ERR_HIP, "dfn_nerfh_range_status_async: enqueueing the read failed");
  return DFN_OK;
}

namespace {
enum { FIELD_BLOB = 0, FIELD_RES = 1, FIELD_EXTRA = 2, FIELD_GEN = 3 };
const char* const kPrecNames[3] = {"f16", "f32", "f16x3"};

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
    return device ? upload(tab.data(), tab.size() * 4, reinterpret_cast<void**>(&n.tab)) : int(DFN_OK);
  }
  void publish() {   // device mode: the handle's buffer list
    h->bufs.clear();
    for (size_t i = 0; i < shapes.size(); ++i) h->bufs.push_back(PackedBufInfo{shapes[i].name, ptrs[i], shapes[i].bytes, shapes[i].net, shapes[i].scale});
  }
};

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
  std::vector<float> fold_bd, fold_bt;   // netwidth 128: W_dir[:, :W] b_final, W_tr[:, :W] b_final (fold_final)
  std::vector<float> cfold_bd;           // netwidth 128: the coarse network's W_dir[:, :W] b_final (the training query's folded kernel)
  auto net_name = [](int f, int prec, int var) { return std::string("net.") + (f ? "fine." : "coarse.") + kPrecNames[prec] + ".v" + std::to_string(var); };
  auto weight_max = [&](const std::string& pre) {
    float wmax = 0.f;
    for (const auto& kv : h->params)
      if (kv.first.compare(0, pre.size(), pre) == 0 && kv.first.find(".weight") != std::string::npos)
        for (float v : kv.second) wmax = std::fmax(wmax, std::fabs(v));
    return wmax;
  };
  if (Wd != kWidth && Wd != kMaxWidth) return DFN_OK;   // generic-width path only
  if (Wd == kMaxWidth) {   // netwidth 256: one kernel variant per precision, plain staging units (nerfh_mlp.hip: launch_mlp)
    for (int f = 0; f < 2; ++f)
      for (int prec = 0; prec < 3; ++prec) {
        Packer pk{h, f ? "fine." : "coarse."};
        pk.plan = plan;
        pk.buf_main = sink.reserve();
        std::vector<uint8_t> blob;
        std::vector<uint32_t> tab;
        PackedNet& n = h->net[f][prec][0];
        if (prec == DFN_PREC_F16) pk.pack<PrecF16>(f, unit_mb_w256<PrecF16>(), false, blob, tab);
        else if (prec == DFN_PREC_F32) pk.pack<PrecF32>(f, unit_mb_w256<PrecF32>(), false, blob, tab);
        else {
          pk.wscale = recommit::weight_scale(weight_max(pk.pre));
          n.in_scale = pk.wscale * kX3ActScale;
          pk.pack<PrecX3>(f, unit_mb_w256<PrecX3>(), false, blob, tab);
        }
        if (int rc = sink.put_net(pk.buf_main, net_name(f, prec, 0), n, prec == DFN_PREC_F16X3 ? f : -1, blob, tab)) return rc;
      }
    // the coarse network's training query (dfn_mlp_coarse_static_points), forward only: the plain sequence in the staging units and at
    // the weight scale of net[0][prec][0].  1 245 184 B (f16, 40 units), 2 488 320 B (fp32, 78 units), 2 488 320 B (split-f16, 78 units)
    for (int prec = 0; prec < 3; ++prec) {
      Packer pk{h, "coarse."};
      pk.plan = plan;
      pk.buf_main = sink.reserve();
      std::vector<uint8_t> blob;
      std::vector<uint32_t> tab;
      PackedNet& n = h->cstatic[prec];
      if (prec == DFN_PREC_F16) pk.pack<PrecF16>(false, unit_mb_w256<PrecF16>(), false, blob, tab, -1, false, nullptr, true);
      else if (prec == DFN_PREC_F32) pk.pack<PrecF32>(false, unit_mb_w256<PrecF32>(), false, blob, tab, -1, false, nullptr, true);
      else {
        n.in_scale = h->net[0][prec][0].in_scale;
        pk.wscale = n.in_scale / kX3ActScale;
        pk.pack<PrecX3>(false, unit_mb_w256<PrecX3>(), false, blob, tab, -1, false, nullptr, true);
      }
      if (int rc = sink.put_net(pk.buf_main, std::string("cstatic.") + kPrecNames[prec], n, prec == DFN_PREC_F16X3 ? 0 : -1, blob, tab)) return rc;
    }
  } else {
  for (int f = 0; f < 2; ++f)
    for (int prec = 0; prec < 3; ++prec)
      for (int var = 0; var < kVariants; ++var) {
        // A variant with kernels of its own (kVariantFacts: base != var) packs the split-f16 networks they read and nothing else: the
        // fine one from the fold on, the coarse one from the half-height heads on; the rest of it is its base's (nerfh_route.h).
        // Half heads: also h->half_maps, the folded fine network with transient_beta's half (the maps flavour; variant 7 reads variant
        // 6's).  Resident: the resident layers leave the unit table for a blob of their own (res_blob).
        const VariantFacts vf = kVariantFacts[var];
        const bool resident = vf.resident, half = vf.half, fold = vf.fold && f == 1;
        if (vf.base != var && !(prec == DFN_PREC_F16X3 && (f == 1 ? vf.fold : vf.half))) continue;
        Packer pk{h, f ? "fine." : "coarse."};
        pk.plan = plan;
        const int own_buf = pk.buf_main = sink.reserve();
        if (resident) pk.buf_res = sink.reserve();
        pk.half_heads = half;
        pk.half_thead = half;
        std::vector<uint8_t> blob, rblob;
        std::vector<uint8_t>* res = resident ? &rblob : nullptr;
        std::vector<uint32_t> tab;
        PackedNet& n = h->net[f][prec][var];
        if (prec == DFN_PREC_F16) pk.pack<PrecF16>(f, unit_mb<PrecF16>(var), unit_mb<PrecF16>(var) >= 8, blob, tab);
        else if (prec == DFN_PREC_F32) pk.pack<PrecF32>(f, unit_mb<PrecF32>(var), false, blob, tab);
        else {
          // one power-of-two weight scale per network: the largest |w| lands in (0.5, 1].  The lo halves of most weights are then f16
          // subnormals — still exact to 2^-24 of the largest weight (the matrix cores do not flush f16 denormals), which is fp32's
          // resolution — and the accumulators (in_scale x the value = 16 x value / max|w|) fit f16 up to |value| = 4094 max|w|: that is
          // what lets the render kernels narrow BEFORE they scale (X3Piece: one packed multiply per result pair instead of two)
          pk.wscale = recommit::weight_scale(weight_max(pk.pre));
          n.in_scale = pk.wscale * kX3ActScale;
          if (fold) {
            // the folded matrices stay out of the scan above: wscale is what every other layer's operands were scaled for.  Their
            // entries may exceed the largest weight (sums of W products); as hi + lo f16 pairs of w x wscale that is harmless.
            const int ldd = Wd + kChDir + h->desc.hist_bin * h->desc.dim_a, ldt = Wd + h->desc.hist_bin * h->desc.dim_t;
            const auto& F = h->params.at("fine.xyz_encoding_final.weight");
            const auto& bF = h->params.at("fine.xyz_encoding_final.bias");
            fold_final(h->params.at("fine.dir_encoding.0.weight"), Wd / 2, ldd, F, bF, Wd, pk.fold_dir, fold_bd);
            fold_final(h->params.at("fine.transient_encoding.0.weight"), Wd / 2, ldt, F, bF, Wd, pk.fold_tr, fold_bt);
            pk.fold_dir_id = np + 0;
            pk.fold_tr_id = np + 1;
            pk.pack<PrecX3M16>(f, unit_mb<PrecX3M16>(var), false, blob, tab, l5_unit_mb_p<PrecX3M16>(unit_mb<PrecX3M16>(var)), true, res);
            if (half && !resident) {   // the maps flavour's network: the transient head at full height
              std::vector<uint8_t> mblob;
              std::vector<uint32_t> mtab;
              pk.half_thead = false;
              pk.buf_main = sink.reserve();
              pk.pack<PrecX3M16>(f, unit_mb<PrecX3M16>(var), false, mblob, mtab, l5_unit_mb_p<PrecX3M16>(unit_mb<PrecX3M16>(var)), true);
              PackedNet& m = h->half_maps;
              m.in_scale = n.in_scale;
              if (int rc = sink.put_net(pk.buf_main, "half_maps", m, 1, mblob, mtab)) return rc;
              pk.buf_main = own_buf;
            }
          } else if (vf.base == 4) pk.pack<PrecX3M16>(f, unit_mb<PrecX3M16>(var), false, blob, tab, l5_unit_mb_p<PrecX3M16>(unit_mb<PrecX3M16>(var)), false, res);
          else pk.pack<PrecX3>(f, unit_mb<PrecX3>(var), false, blob, tab, l5_unit_mb_p<PrecX3>(unit_mb<PrecX3>(var)));
        }
        const int scale = prec == DFN_PREC_F16X3 ? f : -1;
        if (int rc = sink.put_net(pk.buf_main, net_name(f, prec, var), n, scale, blob, tab)) return rc;
        if (resident) {
          if (rblob.size() != resident_bytes<PrecX3M16>(f != 0))
            return set_error(DFN_ERR_STATE, "dfn_nerfh_commit: the resident layers pack to %zu bytes, the kernels expect %u", rblob.size(),
                             resident_bytes<PrecX3M16>(f != 0));
          if (int rc = sink.put(pk.buf_res, net_name(f, prec, var) + ".res", &n, FIELD_RES, scale, rblob.data(), rblob.size())) return rc;
          n.res_bytes = uint32_t(rblob.size());
        }
      }
  for (int prec = 0; prec < 3; ++prec) {
    Packer pk{h, "fine."};
    pk.plan = plan;
    pk.buf_main = sink.reserve();
    std::vector<uint8_t> blob;
    std::vector<uint32_t> tab;
    PackedNet& n = h->bwd[prec];
    if (prec == DFN_PREC_F16) pk.pack_bwd<PrecF16, PrecF16>(blob, tab);
    else if (prec == DFN_PREC_F32) pk.pack_bwd<PrecF32, PrecF32>(blob, tab);
    else {
      // the gradient kernels scale their accumulators in fp32 BEFORE narrowing them (store_hidden), so their weights can sit where
      // every lo half is a normal f16 (largest |w| near 2^10: 22 bits per weight) instead of at the render kernels' unit scale
      n.in_scale = h->net[1][2][0].in_scale * 1024.f;
      pk.wscale = n.in_scale / kX3ActScale;
      pk.pack_bwd<PrecX3, PrecX3>(blob, tab);
    }
    if (int rc = sink.put_net(pk.buf_main, std::string("bwd.") + kPrecNames[prec], n, prec == DFN_PREC_F16X3 ? 3 : -1, blob, tab)) return rc;
    n.n_fwd_units = pk.fwd_units;
  }
  // the coarse network's gradient blob (dfn_mlp_coarse_points_backward): exact fp32 and split-f16, the latter at the fine gradient
  // blob's weight scale rule.  Two buffers per precision (blob, unit table): 1 152 000 B + 552 B (fp32: 33 + 36 units) and 1 117 184 B +
  // 280 B (split-f16: 17 + 18 units), 2.27 MB per handle in all.
  for (int prec : {int(DFN_PREC_F32), int(DFN_PREC_F16X3)}) {
    Packer pk{h, "coarse."};
    pk.plan = plan;
    pk.buf_main = sink.reserve();
    std::vector<uint8_t> blob;
    std::vector<uint32_t> tab;
    PackedNet& n = h->bwd_coarse[prec];
    if (prec == DFN_PREC_F32) pk.pack_bwd<PrecF32, PrecF32>(blob, tab, true);
    else {
      n.in_scale = h->net[0][2][0].in_scale * 1024.f;
      pk.wscale = n.in_scale / kX3ActScale;
      pk.pack_bwd<PrecX3, PrecX3>(blob, tab, true);
    }
    if (int rc = sink.put_net(pk.buf_main, std::string("bwd_coarse.") + kPrecNames[prec], n, prec == DFN_PREC_F16X3 ? 2 : -1, blob, tab)) return rc;
    n.n_fwd_units = pk.fwd_units;
  }
  // the coarse network's training query (dfn_mlp_coarse_static_points): the coarse weights along kCoarseStaticSeq in the staging units
  // of the fine point query's kernels (f16: merged, variant 0's; exact fp32: one M-block; split-f16: PrecX3M16 along
  // kCoarseStaticFoldSeq, two M-blocks, layer 5 in one-M-block units) at the coarse network's weight scale.  Two buffers per precision
  // (blob, unit table): 334 848 B + 88 B (f16, 11 units), 688 128 B + 320 B (fp32, 40 units), 603 136 B + 168 B (split-f16, 21 units).
  for (int prec = 0; prec < 3; ++prec) {
    Packer pk{h, "coarse."};
    pk.plan = plan;
    pk.buf_main = sink.reserve();
    std::vector<uint8_t> blob;
    std::vector<uint32_t> tab;
    PackedNet& n = h->cstatic[prec];
    if (prec == DFN_PREC_F16) pk.pack<PrecF16>(false, unit_mb<PrecF16>(0), true, blob, tab, -1, false, nullptr, true);
    else if (prec == DFN_PREC_F32) pk.pack<PrecF32>(false, unit_mb<PrecF32>(0), false, blob, tab, -1, false, nullptr, true);
    else {
      n.in_scale = h->net[0][prec][0].in_scale;   // the scan over the "coarse." weights: every coarse network's
      pk.wscale = n.in_scale / kX3ActScale;
      fold_final(h->params.at("coarse.dir_encoding.0.weight"), Wd / 2, Wd + kChDir, h->params.at("coarse.xyz_encoding_final.weight"),
                 h->params.at("coarse.xyz_encoding_final.bias"), Wd, pk.fold_dir, cfold_bd);
      pk.fold_dir_id = np + 2;
      constexpr int umb = unit_mb<PrecX3M16>(kFoldVariant);
      pk.pack<PrecX3M16>(false, umb, false, blob, tab, l5_unit_mb_p<PrecX3M16>(umb), true, nullptr, true);
    }
    if (int rc = sink.put_net(pk.buf_main, std::string("cstatic.") + kPrecNames[prec], n, prec == DFN_PREC_F16X3 ? 0 : -1, blob, tab)) return rc;
  }
  // ... and its gradient blob (dfn_mlp_coarse_static_points_backward): the plain forward sequence followed by kBwdCoarseStaticSeq, exact
  // fp32 and split-f16 at the gradient blobs' weight scale rule.  1 387 520 B + 664 B (fp32: 40 + 43 units) and 1 346 560 B + 344 B
  // (split-f16: 21 + 22 units), 2.73 MB per handle; with the three forward networks above 4.36 MB in all.
  for (int prec : {int(DFN_PREC_F32), int(DFN_PREC_F16X3)}) {
    Packer pk{h, "coarse."};
    pk.plan = plan;
    pk.buf_main = sink.reserve();
    std::vector<uint8_t> blob;
    std::vector<uint32_t> tab;
    PackedNet& n = h->bwd_cstatic[prec];
    if (prec == DFN_PREC_F32) pk.pack_bwd<PrecF32, PrecF32>(blob, tab, true, true);
    else {
      n.in_scale = h->net[0][2][0].in_scale * 1024.f;
      pk.wscale = n.in_scale / kX3ActScale;
      pk.pack_bwd<PrecX3, PrecX3>(blob, tab, true, true);
    }
    if (int rc = sink.put_net(pk.buf_main, std::string("bwd_cstatic.") + kPrecNames[prec], n, prec == DFN_PREC_F16X3 ? 2 : -1, blob, tab)) return rc;
    n.n_fwd_units = pk.fwd_units;
  }
  }   // netwidth 128
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
    if (fold_bd.empty()) put_extra(o_bdf + f, bd[f], i_bd, f);
    else put_extra(o_bdf + f, bd[f] + fold_bd[f], np + 3, f);
    if (fold_bt.empty()) put_extra(o_btf + f, bt[f], i_bt, f);
    else put_extra(o_btf + f, bt[f] + fold_bt[f], np + 4, f);
  }
  {  // the coarse dir_encoding.0 [W/2, W + 27]: its 27 direction columns transposed, its bias, and the bias of the folded kernel
    const auto& cwd = h->params.at("coarse.dir_encoding.0.weight");
    const auto& cbd = h->params.at("coarse.dir_encoding.0.bias");
    for (int j = 0; j < kChDir; ++j)
      for (int f = 0; f < NO; ++f)
        put_extra(o_cwd + size_t(j) * NO + f, cwd[size_t(f) * (Wd + kChDir) + Wd + j], i_cwd, size_t(f) * (Wd + kChDir) + Wd + j);
    for (int f = 0; f < NO; ++f) {
      put_extra(o_cbd + f, cbd[f], i_cbd, f);
      if (cfold_bd.empty()) put_extra(o_cbdf + f, cbd[f], i_cbd, f);
      else put_extra(o_cbdf + f, cbd[f] + cfold_bd[f], np + 5, f);
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
  if (!h->tile_counter) {   // kernel variant 8: the tile heads of the coarse and the fine kernel (zeroed in front of every pass that claims from them)
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
  return set_error(DFN_OK, "netwidth %d: %zu buffers of %zu bytes; plan of %zu entries (%zu bytes) and %zu segments; %zu bytes written per re-commit",
                   width, sa.shapes.size(), total, plan.elems.size(), plan.elems.size() * sizeof(PlanElem), plan.copies.size(), written);
}

// ------------------------------------------------------------------------------------------ profiling aid
namespace {
struct KernelTimer {
  bool on = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[DFN_PROF_SLOTS];
} g_prof;
struct ScopedTimer {
  int which;
  hipStream_t s;
  hipEvent_t a = nullptr, b = nullptr;
  ScopedTimer(int w, hipStream_t st) : which(w), s(st) {
    if (!g_prof.on) return;
    (void)hipEventCreate(&a);
    (void)hipEventCreate(&b);
    (void)hipEventRecord(a, s);
  }
  ~ScopedTimer() {
    if (!a) return;
    (void)hipEventRecord(b, s);
    g_prof.ev[which].emplace_back(a, b);
  }
};
}  // namespace

extern "C" int dfn_profile_enable(int on) {
  for (auto& v : g_prof.ev) {
    for (auto& p : v) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
    v.clear();
  }
  g_prof.on = on != 0;
  return DFN_OK;
}
extern "C" int dfn_profile_read(int which, double* avg_ms, int* launches) {
  if (which < 0 || which >= DFN_PROF_SLOTS || !avg_ms || !launches) return set_error(DFN_ERR_ARG, "dfn_profile_read: bad argument");
  double tot = 0;
  for (auto& p : g_prof.ev[which]) {
    float ms = 0;
    if (hipEventSynchronize(p.second) != hipSuccess || hipEventElapsedTime(&ms, p.first, p.second) != hipSuccess)
      return set_error(DFN_ERR_HIP, "dfn_profile_read: event query failed");
    tot += ms;
  }
  *launches = int(g_prof.ev[which].size());
  *avg_ms = *launches ? tot / *launches : 0.0;
  return DFN_OK;
}

// ------------------------------------------------------------------------------------------ stage entry points
#define HS(s) reinterpret_cast<hipStream_t>(s)
#define CHECK_HIP(expr, what)                                                                   \
  do {                                                                                          \
    hipError_t e_ = (expr);                                                                     \
    if (e_ != hipSuccess) return set_error(DFN_ERR_HIP, "%s: %s", what, hipGetErrorString(e_)); \
  } while (0)

static int check_net(dfn_nerfh_t h, int prec, const char* fn, bool allow_x3 = false) {
  if (!h) return set_error(DFN_ERR_ARG, "%s: null handle", fn);
  if (!h->committed) return set_error(DFN_ERR_STATE, "%s: dfn_nerfh_commit() has not been called", fn);
  if (!h->fast)
    return set_error(DFN_ERR_UNSUPPORTED, "%s: the register-resident kernels exist for netwidth %d and %d (this handle: %d); "
                     "use the generic-width entry points (dfn_nerfh_generic_*)", fn, kWidth, kMaxWidth, h->desc.width);
  if (prec != DFN_PREC_F16 && prec != DFN_PREC_F32 && !(allow_x3 && prec == DFN_PREC_F16X3))
    return set_error(DFN_ERR_ARG, "%s: unknown / unsupported precision %d", fn, prec);
  return DFN_OK;
}

// Gradient entry points: fp32-grade arithmetic only (DFN_PREC_F32, DFN_PREC_F16X3).
static int check_grad_width(dfn_nerfh_t h, const char* fn) {
  if (h->desc.width != kWidth)
    return set_error(DFN_ERR_UNSUPPORTED, "%s: the input-gradient kernels are built for netwidth %d only (this handle: %d)", fn, kWidth,
                     h->desc.width);
  return DFN_OK;
}
static int check_grad_prec(int prec, const char* fn) {
  if (prec == DFN_PREC_F16)
    return set_error(DFN_ERR_UNSUPPORTED, "%s: gradients run in DFN_PREC_F16X3 or DFN_PREC_F32 only (plain-f16 ReLU gates are 3e-2 off "
                     "autograd)", fn);
  return DFN_OK;
}

// The handle's range-guard flag (device int): allocated and cleared by dfn_nerfh_commit, which fails loudly when it cannot be —
// every kernel launch that carries the guard runs on a committed handle.
static int* range_flag_of(dfn_nerfh_t h) { return h->range_flag; }

// Kernel variant: DFN_MLP_VARIANT=0..10 (A/B aid; nerfh_layout.h: kVariantFacts, kSelectedByDefault), read once.  What it means for a call
// is nerfh_route.h; the gradient paths (render backward, dfn_mlp_fine_saving) run the base variant's / variant 0's plain kernels on
// the plain table, which their backward kernels read.
static int mlp_variant_128() {
  static int v = -1;
  if (v < 0) {
    const char* e = getenv("DFN_MLP_VARIANT");
    char* end = nullptr;
    const long n = e ? strtol(e, &end, 10) : -1;   // whole decimal numbers only; anything else selects the default
    v = (e && end != e && *end == '\0' && n >= 0 && n <= kLastVariant) ? int(n) : kSelectedByDefault;
  }
  return v;
}
static const PackedNet& route_net(dfn_nerfh_t h, bool fine, int prec, const Route& r) {
  return r.net == kNetHalfMaps ? h->half_maps : h->net[fine][prec][r.net];
}
// A route's launch.  a: the call's arguments over route_net(h, fine, prec, r); the resident blob and the tile counter (coarse [0],
// fine [1]; zero_tile_counters in front of the pass) ride behind them for the two launchers that take them.
static hipError_t launch_route(dfn_nerfh_t h, bool fine, int prec, const Route& r, const MlpArgs& a, hipStream_t s) {
  const int cus = device_cu_count(), width = h->desc.width;
  const PackedNet& n = route_net(h, fine, prec, r);
  MlpDynArgs d{};
  static_cast<MlpArgs&>(d) = a;
  d.res_blob = n.res_blob;
  d.res_bytes = n.res_bytes;
  d.tile_counter = h->tile_counter + (fine ? 1 : 0);
  switch (r.launcher) {
    case kLaunchPlain: return launch_mlp(fine, prec, r.variant, a, cus, s, width);
    case kLaunchMaps: return launch_mlp_maps(fine, prec, r.variant, a, cus, s, width);
    case kLaunchFold: return launch_mlp_fold(r.maps, a, cus, s);
    case kLaunchHalf: return launch_mlp_half(fine, r.maps, a, cus, s);
    case kLaunchResident: return launch_mlp_res(fine, d, cus, s);
    case kLaunchClaimed: return launch_mlp_dyn(fine, d, cus, s);
    case kLaunchKept: return launch_mlp_pe(fine, d, cus, s);
    case kLaunchHoisted: return launch_mlp_hoist(fine, d, cus, s);
    case kLaunchPoints: return launch_mlp_pts(fine, prec, a, cus, s, width);
    case kLaunchPointsFold: return launch_mlp_pts_fold(a, cus, s);
    case kLaunchPointsHalf: return launch_mlp_pts_half(a, cus, s);
  }
  return hipErrorInvalidValue;
}
static hipError_t zero_tile_counters(dfn_nerfh_t h, hipStream_t s) { return hipMemsetAsync(h->tile_counter, 0, 2 * sizeof(uint32_t), s); }

static unsigned long long* g_timing_buf = nullptr;  // DFN_TIMING builds only (tools/gpu_timing.py)
extern "C" void dfn_debug_set_timing_buffer(void* p) { g_timing_buf = static_cast<unsigned long long*>(p); }


extern "C" int dfn_raygen(int H, int W, float focal, const float* c2w, float* rays_o, float* rays_d,
                          float* viewdirs, void* stream) {
  if (H < 0 || W < 0 || !c2w || !rays_o || !rays_d || !(focal > 0)) return set_error(DFN_ERR_ARG, "dfn_raygen: bad argument");
  CHECK_HIP(launch_raygen(H, W, focal, c2w, rays_o, rays_d, viewdirs, HS(stream)), "dfn_raygen");
  return DFN_OK;
}

extern "C" int dfn_posenc(const float* x, size_t n, int L, int mode, float* out, void* stream) {
  if (!x || !out || L < 0 || L > 16 || (mode != 0 && mode != 1)) return set_error(DFN_ERR_ARG, "dfn_posenc: bad argument");
  CHECK_HIP(launch_posenc(x, n, L, mode, out, HS(stream)), "dfn_posenc");
  return DFN_OK;
}

extern "C" int dfn_mlp_coarse(dfn_nerfh_t h, int prec, const float* rays_o, const float* rays_d, size_t n_rays,
                              int Nc, float near, float far, float* sigma, void* stream) {
  if (int rc = check_net(h, prec, "dfn_mlp_coarse", true)) return rc;
  if (!n_rays) return DFN_OK;
  if (!rays_o || !rays_d || !sigma || Nc < 1) return set_error(DFN_ERR_ARG, "dfn_mlp_coarse: bad argument");
  const Route r = coarse_route(mlp_variant_128(), h->desc.width, prec);
  const PackedNet& n = route_net(h, false, prec, r);
  MlpArgs a{n.blob, n.tab, n.n_units, rays_o, rays_d, nullptr, nullptr, sigma, nullptr, (long long)n_rays, Nc, near, far, nullptr, n.in_scale,
            h->render_flags & DFN_RENDER_LINDISP};
  a.status = range_flag_of(h);
  if (claims_tiles(r.launcher)) CHECK_HIP(zero_tile_counters(h, HS(stream)), "dfn_mlp_coarse(tile counters)");
  ScopedTimer t(0, HS(stream));
  CHECK_HIP(launch_route(h, false, prec, r, a, HS(stream)), "dfn_mlp_coarse");
  return DFN_OK;
}

extern "C" int dfn_coarse_weights(const float* sigma, const float* z, size_t n, int N, float* weights, void* stream) {
  if (!sigma || !z || !weights || N < 1 || N > 2048) return set_error(DFN_ERR_ARG, "dfn_coarse_weights: bad argument");
  CHECK_HIP(launch_coarse_weights(sigma, z, n, N, weights, HS(stream)), "dfn_coarse_weights");
  return DFN_OK;
}

extern "C" int dfn_sample_pdf(const float* bins, const float* weights, size_t n, int nb, int Ni, const float* u,
                              float* out, void* stream) {
  if (!bins || !weights || !out || nb < 2 || Ni < 1 || 3 * nb + 2 * Ni > 8192)
    return set_error(DFN_ERR_ARG, "dfn_sample_pdf: bad argument");
  CHECK_HIP(launch_sample_pdf(bins, weights, n, nb, Ni, u, out, HS(stream)), "dfn_sample_pdf");
  return DFN_OK;
}

extern "C" int dfn_sample_pdf_backward(const float* bins, const float* weights, size_t n, int nb, int Ni, const float* u,
                                       const float* grad_out, float* grad_bins, float* grad_weights, float* grad_u, void* stream) {
  if (!bins || !weights || !grad_out) return set_error(DFN_ERR_ARG, "dfn_sample_pdf_backward: bad argument (bins, weights or grad_out NULL)");
  if (nb < 2 || Ni < 1) return set_error(DFN_ERR_ARG, "dfn_sample_pdf_backward: bad argument (need nb >= 2 and Ni >= 1, got %d and %d)", nb, Ni);
  if (!grad_bins && !grad_weights && !grad_u)
    return set_error(DFN_ERR_ARG, "dfn_sample_pdf_backward: bad argument (grad_bins, grad_weights and grad_u all NULL)");
  if (grad_u && !u) return set_error(DFN_ERR_ARG, "dfn_sample_pdf_backward: bad argument (grad_u without u: the linspace draws are constants)");
  if (sample_pdf_backward_lds_bytes(nb, Ni) > kSamplePdfBackwardMaxLds)
    return set_error(DFN_ERR_UNSUPPORTED, "dfn_sample_pdf_backward: nb = %d, Ni = %d need %zu bytes of LDS per block, the kernel has %zu", nb, Ni,
                     sample_pdf_backward_lds_bytes(nb, Ni), kSamplePdfBackwardMaxLds);
  if (!n) return DFN_OK;
  CHECK_HIP(launch_sample_pdf_backward(bins, weights, n, nb, Ni, u, grad_out, grad_bins, grad_weights, grad_u, HS(stream)),
            "dfn_sample_pdf_backward");
  return DFN_OK;
}

extern "C" int dfn_sample_fine_opt(const float* sigma, size_t n_rays, int Nc, int Ni, float near, float far, int render_flags,
                                   float* z_fine, float* weights_coarse, float* z_samples, void* stream) {
  if (!sigma || !z_fine || Nc < 3 || Ni < 1 || 6 * Nc + 2 * Ni > 8192)
    return set_error(DFN_ERR_ARG, "dfn_sample_fine: bad argument (need N_samples >= 3, N_importance >= 1)");
  if ((render_flags & DFN_RENDER_LINDISP) && !(near > 0.f))
    return set_error(DFN_ERR_ARG, "dfn_sample_fine: lindisp needs near > 0");
  CHECK_HIP(launch_sample_fine(sigma, n_rays, Nc, Ni, near, far, z_fine, weights_coarse, z_samples, HS(stream),
                               render_flags & DFN_RENDER_LINDISP),
            "dfn_sample_fine");
  return DFN_OK;
}
extern "C" int dfn_sample_fine(const float* sigma, size_t n_rays, int Nc, int Ni, float near, float far,
                               float* z_fine, float* weights_coarse, float* z_samples, void* stream) {
  return dfn_sample_fine_opt(sigma, n_rays, Nc, Ni, near, far, 0, z_fine, weights_coarse, z_samples, stream);
}

extern "C" int dfn_ndc_rays(int H, int W, float focal, float near, const float* rays_o, const float* rays_d, size_t n, float* out_o,
                            float* out_d, void* stream) {
  if (!n) return DFN_OK;
  if (!rays_o || !rays_d || !out_o || !out_d || H < 1 || W < 1 || !(focal > 0.f)) return set_error(DFN_ERR_ARG, "dfn_ndc_rays: bad argument");
  CHECK_HIP(launch_ndc_rays(H, W, focal, near, rays_o, rays_d, n, out_o, out_d, HS(stream)), "dfn_ndc_rays");
  return DFN_OK;
}

extern "C" int dfn_upsample_bicubic(const float* in, int H, int W, int C, int outH, int outW, float* out, void* stream) {
  if (!in || !out || H < 1 || W < 1 || C < 1 || outH < 1 || outW < 1) return set_error(DFN_ERR_ARG, "dfn_upsample_bicubic: bad argument");
  CHECK_HIP(launch_bicubic(in, H, W, C, outH, outW, out, HS(stream)), "dfn_upsample_bicubic");
  return DFN_OK;
}

extern "C" int dfn_upsample_bicubic_frames(const float* in, int B, int H, int W, int C, int outH, int outW, int out_nchw, float* out,
                                           void* stream) {
  if (!in || !out || B < 1 || H < 1 || W < 1 || C < 1 || outH < 1 || outW < 1) return set_error(DFN_ERR_ARG, "dfn_upsample_bicubic_frames: bad argument");
  CHECK_HIP(launch_bicubic(in, H, W, C, outH, outW, out, HS(stream), B, out_nchw != 0), "dfn_upsample_bicubic_frames");
  return DFN_OK;
}
extern "C" int dfn_upsample_bicubic_frames_backward(const float* grad_out, int B, int H, int W, int C, int outH, int outW, int out_nchw,
                                                    float* grad_in, void* stream) {
  if (!grad_out || !grad_in || B < 1 || H < 1 || W < 1 || C < 1 || outH < 1 || outW < 1)
    return set_error(DFN_ERR_ARG, "dfn_upsample_bicubic_frames_backward: bad argument");
  CHECK_HIP(launch_bicubic_backward(grad_out, H, W, C, outH, outW, grad_in, HS(stream), B, out_nchw != 0), "dfn_upsample_bicubic_frames_backward");
  return DFN_OK;
}

extern "C" int dfn_upsample_bicubic_backward(const float* grad_out, int H, int W, int C, int outH, int outW, float* grad_in,
                                             void* stream) {
  if (!grad_out || !grad_in || H < 1 || W < 1 || C < 1 || outH < 1 || outW < 1)
    return set_error(DFN_ERR_ARG, "dfn_upsample_bicubic_backward: bad argument");
  CHECK_HIP(launch_bicubic_backward(grad_out, H, W, C, outH, outW, grad_in, HS(stream)), "dfn_upsample_bicubic_backward");
  return DFN_OK;
}

extern "C" size_t dfn_fine_bias_bytes(size_t n_rays) { return (n_rays ? n_rays : 1) * ray_bias_floats(kMaxWidth) * sizeof(float); }

extern "C" int dfn_mlp_fine(dfn_nerfh_t h, int prec, const float* rays_o, const float* rays_d, const float* viewdirs,
                            const float* hist, size_t hist_rows, size_t n_rays, const float* z_fine, int Nf,
                            float* raw, void* bias_ws, void* stream) {
  if (int rc = check_net(h, prec, "dfn_mlp_fine", true)) return rc;
  if (!n_rays) return DFN_OK;
  if (!rays_o || !rays_d || !viewdirs || !hist || !z_fine || !raw || !bias_ws || Nf < 1 ||
      (hist_rows != 1 && hist_rows != n_rays))
    return set_error(DFN_ERR_ARG, "dfn_mlp_fine: bad argument (hist_rows must be 1 or n_rays)");
  float* table = static_cast<float*>(bias_ws);
  const Route r = fine_route(mlp_variant_128(), h->desc.width, prec, false, false);
  CHECK_HIP(launch_ray_bias(r.fold_table ? h->rb_fold : h->rb, viewdirs, hist, hist_rows, n_rays, table, HS(stream)), "dfn_mlp_fine(ray_bias)");
  const PackedNet& n = route_net(h, true, prec, r);
  MlpArgs a{n.blob, n.tab, n.n_units, rays_o, rays_d, z_fine, table, raw, nullptr, (long long)n_rays, Nf, 0.f, 0.f, g_timing_buf, n.in_scale};
  a.status = range_flag_of(h);
  ScopedTimer t(1, HS(stream));
  CHECK_HIP(launch_route(h, true, prec, r, a, HS(stream)), "dfn_mlp_fine");
  return DFN_OK;
}

extern "C" int dfn_composite_fine(const float* raw, const float* z, size_t n_rays, int Nf, float beta_min, int flags,
                                  float* rgb, float* disp, float* acc, float* depth, float* weights, float* beta,
                                  void* stream) {
  if (!raw || !z || !rgb || !disp || !acc || Nf < 1 || Nf > 512)
    return set_error(DFN_ERR_ARG, "dfn_composite_fine: bad argument (1 <= Nf <= 512)");
  CHECK_HIP(launch_composite_fine(raw, z, n_rays, Nf, beta_min, flags, rgb, disp, acc, depth, weights, beta, HS(stream)),
            "dfn_composite_fine");
  return DFN_OK;
}

// dfn_render_maps -> the kernels' MapPtrs; nothing requested (NULL or five NULL members) = no maps at all
static MapPtrs map_ptrs(const dfn_render_maps* m) {
  return m ? MapPtrs{m->depth, m->depth_static, m->beta, m->rgb_static, m->rgb_transient} : MapPtrs{};
}

extern "C" int dfn_composite_fine_maps(const float* raw, const float* z, size_t n_rays, int Nf, float beta_min,
                                       const dfn_render_maps* maps, void* stream) {
  if (!raw || !z || Nf < 1 || Nf > 512) return set_error(DFN_ERR_ARG, "dfn_composite_fine_maps: bad argument (1 <= Nf <= 512)");
  CHECK_HIP(launch_composite_fine_maps(raw, z, n_rays, Nf, beta_min, map_ptrs(maps), HS(stream)), "dfn_composite_fine_maps");
  return DFN_OK;
}

// ------------------------------------------------------------------------------------------ whole path
namespace {
constexpr size_t kMaxChunkRays = 65536;  // rays per internal pass where raw lives in the workspace (bounds the raw buffer)
// ... and on the fused route, where raw never reaches memory and only sigma, z, the per-ray table and the segment records scale with
// the pass.  A bound of its own: 327 680 (a 640x480 frame in ONE pass; 327 680 rays x 512 samples = 1.7e8 points, inside the kernels'
// 32-bit point indices; every output bit for bit) was built and measured -0.11 ms of 52.07 per frame, inside three times the parent's
// spread (LABBOOK R16.1), for 150 MB more workspace: not a gain by the project's rule, so the bound stays the raw route's.
constexpr size_t kMaxFusedChunkRays = 65536;
inline size_t al(size_t b) { return (b + 255) & ~size_t(255); }
// Equal passes of at most max_rays rays (multiple of 64 rays so MLP tiles stay aligned).
inline size_t chunk_rays(size_t n_rays, size_t max_rays = kMaxChunkRays) {
  const size_t passes = (n_rays + max_rays - 1) / max_rays;
  const size_t c = passes ? (n_rays + passes - 1) / passes : 1;
  return (c + 63) & ~size_t(63);
}
// Whether a render call composites inside the fine kernel (nerfh_route.h), as render_core takes it; the caller carves for it.
bool fused_route(dfn_nerfh_t h, int prec, int Nf, bool want_raw) { return fused_compositing(mlp_variant_128(), h->desc.width, prec, Nf, want_raw); }
struct Workspace {
  float *o, *d, *v, *sigma, *z, *raw, *bias, *partial;
  size_t total;
  size_t chunk;   // rays per pass of this layout
};
// fused: the layout of the fused route -- passes of up to kMaxFusedChunkRays rays and no raw slot (w.raw = nullptr)
Workspace carve(char* base, size_t n_rays, int Nc, int Ni, bool own_rays, int rec_floats = 12, bool fused = false) {
  const size_t chunk = chunk_rays(n_rays, fused ? kMaxFusedChunkRays : kMaxChunkRays);
  const size_t Nf = size_t(Nc) + Ni;
  Workspace w{};
  size_t off = 0;
  auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += al(bytes); return reinterpret_cast<float*>(p); };
  w.o = take(own_rays ? n_rays * 12 : 0);
  w.d = take(own_rays ? n_rays * 12 : 0);
  w.v = take(n_rays * 12);
  w.sigma = take(chunk * Nc * 4);
  w.z = take(chunk * Nf * 4);
  w.raw = fused ? nullptr : take(chunk * Nf * 9 * 4);
  w.bias = take(chunk * ray_bias_floats(kMaxWidth) * 4);
  w.partial = take(chunk * ((Nf + 31) / 32) * rec_floats * 4);   // kMapsRecFloats per segment for the render-maps entries
  w.total = off;
  w.chunk = chunk;
  return w;
}
// What the size queries return: they take no route, so the larger of the two layouts -- a buffer of that size serves whichever
// route the call takes.
size_t workspace_bytes_any_route(size_t n_rays, int Nc, int Ni, int rec_floats) {
  const size_t a = carve(nullptr, n_rays, Nc, Ni, true, rec_floats, false).total, b = carve(nullptr, n_rays, Nc, Ni, true, rec_floats, true).total;
  return a > b ? a : b;
}

int render_core(dfn_nerfh_t h, int prec, const float* o, const float* d, const float* v, const float* hist,
                size_t hist_rows, size_t n_rays, int Nc, int Ni, float near, float far, float* rgb, float* disp,
                float* acc, float* raw_out, const Workspace& w, hipStream_t s, const MapPtrs& maps = MapPtrs{}) {
  const int Nf = Nc + Ni;
  const bool want_maps = maps.any();   // w.partial then holds kMapsRecFloats floats per segment (carve)
  const int seg = fused_segment(prec);
  const bool fused = fused_route(h, prec, Nf, raw_out != nullptr);   // the caller carved w for this route
  const int cprec = (h->render_flags & DFN_RENDER_COARSE_F16) ? DFN_PREC_F16 : prec;   // the coarse pass only places the fine samples
  const Route rc = coarse_route(mlp_variant_128(), h->desc.width, cprec), rf = fine_route(mlp_variant_128(), h->desc.width, prec, fused, want_maps);
  const PackedNet &nc = route_net(h, false, cprec, rc), &nf = route_net(h, true, prec, rf);
  const size_t chunk = w.chunk;
  for (size_t r0 = 0; r0 < n_rays; r0 += chunk) {
    const size_t n = n_rays - r0 < chunk ? n_rays - r0 : chunk;
    const float* co = o + r0 * 3;
    const float* cd = d + r0 * 3;
    const float* cv = v + r0 * 3;
    const float* ch = hist_rows == 1 ? hist : hist + r0 * h->desc.hist_bin;
    float* raw = raw_out ? raw_out + r0 * size_t(Nf) * 9 : w.raw;
    {
      MlpArgs a{nc.blob, nc.tab, nc.n_units, co, cd, nullptr, nullptr, w.sigma, nullptr, (long long)n, Nc, near, far, nullptr, nc.in_scale,
                 h->render_flags & DFN_RENDER_LINDISP};
      a.status = range_flag_of(h);
      if (claims_tiles(rc.launcher) || claims_tiles(rf.launcher)) CHECK_HIP(zero_tile_counters(h, s), "render: tile counters");
      ScopedTimer t(0, s);
      CHECK_HIP(launch_route(h, false, cprec, rc, a, s), "render: coarse MLP");
    }
    {
      ScopedTimer t(DFN_PROF_SAMPLE_FINE, s);
      CHECK_HIP(launch_sample_fine(w.sigma, n, Nc, Ni, near, far, w.z, nullptr, nullptr, s, h->render_flags & DFN_RENDER_LINDISP),
                "render: sample_fine");
    }
    {
      ScopedTimer t(DFN_PROF_RAY_BIAS, s);
      // w.bias is written for this pass's fine launch and read by nothing else: on a seed_scaled route it holds in_scale x the seeds
      CHECK_HIP(launch_ray_bias(rf.fold_table ? h->rb_fold : h->rb, cv, ch, hist_rows, n, w.bias, s, rf.seed_scaled ? nf.in_scale : 1.f),
                "render: ray_bias");
    }
    {
      MlpArgs a{nf.blob, nf.tab, nf.n_units, co, cd, w.z, w.bias, raw, fused ? w.partial : nullptr, (long long)n, Nf, 0.f, 0.f, g_timing_buf, nf.in_scale};
      a.status = range_flag_of(h);
      ScopedTimer t(1, s);
      CHECK_HIP(launch_route(h, true, prec, rf, a, s), "render: fine MLP");
    }
    if (fused && want_maps) {
      ScopedTimer t(DFN_PROF_COMBINE, s);
      CHECK_HIP(launch_composite_combine_maps(w.partial, n, Nf / seg, 0.1f, DFN_COMP_TEST_TIME | DFN_COMP_STATIC_ONLY, rgb + r0 * 3,
                                              disp + r0, acc + r0, maps.at(r0), s),
                "render: composite combine (maps)");
    } else if (fused) {
      ScopedTimer t(DFN_PROF_COMBINE, s);
      CHECK_HIP(launch_composite_combine(w.partial, n, Nf / seg, 0.1f, DFN_COMP_TEST_TIME | DFN_COMP_STATIC_ONLY, rgb + r0 * 3,
                                         disp + r0, acc + r0, s),
                "render: composite combine");
    } else {
      ScopedTimer t(DFN_PROF_COMPOSITE, s);
      CHECK_HIP(launch_composite_fine(raw, w.z, n, Nf, 0.1f, DFN_COMP_TEST_TIME | DFN_COMP_STATIC_ONLY, rgb + r0 * 3,
                                      disp + r0, acc + r0, nullptr, nullptr, nullptr, s),
                "render: composite");
      if (want_maps) CHECK_HIP(launch_composite_fine_maps(raw, w.z, n, Nf, 0.1f, maps.at(r0), s), "render: composite (maps)");
    }
  }
  return DFN_OK;
}

int check_render_args(int Nc, int Ni, const char* fn) {
  if (Nc < 3 || Ni < 1 || Nc + Ni > 512 || 6 * Nc + 2 * Ni > 8192)
    return set_error(DFN_ERR_UNSUPPORTED, "%s: need 3 <= N_samples, 1 <= N_importance, N_samples+N_importance <= 512", fn);
  return DFN_OK;
}
}  // namespace

extern "C" size_t dfn_render_workspace_bytes(size_t n_rays, int Nc, int Ni) {
  return workspace_bytes_any_route(n_rays ? n_rays : 1, Nc, Ni, 12);
}

// dfn_render_rays / dfn_render_rays_maps (`fn`: the name the messages carry; no map requested: the plain entry's launches)
static int render_rays_entry(const char* fn, dfn_nerfh_t h, int prec, const float* rays_o, const float* rays_d, const float* viewdirs,
                             const float* hist, size_t hist_rows, size_t n_rays, int Nc, int Ni, float near, float far,
                             float* rgb, float* disp, float* acc, float* raw, void* workspace, size_t workspace_bytes,
                             const MapPtrs& maps, void* stream) {
  if (int rc = check_net(h, prec, fn, true)) return rc;
  if (int rc = check_render_args(Nc, Ni, fn)) return rc;
  if (!n_rays) return DFN_OK;  // an empty batch is valid (its buffers may be null)
  if (!rays_o || !rays_d || !hist || !rgb || !disp || !acc || !workspace || (hist_rows != 1 && hist_rows != n_rays))
    return set_error(DFN_ERR_ARG, "%s: bad argument (hist_rows must be 1 or n_rays)", fn);
  const Workspace w = carve(static_cast<char*>(workspace), n_rays, Nc, Ni, true, maps.any() ? kMapsRecFloats : 12,
                            fused_route(h, prec, Nc + Ni, raw != nullptr));
  if (w.total > workspace_bytes)
    return set_error(DFN_ERR_ARG, "%s: workspace too small (%zu < %zu)", fn, workspace_bytes, w.total);
  const float* v = viewdirs;
  if (!v) {
    if (hipError_t e = launch_viewdirs(rays_d, n_rays, w.v, HS(stream)); e != hipSuccess)
      return set_error(DFN_ERR_HIP, "%s: viewdirs: %s", fn, hipGetErrorString(e));
    v = w.v;
  }
  return render_core(h, prec, rays_o, rays_d, v, hist, hist_rows, n_rays, Nc, Ni, near, far, rgb, disp, acc, raw, w,
                     HS(stream), maps);
}

static int render_image_entry(const char* fn, dfn_nerfh_t h, int prec, const float* c2w, int H, int W, float focal, float near,
                              float far, int Nc, int Ni, const float* hist, float* rgb, float* disp, float* acc,
                              void* workspace, size_t workspace_bytes, const MapPtrs& maps, void* stream) {
  if (int rc = check_net(h, prec, fn, true)) return rc;
  if (int rc = check_render_args(Nc, Ni, fn)) return rc;
  if (!c2w || !hist || !rgb || !disp || !acc || !workspace || H < 1 || W < 1 || !(focal > 0))
    return set_error(DFN_ERR_ARG, "%s: bad argument", fn);
  const size_t n_rays = size_t(H) * W;
  const Workspace w = carve(static_cast<char*>(workspace), n_rays, Nc, Ni, true, maps.any() ? kMapsRecFloats : 12,
                            fused_route(h, prec, Nc + Ni, false));
  if (w.total > workspace_bytes)
    return set_error(DFN_ERR_ARG, "%s: workspace too small (%zu < %zu)", fn, workspace_bytes, w.total);
  if (hipError_t e = launch_raygen(H, W, focal, c2w, w.o, w.d, w.v, HS(stream)); e != hipSuccess)
    return set_error(DFN_ERR_HIP, "%s: raygen: %s", fn, hipGetErrorString(e));
  return render_core(h, prec, w.o, w.d, w.v, hist, 1, n_rays, Nc, Ni, near, far, rgb, disp, acc, nullptr, w, HS(stream), maps);
}

extern "C" int dfn_render_rays(dfn_nerfh_t h, int prec, const float* rays_o, const float* rays_d, const float* viewdirs,
                               const float* hist, size_t hist_rows, size_t n_rays, int Nc, int Ni, float near, float far,
                               float* rgb, float* disp, float* acc, float* raw, void* workspace, size_t workspace_bytes,
                               void* stream) {
  return render_rays_entry("dfn_render_rays", h, prec, rays_o, rays_d, viewdirs, hist, hist_rows, n_rays, Nc, Ni, near, far, rgb, disp,
                           acc, raw, workspace, workspace_bytes, MapPtrs{}, stream);
}

extern "C" int dfn_render_image(dfn_nerfh_t h, int prec, const float* c2w, int H, int W, float focal, float near,
                                float far, int Nc, int Ni, const float* hist, float* rgb, float* disp, float* acc,
                                void* workspace, size_t workspace_bytes, void* stream) {
  return render_image_entry("dfn_render_image", h, prec, c2w, H, W, focal, near, far, Nc, Ni, hist, rgb, disp, acc, workspace,
                            workspace_bytes, MapPtrs{}, stream);
}

extern "C" size_t dfn_render_maps_workspace_bytes(size_t n_rays, int Nc, int Ni) {
  return workspace_bytes_any_route(n_rays ? n_rays : 1, Nc, Ni, kMapsRecFloats);
}

extern "C" int dfn_render_rays_maps(dfn_nerfh_t h, int prec, const float* rays_o, const float* rays_d, const float* viewdirs,
                                    const float* hist, size_t hist_rows, size_t n_rays, int Nc, int Ni, float near, float far,
                                    float* rgb, float* disp, float* acc, float* raw, void* workspace, size_t workspace_bytes,
                                    const dfn_render_maps* maps, void* stream) {
  return render_rays_entry("dfn_render_rays_maps", h, prec, rays_o, rays_d, viewdirs, hist, hist_rows, n_rays, Nc, Ni, near, far, rgb,
                           disp, acc, raw, workspace, workspace_bytes, map_ptrs(maps), stream);
}

extern "C" int dfn_render_image_maps(dfn_nerfh_t h, int prec, const float* c2w, int H, int W, float focal, float near,
                                     float far, int Nc, int Ni, const float* hist, float* rgb, float* disp, float* acc,
                                     void* workspace, size_t workspace_bytes, const dfn_render_maps* maps, void* stream) {
  return render_image_entry("dfn_render_image_maps", h, prec, c2w, H, W, focal, near, far, Nc, Ni, hist, rgb, disp, acc, workspace,
                            workspace_bytes, map_ptrs(maps), stream);
}

// ------------------------------------------------------------------------------------------ gradient path
extern "C" int dfn_composite_fine_backward(const float* raw, const float* z, const float* grad_rgb, size_t n_rays, int Nf,
                                           float* grad_raw, void* stream) {
  if (!raw || !z || !grad_rgb || !grad_raw || Nf < 1 || Nf > 512)
    return set_error(DFN_ERR_ARG, "dfn_composite_fine_backward: bad argument (1 <= Nf <= 512)");
  CHECK_HIP(launch_composite_fine_backward(raw, z, grad_rgb, n_rays, Nf, grad_raw, HS(stream)), "dfn_composite_fine_backward");
  return DFN_OK;
}

// Every output of the compositor (rgb, acc, depth, depth_static, disp, beta, rgb_static, rgb_transient): nerfh_maps_bwd.hip.
extern "C" int dfn_composite_fine_backward_maps(const float* raw, const float* z, size_t n_rays, int Nf, float beta_min,
                                                const dfn_map_grads* grads, const float* grad_raw_ext, float* grad_raw, void* stream) {
  if (!raw || !z || !grad_raw || Nf < 1 || Nf > 512)
    return set_error(DFN_ERR_ARG, "dfn_composite_fine_backward_maps: bad argument (1 <= Nf <= 512)");
  const MapGrads g = grads ? MapGrads{grads->rgb, grads->acc, grads->depth, grads->depth_static, grads->disp, grads->beta,
                                      grads->rgb_static, grads->rgb_transient}
                           : MapGrads{};
  if (!g.any() && !grad_raw_ext)
    return set_error(DFN_ERR_ARG, "dfn_composite_fine_backward_maps: bad argument (no upstream gradient and no grad_raw_ext)");
  CHECK_HIP(launch_composite_fine_backward_all(raw, z, n_rays, Nf, beta_min, g, grad_raw, HS(stream), grad_raw_ext),
            "dfn_composite_fine_backward_maps");
  return DFN_OK;
}

extern "C" int dfn_mlp_fine_backward(dfn_nerfh_t h, int prec, const float* rays_o, const float* rays_d, const float* viewdirs,
                                     const float* hist, size_t hist_rows, size_t n_rays, const float* z_fine, int Nf,
                                     const float* grad_raw, float* grad_pts, void* bias_ws, void* stream) {
  if (int rc = check_net(h, prec, "dfn_mlp_fine_backward", true)) return rc;
  if (int rc = check_grad_prec(prec, "dfn_mlp_fine_backward")) return rc;
  if (int rc = check_grad_width(h, "dfn_mlp_fine_backward")) return rc;
  if (!n_rays) return DFN_OK;
  if (!rays_o || !rays_d || !viewdirs || !hist || !z_fine || !grad_raw || !grad_pts || !bias_ws || Nf < 1 ||
      (hist_rows != 1 && hist_rows != n_rays))
    return set_error(DFN_ERR_ARG, "dfn_mlp_fine_backward: bad argument (hist_rows must be 1 or n_rays)");
  float* table = static_cast<float*>(bias_ws);
  CHECK_HIP(launch_ray_bias(h->rb, viewdirs, hist, hist_rows, n_rays, table, HS(stream)), "dfn_mlp_fine_backward(ray_bias)");
  const PackedNet& n = h->bwd[prec];
  BwdArgs a{n.blob, n.tab, n.n_units, rays_o, rays_d, viewdirs, z_fine, table, grad_raw, grad_pts, (long long)n_rays, Nf, n.in_scale};
  CHECK_HIP(launch_mlp_fine_backward(prec, a, device_cu_count(), HS(stream)), "dfn_mlp_fine_backward");
  return DFN_OK;
}

// Point queries (nerfw.py:15-95 run_network_NeRFW as network_query_fn calls it, :425-434).  The default kernel variant's kernels whatever
// DFN_MLP_VARIANT says: split-f16 at netwidth 128 = variant 6's coarse kernel and variant 5's fine kernel (the raw route of dfn_mlp_fine).
static int check_points(size_t n_rows, int N, const char* fn) {
  if (N < 1) return set_error(DFN_ERR_ARG, "%s: bad argument (N >= 1)", fn);
  if (n_rows > ((size_t(1) << 31) - 1) / size_t(N)) return set_error(DFN_ERR_ARG, "%s: n_rows * N must stay below 2^31 (chunk by rows)", fn);
  return DFN_OK;
}

extern "C" int dfn_mlp_coarse_points(dfn_nerfh_t h, int prec, const float* pts, size_t n_rows, int N, float* sigma, void* stream) {
  if (int rc = check_net(h, prec, "dfn_mlp_coarse_points", true)) return rc;
  if (!n_rows) return DFN_OK;
  if (!pts || !sigma) return set_error(DFN_ERR_ARG, "dfn_mlp_coarse_points: bad argument");
  if (int rc = check_points(n_rows, N, "dfn_mlp_coarse_points")) return rc;
  const Route r = coarse_route(kDefaultVariant, h->desc.width, prec, true);
  const PackedNet& n = route_net(h, false, prec, r);
  MlpArgs a{n.blob, n.tab, n.n_units, pts, nullptr, nullptr, nullptr, sigma, nullptr, (long long)n_rows, N, 0.f, 0.f, nullptr, n.in_scale};
  a.status = range_flag_of(h);
  CHECK_HIP(launch_route(h, false, prec, r, a, HS(stream)), "dfn_mlp_coarse_points");
  return DFN_OK;
}

extern "C" int dfn_mlp_fine_points(dfn_nerfh_t h, int prec, const float* pts, const float* viewdirs, const float* hist, size_t hist_rows,
                                   size_t n_rows, int N, float* raw, void* bias_ws, void* stream) {
  if (int rc = check_net(h, prec, "dfn_mlp_fine_points", true)) return rc;
  if (!n_rows) return DFN_OK;
  if (!pts || !viewdirs || !hist || !raw || !bias_ws || (hist_rows != 1 && hist_rows != n_rows))
    return set_error(DFN_ERR_ARG, "dfn_mlp_fine_points: bad argument (hist_rows must be 1 or n_rows)");
  if (int rc = check_points(n_rows, N, "dfn_mlp_fine_points")) return rc;
  float* table = static_cast<float*>(bias_ws);
  const Route r = fine_route(kDefaultVariant, h->desc.width, prec, false, false, true);
  CHECK_HIP(launch_ray_bias(r.fold_table ? h->rb_fold : h->rb, viewdirs, hist, hist_rows, n_rows, table, HS(stream)), "dfn_mlp_fine_points(ray_bias)");
  const PackedNet& n = route_net(h, true, prec, r);
  MlpArgs a{n.blob, n.tab, n.n_units, pts, nullptr, nullptr, table, raw, nullptr, (long long)n_rows, N, 0.f, 0.f, nullptr, n.in_scale};
  a.status = range_flag_of(h);
  CHECK_HIP(launch_route(h, true, prec, r, a, HS(stream)), "dfn_mlp_fine_points");
  return DFN_OK;
}

extern "C" int dfn_mlp_fine_points_backward(dfn_nerfh_t h, int prec, const float* pts, const float* viewdirs, const float* hist,
                                            size_t hist_rows, size_t n_rows, int N, const float* grad_raw, float* grad_pts, void* bias_ws,
                                            void* stream) {
  if (int rc = check_net(h, prec, "dfn_mlp_fine_points_backward", true)) return rc;
  if (int rc = check_grad_prec(prec, "dfn_mlp_fine_points_backward")) return rc;
  if (int rc = check_grad_width(h, "dfn_mlp_fine_points_backward")) return rc;
  if (!n_rows) return DFN_OK;
  if (!pts || !viewdirs || !hist || !grad_raw || !grad_pts || !bias_ws || (hist_rows != 1 && hist_rows != n_rows))
    return set_error(DFN_ERR_ARG, "dfn_mlp_fine_points_backward: bad argument (hist_rows must be 1 or n_rows)");
  if (int rc = check_points(n_rows, N, "dfn_mlp_fine_points_backward")) return rc;
  float* table = static_cast<float*>(bias_ws);
  CHECK_HIP(launch_ray_bias(h->rb, viewdirs, hist, hist_rows, n_rows, table, HS(stream)), "dfn_mlp_fine_points_backward(ray_bias)");
  const PackedNet& n = h->bwd[prec];
  BwdArgs a{n.blob, n.tab, n.n_units, pts, nullptr, viewdirs, nullptr, table, grad_raw, grad_pts, (long long)n_rows, N, n.in_scale};
  CHECK_HIP(launch_mlp_fine_backward_pts(prec, a, device_cu_count(), HS(stream)), "dfn_mlp_fine_points_backward");
  return DFN_OK;
}

// nerfw.py:37-46, 315-334 under autograd: d L / d sigma of the test-time coarse query -> d L / d point.
extern "C" int dfn_mlp_coarse_points_backward(dfn_nerfh_t h, int prec, const float* pts, size_t n_rows, int N, const float* grad_sigma,
                                              float* grad_pts, void* stream) {
  if (int rc = check_net(h, prec, "dfn_mlp_coarse_points_backward", true)) return rc;
  if (int rc = check_grad_prec(prec, "dfn_mlp_coarse_points_backward")) return rc;
  if (int rc = check_grad_width(h, "dfn_mlp_coarse_points_backward")) return rc;
  if (!n_rows) return DFN_OK;
  if (!pts || !grad_sigma || !grad_pts) return set_error(DFN_ERR_ARG, "dfn_mlp_coarse_points_backward: bad argument (null pointer)");
  if (int rc = check_points(n_rows, N, "dfn_mlp_coarse_points_backward")) return rc;
  const PackedNet& n = h->bwd_coarse[prec];
  BwdArgs a{n.blob, n.tab, n.n_units, pts, nullptr, nullptr, nullptr, nullptr, grad_sigma, grad_pts, (long long)n_rows, N, n.in_scale};
  CHECK_HIP(launch_mlp_coarse_backward_pts(prec, a, device_cu_count(), HS(stream)), "dfn_mlp_coarse_points_backward");
  return DFN_OK;
}

// nerfw.py:47-60, 326-343: the training coarse query of run_network_NeRFW on pre-sampled points, [static_rgb(3), static_sigma] per point.
// The per-row seed table (b_dir + W_dir[:, W:W+27] . pe_dir(v) of the coarse dir_encoding.0) is written by ray_bias_kernel from a weight
// set without appearance columns; its "shared histogram" order (hist_rows = 1, nothing to gather) is used for every row count, so a
// row's seeds do not depend on how the caller chunks the rows.
extern "C" int dfn_mlp_coarse_static_points(dfn_nerfh_t h, int prec, const float* pts, const float* viewdirs, size_t n_rows, int N,
                                            float* raw4, void* bias_table, void* stream) {
  if (int rc = check_net(h, prec, "dfn_mlp_coarse_static_points", true)) return rc;
  if (!n_rows) return DFN_OK;
  if (!pts || !viewdirs || !raw4 || !bias_table) return set_error(DFN_ERR_ARG, "dfn_mlp_coarse_static_points: bad argument (null pointer)");
  if (int rc = check_points(n_rows, N, "dfn_mlp_coarse_static_points")) return rc;
  float* table = static_cast<float*>(bias_table);
  const bool fold = prec == DFN_PREC_F16X3 && h->desc.width == kWidth;   // the 16x16x32 kernel with the folded tail
  CHECK_HIP(launch_ray_bias(fold ? h->rb_cstatic_fold : h->rb_cstatic, viewdirs, nullptr, 1, n_rows, table, HS(stream)),
            "dfn_mlp_coarse_static_points(ray_bias)");
  const PackedNet& n = h->cstatic[prec];
  MlpArgs a{n.blob, n.tab, n.n_units, pts, nullptr, nullptr, table, raw4, nullptr, (long long)n_rows, N, 0.f, 0.f, nullptr, n.in_scale};
  a.status = range_flag_of(h);
  CHECK_HIP(fold ? launch_mlp_static_pts_fold(a, device_cu_count(), HS(stream))
                 : launch_mlp_static_pts(prec, a, device_cu_count(), HS(stream), h->desc.width),
            "dfn_mlp_coarse_static_points");
  return DFN_OK;
}

// ... under autograd: d L / d raw4 -> [d L / d point (3), d L / d viewdir through that point (3)].
extern "C" int dfn_mlp_coarse_static_points_backward(dfn_nerfh_t h, int prec, const float* pts, const float* viewdirs, size_t n_rows, int N,
                                                     const float* grad_raw4, float* grad_pts6, void* bias_table, void* stream) {
  if (int rc = check_net(h, prec, "dfn_mlp_coarse_static_points_backward", true)) return rc;
  if (int rc = check_grad_prec(prec, "dfn_mlp_coarse_static_points_backward")) return rc;
  if (int rc = check_grad_width(h, "dfn_mlp_coarse_static_points_backward")) return rc;
  if (!n_rows) return DFN_OK;
  if (!pts || !viewdirs || !grad_raw4 || !grad_pts6 || !bias_table)
    return set_error(DFN_ERR_ARG, "dfn_mlp_coarse_static_points_backward: bad argument (null pointer)");
  if (int rc = check_points(n_rows, N, "dfn_mlp_coarse_static_points_backward")) return rc;
  float* table = static_cast<float*>(bias_table);
  CHECK_HIP(launch_ray_bias(h->rb_cstatic, viewdirs, nullptr, 1, n_rows, table, HS(stream)), "dfn_mlp_coarse_static_points_backward(ray_bias)");
  const PackedNet& n = h->bwd_cstatic[prec];
  BwdArgs a{n.blob, n.tab, n.n_units, pts, nullptr, viewdirs, nullptr, table, grad_raw4, grad_pts6, (long long)n_rows, N, n.in_scale};
  CHECK_HIP(launch_mlp_coarse_static_backward_pts(prec, a, device_cu_count(), HS(stream)), "dfn_mlp_coarse_static_points_backward");
  return DFN_OK;
}

extern "C" size_t dfn_mlp_fine_mask_bytes(size_t n_points) {
  return (n_points + kBwdTilePoints - 1) / kBwdTilePoints * (kBwdTilePoints / 32) * kBwdMaskWords * 64 * sizeof(uint32_t);
}

extern "C" int dfn_mlp_fine_saving(dfn_nerfh_t h, int prec, const float* rays_o, const float* rays_d, const float* viewdirs,
                                   const float* hist, size_t hist_rows, size_t n_rays, const float* z_fine, int Nf, float* raw,
                                   void* masks, void* bias_ws, void* stream) {
  if (int rc = check_net(h, prec, "dfn_mlp_fine_saving", true)) return rc;
  if (int rc = check_grad_width(h, "dfn_mlp_fine_saving")) return rc;
  if (prec != DFN_PREC_F16X3) return set_error(DFN_ERR_UNSUPPORTED, "dfn_mlp_fine_saving: split-f16 (DFN_PREC_F16X3) only");
  if (!n_rays) return DFN_OK;
  if (!rays_o || !rays_d || !viewdirs || !hist || !z_fine || !raw || !masks || !bias_ws || Nf < 1 ||
      (hist_rows != 1 && hist_rows != n_rays))
    return set_error(DFN_ERR_ARG, "dfn_mlp_fine_saving: bad argument (hist_rows must be 1 or n_rays)");
  float* table = static_cast<float*>(bias_ws);
  CHECK_HIP(launch_ray_bias(h->rb, viewdirs, hist, hist_rows, n_rays, table, HS(stream)), "dfn_mlp_fine_saving(ray_bias)");
  // the test-time fine kernel itself (pipelined epilogue, unit-scale weights), recording the ReLU signs as it goes
  const PackedNet& n = h->net[1][prec][0];
  MlpArgs a{n.blob, n.tab, n.n_units, rays_o, rays_d, z_fine, table, raw, nullptr, (long long)n_rays, Nf, 0.f, 0.f, nullptr, n.in_scale};
  a.status = range_flag_of(h);
  a.masks = static_cast<uint32_t*>(masks);
  CHECK_HIP(launch_mlp(true, prec, 0, a, device_cu_count(), HS(stream), h->desc.width), "dfn_mlp_fine_saving");
  return DFN_OK;
}

extern "C" int dfn_mlp_fine_backward_saved(dfn_nerfh_t h, int prec, const float* rays_o, const float* rays_d, const float* viewdirs,
                                           size_t n_rays, const float* z_fine, int Nf, const float* raw, const void* masks,
                                           const float* grad_raw, float* grad_pts, void* stream) {
  if (int rc = check_net(h, prec, "dfn_mlp_fine_backward_saved", true)) return rc;
  if (int rc = check_grad_width(h, "dfn_mlp_fine_backward_saved")) return rc;
  if (prec != DFN_PREC_F16X3) return set_error(DFN_ERR_UNSUPPORTED, "dfn_mlp_fine_backward_saved: split-f16 (DFN_PREC_F16X3) only");
  if (!n_rays) return DFN_OK;
  if (!rays_o || !rays_d || !viewdirs || !z_fine || !raw || !masks || !grad_raw || !grad_pts || Nf < 1)
    return set_error(DFN_ERR_ARG, "dfn_mlp_fine_backward_saved: bad argument");
  const PackedNet& n = h->bwd[prec];
  BwdArgs a{n.blob, n.tab + 2 * n.n_fwd_units, n.n_units - n.n_fwd_units, rays_o, rays_d, viewdirs, z_fine, nullptr, grad_raw, grad_pts,
            (long long)n_rays, Nf, n.in_scale, nullptr, raw, static_cast<uint32_t*>(const_cast<void*>(masks))};
  CHECK_HIP(launch_mlp_fine_backward(prec, a, device_cu_count(), HS(stream), 2), "dfn_mlp_fine_backward_saved");
  return DFN_OK;
}

extern "C" int dfn_ray_grad_reduce(const float* grad_pts, const float* z_fine, const float* rays_d, size_t n_rays, int Nf,
                                   int derive_viewdirs, float* grad_rays_o, float* grad_rays_d, float* grad_viewdirs,
                                   void* stream) {
  if (!grad_pts || !z_fine || !rays_d || !grad_rays_o || !grad_rays_d || Nf < 1)
    return set_error(DFN_ERR_ARG, "dfn_ray_grad_reduce: bad argument");
  CHECK_HIP(launch_ray_grad_reduce(grad_pts, z_fine, rays_d, n_rays, Nf, derive_viewdirs, grad_rays_o, grad_rays_d, grad_viewdirs,
                                   HS(stream)),
            "dfn_ray_grad_reduce");
  return DFN_OK;
}

extern "C" int dfn_raygen_frames(int B, int H, int W, float focal, const float* c2w, float* rays_o, float* rays_d, float* viewdirs,
                                 void* stream) {
  if (B < 1 || H < 0 || W < 0 || !c2w || !rays_o || !rays_d || !(focal > 0)) return set_error(DFN_ERR_ARG, "dfn_raygen_frames: bad argument");
  CHECK_HIP(launch_raygen(H, W, focal, c2w, rays_o, rays_d, viewdirs, HS(stream), B), "dfn_raygen_frames");
  return DFN_OK;
}
extern "C" int dfn_raygen_frames_backward(int B, int H, int W, float focal, const float* grad_rays_o, const float* grad_rays_d,
                                          float* grad_c2w, void* stream) {
  if (B < 1 || H < 1 || W < 1 || !grad_rays_o || !grad_rays_d || !grad_c2w || !(focal > 0))
    return set_error(DFN_ERR_ARG, "dfn_raygen_frames_backward: bad argument");
  CHECK_HIP(launch_raygen_backward(H, W, focal, grad_rays_o, grad_rays_d, grad_c2w, HS(stream), B), "dfn_raygen_frames_backward");
  return DFN_OK;
}

extern "C" int dfn_raygen_backward(int H, int W, float focal, const float* grad_rays_o, const float* grad_rays_d, float* grad_c2w,
                                   void* stream) {
  if (H < 1 || W < 1 || !(focal > 0) || !grad_rays_o || !grad_rays_d || !grad_c2w)
    return set_error(DFN_ERR_ARG, "dfn_raygen_backward: bad argument");
  CHECK_HIP(launch_raygen_backward(H, W, focal, grad_rays_o, grad_rays_d, grad_c2w, HS(stream)), "dfn_raygen_backward");
  return DFN_OK;
}

namespace {
struct BwdWorkspace {
  Workspace f;
  float *graw, *gpts, *go, *gd;
  size_t total;
};
BwdWorkspace carve_bwd(char* base, size_t n_rays, int Nc, int Ni) {
  BwdWorkspace b{};
  b.f = carve(base, n_rays, Nc, Ni, true);
  const size_t chunk = chunk_rays(n_rays), Nf = size_t(Nc) + Ni;
  size_t off = b.f.total;
  auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += al(bytes); return reinterpret_cast<float*>(p); };
  b.graw = take(chunk * Nf * 9 * 4);
  b.gpts = take(chunk * Nf * 6 * 4);
  b.go = take(n_rays * 12);
  b.gd = take(n_rays * 12);
  b.total = off;
  return b;
}

// Forward recompute (coarse -> sampler -> fine raw) then the gradient kernels, chunk by chunk.
int render_backward_core(dfn_nerfh_t h, int prec, const float* o, const float* d, const float* v, bool derive_v,
                         const float* hist, size_t hist_rows, size_t n_rays, int Nc, int Ni, float near, float far,
                         const float* grad_rgb, float* go, float* gd, float* gv, const BwdWorkspace& w, hipStream_t s) {
  const int Nf = Nc + Ni, var = route_facts(mlp_variant_128(), h->desc.width).base, cus = device_cu_count();
  const PackedNet& nc = h->net[0][prec][var];
  const PackedNet& nf = h->net[1][prec][var];
  const PackedNet& nb = h->bwd[prec];
  const size_t chunk = chunk_rays(n_rays);
  for (size_t r0 = 0; r0 < n_rays; r0 += chunk) {
    const size_t n = n_rays - r0 < chunk ? n_rays - r0 : chunk;
    const float* co = o + r0 * 3;
    const float* cd = d + r0 * 3;
    const float* cv = v + r0 * 3;
    const float* ch = hist_rows == 1 ? hist : hist + r0 * h->desc.hist_bin;
    MlpArgs ac{nc.blob, nc.tab, nc.n_units, co, cd, nullptr, nullptr, w.f.sigma, nullptr, (long long)n, Nc, near, far, nullptr, nc.in_scale,
                 h->render_flags & DFN_RENDER_LINDISP};
    ac.status = range_flag_of(h);
    CHECK_HIP(launch_mlp(false, prec, var, ac, cus, s, h->desc.width), "render backward: coarse MLP");
    CHECK_HIP(launch_sample_fine(w.f.sigma, n, Nc, Ni, near, far, w.f.z, nullptr, nullptr, s, h->render_flags & DFN_RENDER_LINDISP),
              "render backward: sample_fine");
    CHECK_HIP(launch_ray_bias(h->rb, cv, ch, hist_rows, n, w.f.bias, s), "render backward: ray_bias");
    MlpArgs af{nf.blob, nf.tab, nf.n_units, co, cd, w.f.z, w.f.bias, w.f.raw, nullptr, (long long)n, Nf, 0.f, 0.f, nullptr, nf.in_scale};
    af.status = range_flag_of(h);
    CHECK_HIP(launch_mlp(true, prec, var, af, cus, s, h->desc.width), "render backward: fine MLP");
    CHECK_HIP(launch_composite_fine_backward(w.f.raw, w.f.z, grad_rgb + r0 * 3, n, Nf, w.graw, s), "render backward: composite");
    BwdArgs ab{nb.blob, nb.tab, nb.n_units, co, cd, cv, w.f.z, w.f.bias, w.graw, w.gpts, (long long)n, Nf, nb.in_scale};
    CHECK_HIP(launch_mlp_fine_backward(prec, ab, cus, s), "render backward: fine MLP gradient");
    CHECK_HIP(launch_ray_grad_reduce(w.gpts, w.f.z, cd, n, Nf, derive_v ? 1 : 0, go + r0 * 3, gd + r0 * 3,
                                     gv ? gv + r0 * 3 : nullptr, s),
              "render backward: ray reduction");
  }
  return DFN_OK;
}
}  // namespace

extern "C" size_t dfn_render_backward_workspace_bytes(size_t n_rays, int Nc, int Ni) {
  return carve_bwd(nullptr, n_rays ? n_rays : 1, Nc, Ni).total;
}

extern "C" int dfn_render_rays_backward(dfn_nerfh_t h, int prec, const float* rays_o, const float* rays_d, const float* viewdirs,
                                        const float* hist, size_t hist_rows, size_t n_rays, int Nc, int Ni, float near,
                                        float far, const float* grad_rgb, float* grad_rays_o, float* grad_rays_d,
                                        float* grad_viewdirs, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_net(h, prec, "dfn_render_rays_backward", true)) return rc;
  if (int rc = check_grad_prec(prec, "dfn_render_rays_backward")) return rc;
  if (int rc = check_grad_width(h, "dfn_render_rays_backward")) return rc;
  if (int rc = check_render_args(Nc, Ni, "dfn_render_rays_backward")) return rc;
  if (!n_rays) return DFN_OK;
  if (!rays_o || !rays_d || !hist || !grad_rgb || !grad_rays_o || !grad_rays_d || !workspace ||
      (hist_rows != 1 && hist_rows != n_rays))
    return set_error(DFN_ERR_ARG, "dfn_render_rays_backward: bad argument (hist_rows must be 1 or n_rays)");
  if (!n_rays) return DFN_OK;
  const BwdWorkspace w = carve_bwd(static_cast<char*>(workspace), n_rays, Nc, Ni);
  if (w.total > workspace_bytes)
    return set_error(DFN_ERR_ARG, "dfn_render_rays_backward: workspace too small (%zu < %zu)", workspace_bytes, w.total);
  const float* v = viewdirs;
  if (!v) {
    CHECK_HIP(launch_viewdirs(rays_d, n_rays, w.f.v, HS(stream)), "dfn_render_rays_backward: viewdirs");
    v = w.f.v;
  }
  return render_backward_core(h, prec, rays_o, rays_d, v, viewdirs == nullptr, hist, hist_rows, n_rays, Nc, Ni, near, far,
                              grad_rgb, grad_rays_o, grad_rays_d, viewdirs ? grad_viewdirs : nullptr, w, HS(stream));
}

extern "C" int dfn_render_image_backward(dfn_nerfh_t h, int prec, const float* c2w, int H, int W, float focal, float near,
                                         float far, int Nc, int Ni, const float* hist, const float* grad_rgb,
                                         float* grad_c2w, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_net(h, prec, "dfn_render_image_backward", true)) return rc;
  if (int rc = check_grad_prec(prec, "dfn_render_image_backward")) return rc;
  if (int rc = check_grad_width(h, "dfn_render_image_backward")) return rc;
  if (int rc = check_render_args(Nc, Ni, "dfn_render_image_backward")) return rc;
  if (!c2w || !hist || !grad_rgb || !grad_c2w || !workspace || H < 1 || W < 1 || !(focal > 0))
    return set_error(DFN_ERR_ARG, "dfn_render_image_backward: bad argument");
  const size_t n_rays = size_t(H) * W;
  const BwdWorkspace w = carve_bwd(static_cast<char*>(workspace), n_rays, Nc, Ni);
  if (w.total > workspace_bytes)
    return set_error(DFN_ERR_ARG, "dfn_render_image_backward: workspace too small (%zu < %zu)", workspace_bytes, w.total);
  CHECK_HIP(launch_raygen(H, W, focal, c2w, w.f.o, w.f.d, w.f.v, HS(stream)), "dfn_render_image_backward: raygen");
  if (int rc = render_backward_core(h, prec, w.f.o, w.f.d, w.f.v, true, hist, 1, n_rays, Nc, Ni, near, far, grad_rgb, w.go,
                                    w.gd, nullptr, w, HS(stream)))
    return rc;
  CHECK_HIP(launch_raygen_backward(H, W, focal, w.go, w.gd, grad_c2w, HS(stream)), "dfn_render_image_backward: raygen");
  return DFN_OK;
}
