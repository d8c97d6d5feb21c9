// nerfh_recommit.h — the device-side re-commit of a NeRF-H handle (dfn_nerfh_recommit_device): what nerfh_pack.hip (the host packer,
// which emits the plan) and nerfh_recommit.hip (the kernels that execute it) share.
//
// A plan is the host packer's own record of where every packed element came from.  While dfn_nerfh_commit's packing code runs in plan
// mode, each store of a value that is a parameter goes through one emit helper (Packer::emit_w / emit_b, put_extra), which ALSO notes
// (buffer, byte offset, element kind, parameter, index).  Elements the packer fills with zero have no entry: a re-commit rewrites
// buffers that a host commit produced, geometry does not change, so they already hold zero.  The three matrices and three bias
// vectors of fold_final are pseudo-parameters behind the canonical list, in a device arena that a fold kernel fills first.  gen_blob
// (every parameter as a plain tensor) is copied segment by segment without entries.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/dfnet_hip.h"
#include "nerfh_layout.h"

struct dfn_nerfh_s;

namespace dfn {
namespace recommit {

enum ElemKind : uint32_t {
  K_F32 = 0,    // float = w
  K_F16 = 1,    // f16 = w
  K_SPLIT = 2,  // f16 hi = w x wscale at the offset, f16 lo = w x wscale - hi 1024 bytes behind it
  K_BIAS = 3    // float = b x wscale x kX3ActScale
};
// weight scales of a handle: [0] coarse, [1] fine render blobs; [2] coarse, [3] fine gradient blobs (x 1024)
constexpr int kScales = 4;
constexpr int kMaxBufs = 96;     // packed buffers of one handle (netwidth 128: 53)
constexpr int kMaxSrc = 80;      // canonical parameters + pseudo-parameters
constexpr int kPseudo = 6;       // fold_dir, fold_tr, coarse fold_dir [W/2][W]; b_dir + fold, b_tr + fold, coarse b_dir + fold [W/2]
constexpr uint32_t kOffBits = 22, kIdxBits = 24;

// dst = buffer << 24 | kind << 22 | byte offset >> 1;  src = source << 24 | index
struct PlanElem { uint32_t dst, src; };
struct CopySeg { int src; uint32_t numel; size_t dst_off; };   // gen_blob: floats [dst_off, dst_off + numel) = parameter src

struct BufShape { std::string name; size_t bytes = 0; int net = -1; int field = 0; int scale = -1; };

struct HostPlan {
  std::vector<PlanElem> elems;
  std::vector<CopySeg> copies;
  int gen_buf = -1;
  bool overflow = false;   // an offset or index outside the entry's fields
  void add(int buf, uint32_t kind, size_t byte_off, int src, size_t idx) {
    if (buf < 0 || buf >= kMaxBufs || (byte_off >> 1) >> kOffBits || src < 0 || src >= kMaxSrc || idx >> kIdxBits) { overflow = true; return; }
    elems.push_back(PlanElem{uint32_t(buf) << 24 | kind << kOffBits | uint32_t(byte_off >> 1), uint32_t(src) << kIdxBits | uint32_t(idx)});
  }
};

// One power-of-two weight scale per network: the largest |w| lands in (0.5, 1].  The lo halves of most weights are then f16
// subnormals — still exact to 2^-24 of the largest weight (the matrix cores do not flush f16 denormals), which is fp32's resolution —
// and the accumulators (in_scale x the value = 16 x value / max|w|) fit f16 up to |value| = 4094 max|w|: that is what lets the render
// kernels narrow BEFORE they scale (X3Piece: one packed multiply per result pair instead of two).
inline float weight_scale(float wmax) {
  int sexp = wmax > 0.f ? -int(std::ceil(std::log2(wmax))) : 0;
  sexp = sexp < -8 ? -8 : (sexp > 24 ? 24 : sexp);
  return std::ldexp(1.f, sexp);
}
// The scales of the four classes from the two maxima: the one place that states them, for the host packer (nerfh_pack.hip:
// commit_core) and the device re-commit alike.  in_scale = weight scale x activation scale, what the accumulators carry.  The
// gradient kernels scale their accumulators in fp32 BEFORE narrowing them (store_hidden), so their weights sit x 1024 higher, where
// every lo half is a normal f16 (largest |w| near 2^10: 22 bits per weight) instead of at the render kernels' unit scale.
inline void scales_from_max(const float wmax[2], float in_scale[kScales], float wscale[kScales]) {
  for (int f = 0; f < 2; ++f) {
    in_scale[f] = weight_scale(wmax[f]) * kX3ActScale;
    in_scale[2 + f] = in_scale[f] * 1024.f;
  }
  for (int k = 0; k < kScales; ++k) wscale[k] = in_scale[k] / kX3ActScale;
}
// network whose weight scan a canonical parameter belongs to: 0 coarse, 1 fine, -1 none (biases, embeddings)
inline int scan_net(const std::string& name) {
  if (name.find(".weight") == std::string::npos) return -1;
  if (name.compare(0, 7, "coarse.") == 0) return 0;
  if (name.compare(0, 5, "fine.") == 0) return 1;
  return -1;
}

// does the entry's store stay inside a buffer of `bytes` bytes
inline bool elem_in_bounds(PlanElem e, size_t bytes) {
  const uint32_t kind = (e.dst >> kOffBits) & 3u;
  const size_t off = size_t(e.dst & ((1u << kOffBits) - 1u)) << 1;
  return off + (kind == K_SPLIT ? 1026 : (kind == K_F16 ? 2 : 4)) <= bytes;
}

// One plan entry: the host packer's arithmetic, each operation rounded on its own.
DFN_HD inline void store_elem(char* base, PlanElem e, const float* src, float wscale) {
#pragma clang fp contract(off)
  const uint32_t kind = (e.dst >> kOffBits) & 3u;
  char* p = base + (size_t(e.dst & ((1u << kOffBits) - 1u)) << 1);
  const float v = src[e.src & ((1u << kIdxBits) - 1u)];
  if (kind == K_F32) *reinterpret_cast<float*>(p) = v;
  else if (kind == K_F16) *reinterpret_cast<_Float16*>(p) = _Float16(v);
  else if (kind == K_SPLIT) {
    const float s = v * wscale;
    const _Float16 hi = _Float16(s);
    reinterpret_cast<_Float16*>(p)[0] = hi;
    reinterpret_cast<_Float16*>(p)[512] = _Float16(s - float(hi));
  } else {
    const float s = v * wscale;
    *reinterpret_cast<float*>(p) = s * kX3ActScale;
  }
}

// fold_final, one output: column c < W of (A[:, :W] F)[r], or for c == W the bias (A[:, :W] b_F)[r] + b_A[r].  Double products and
// sums in k order, a multiply and an add each (the host build has no fused multiply-add), rounded to float once.
DFN_HD inline float fold_elem(const float* a, int lda, const float* F, const float* bF, const float* bA, int W, int r, int c) {
#pragma clang fp contract(off)
  double acc = 0.0;
  for (int k = 0; k < W; ++k) {
    const double ark = a[size_t(r) * lda + k];
    const double p = ark * double(c < W ? F[size_t(k) * W + c] : bF[k]);
    acc = acc + p;
  }
  const float f = float(acc);
  return c < W ? f : bA[r] + f;
}

// The pseudo-parameters' arena (netwidth 128 only): three [W/2][W] matrices, then three [W/2] vectors.
DFN_HD inline size_t arena_off(int pseudo, int W) {
  const size_t mat = size_t(W / 2) * W;
  return pseudo < 3 ? pseudo * mat : 3 * mat + size_t(pseudo - 3) * (W / 2);
}
DFN_HD inline size_t arena_floats(int W) { return arena_off(kPseudo, W); }
// fold k of 3: A = parameter a [W/2][lda], F / bF = xyz_encoding_final of the same network, bA = A's bias (canonical indices)
struct FoldSpec { int a, F, bF, bA, lda; };
void fold_specs(const dfn_nerfh_desc& desc, FoldSpec out[3]);   // nerfh_pack.hip

// nerfh_pack.hip: run the packer in plan mode over a scratch parameter set of the handle's geometry (no device call)
int build_plan(const dfn_nerfh_desc& desc, HostPlan& plan, std::vector<BufShape>& shapes);
// nerfh_recommit.hip: frees the uploaded plan of a handle (dfn_nerfh_destroy)
void destroy_state(dfn_nerfh_s* h);

}  // namespace recommit
}  // namespace dfn
