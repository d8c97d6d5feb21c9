// nerfh_recommit.hip — dfn_nerfh_recommit_device: re-pack every buffer of a committed NeRF-H handle in place from parameters that
// live on the device.  Three kernels on the caller's stream: the two weight maxima (read back with one 8-byte copy: the scales are host
// floats that the render kernels take as arguments), fold_final into the pseudo-parameter arena (netwidth 128), and one gather-pack
// over the plan the host packer recorded (nerfh_recommit.h).  No allocation after the first call, no host copy of a parameter.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/dfnet_hip.h"
#include "dfn_common.h"
#include "nerfh_handle.h"
#include "nerfh_recommit.h"

using namespace dfn;
using namespace dfn::recommit;

namespace dfn {
namespace recommit {
struct State {
  PlanElem* elems = nullptr;     // device
  uint32_t n_elems = 0;
  float* arena = nullptr;        // device: pseudo-parameters (arena_floats)
  uint32_t* wmax = nullptr;      // device: bit patterns of the two maxima
  std::vector<CopySeg> copies;
  int gen_buf = -1;
  std::vector<BufShape> shapes;
};
}  // namespace recommit
}  // namespace dfn

namespace {

struct ScanArgs {
  const float* p[kMaxSrc];
  uint32_t numel[kMaxSrc];
  int net[kMaxSrc];
  uint32_t* out;
};
// max |w| per network over its weight tensors, as the host scan: NaN never wins (std::fmax).  Non-negative floats order as their bits.
__global__ __launch_bounds__(256) void weight_max_kernel(ScanArgs a) {
  __shared__ uint32_t sm;
  if (threadIdx.x == 0) sm = 0u;
  __syncthreads();
  const float* p = a.p[blockIdx.y];
  const uint32_t n = a.numel[blockIdx.y];
  uint32_t m = 0u;
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const float x = fabsf(p[i]);
    if (x == x) m = max(m, __float_as_uint(x));
  }
  atomicMax(&sm, m);
  __syncthreads();
  if (threadIdx.x == 0 && sm) atomicMax(a.out + a.net[blockIdx.y], sm);
}

struct FoldArgs {
  const float* a[3];
  const float* F[3];
  const float* bF[3];
  const float* bA[3];
  int lda[3];
  int W;
  float* arena;
};
// blockIdx.y: the fold; one thread per output (row r, column c <= W; c == W is the bias)
__global__ __launch_bounds__(256) void fold_kernel(FoldArgs a) {
  const int k = blockIdx.y, W = a.W;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= (W / 2) * (W + 1)) return;
  const int r = t / (W + 1), c = t % (W + 1);
  const float v = fold_elem(a.a[k], a.lda[k], a.F[k], a.bF[k], a.bA[k], W, r, c);
  a.arena[c < W ? arena_off(k, W) + size_t(r) * W + c : arena_off(3 + k, W) + r] = v;
}

struct PackArgs {
  const float* src[kMaxSrc];       // canonical parameters, then the pseudo-parameters
  char* dst[kMaxBufs];
  float wscale[kMaxBufs];          // 1 for a buffer without a scale
  const PlanElem* elems;
  uint32_t n_elems;
  float* gen;                      // gen_blob
  uint32_t seg_numel[kMaxSrc], seg_off[kMaxSrc];
  int n_seg;
};
// blockIdx.y = 0: the plan entries, a grid-stride loop; 1: gen_blob, segment after segment
__global__ __launch_bounds__(256) void pack_kernel(PackArgs a) {
  const uint32_t stride = gridDim.x * 256, t0 = blockIdx.x * 256 + threadIdx.x;
  if (blockIdx.y == 0) {
    for (uint32_t i = t0; i < a.n_elems; i += stride) {
      const PlanElem e = a.elems[i];
      const uint32_t buf = e.dst >> 24;
      store_elem(a.dst[buf], e, a.src[e.src >> kIdxBits], a.wscale[buf]);
    }
    return;
  }
  for (int s = 0; s < a.n_seg; ++s) {
    const float* p = a.src[s];
    float* q = a.gen + a.seg_off[s];
    for (uint32_t i = t0; i < a.seg_numel[s]; i += stride) q[i] = p[i];
  }
}

int build_state(dfn_nerfh_s* h) {
  HostPlan plan;
  auto* st = new State();
  int rc = build_plan(h->desc, plan, st->shapes);
  if (rc == DFN_OK && st->shapes.size() != h->bufs.size()) rc = set_error(DFN_ERR_STATE, "dfn_nerfh_recommit_device: the plan names %zu buffers, the handle holds %zu", st->shapes.size(), h->bufs.size());
  for (size_t i = 0; rc == DFN_OK && i < st->shapes.size(); ++i)
    if (st->shapes[i].bytes != h->bufs[i].bytes || st->shapes[i].name != h->bufs[i].name)
      rc = set_error(DFN_ERR_STATE, "dfn_nerfh_recommit_device: buffer %zu of the plan (%s) is not the handle's (%s)", i, st->shapes[i].name.c_str(), h->bufs[i].name.c_str());
  // every load and store of the pack kernel stays inside its tensor / buffer: checked here, once, on the host
  const int np = dfn_nerfh_train_param_count(), W = h->desc.width;
  if (rc == DFN_OK && int(plan.copies.size()) != np) rc = set_error(DFN_ERR_STATE, "dfn_nerfh_recommit_device: the plan lists %zu parameters", plan.copies.size());
  for (size_t i = 0; rc == DFN_OK && i < plan.elems.size(); ++i) {
    const PlanElem e = plan.elems[i];
    const size_t buf = e.dst >> 24, idx = e.src & ((1u << kIdxBits) - 1u);
    const int src = int(e.src >> kIdxBits);
    const size_t numel = src < np ? plan.copies[src].numel : (src < np + 3 ? size_t(W / 2) * W : size_t(W / 2));
    if (buf >= st->shapes.size() || !elem_in_bounds(e, st->shapes[buf].bytes) || src >= np + kPseudo || idx >= numel)
      rc = set_error(DFN_ERR_STATE, "dfn_nerfh_recommit_device: plan entry %zu leaves its buffer or its parameter", i);
  }
  for (size_t i = 0; rc == DFN_OK && i < plan.copies.size(); ++i)
    if (plan.gen_buf < 0 || (plan.copies[i].dst_off + plan.copies[i].numel) * 4 > st->shapes[plan.gen_buf].bytes || plan.copies[i].src != int(i))
      rc = set_error(DFN_ERR_STATE, "dfn_nerfh_recommit_device: gen_blob segment %zu leaves the buffer", i);
  if (rc == DFN_OK) {
    st->n_elems = uint32_t(plan.elems.size());
    st->copies = plan.copies;
    st->gen_buf = plan.gen_buf;
    const size_t eb = plan.elems.size() * sizeof(PlanElem);
    if (hipMalloc(reinterpret_cast<void**>(&st->elems), eb ? eb : 16) != hipSuccess ||
        (eb && hipMemcpy(st->elems, plan.elems.data(), eb, hipMemcpyHostToDevice) != hipSuccess) ||
        hipMalloc(reinterpret_cast<void**>(&st->arena), arena_floats(h->desc.width) * sizeof(float)) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&st->wmax), 2 * sizeof(uint32_t)) != hipSuccess)
      rc = set_error(DFN_ERR_HIP, "dfn_nerfh_recommit_device: uploading the plan (%zu bytes) failed", eb);
  }
  h->recommit = st;   // destroy_state frees a partial state through the handle
  if (rc != DFN_OK) dfn::recommit::destroy_state(h);
  return rc;
}

}  // namespace

void dfn::recommit::destroy_state(dfn_nerfh_s* h) {
  auto* st = static_cast<State*>(h->recommit);
  if (!st) return;
  if (st->elems) (void)hipFree(st->elems);
  if (st->arena) (void)hipFree(st->arena);
  if (st->wmax) (void)hipFree(st->wmax);
  delete st;
  h->recommit = nullptr;
}

extern "C" int dfn_nerfh_recommit_device(dfn_nerfh_t h, const float* const* params, void* stream) {
  if (!h || !params) return set_error(DFN_ERR_ARG, "dfn_nerfh_recommit_device: null handle / parameter list");
  const int np = dfn_nerfh_train_param_count();
  for (int i = 0; i < np; ++i)
    if (!params[i]) return set_error(DFN_ERR_ARG, "dfn_nerfh_recommit_device: parameter %d (%s) is null", i, dfn_nerfh_train_param_name(i));
  if (!h->committed || h->bufs.empty())
    return set_error(DFN_ERR_STATE, "dfn_nerfh_recommit_device: the handle was never committed on the host (dfn_nerfh_set_param x N + dfn_nerfh_commit come first)");
  if (!h->recommit)
    if (int rc = build_state(h)) return rc;
  State* st = static_cast<State*>(h->recommit);
  if (st->shapes.size() != h->bufs.size()) return set_error(DFN_ERR_STATE, "dfn_nerfh_recommit_device: the handle's buffers changed under the plan");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int W = h->desc.width;
  const bool fast = W == kWidth || W == kMaxWidth;

  float in_scale[kScales] = {1.f, 1.f, 1.f, 1.f}, wscale[kScales] = {1.f, 1.f, 1.f, 1.f};
  if (fast) {   // the two maxima: the one wait of this entry, for 8 bytes
    ScanArgs sa{};
    int n = 0;
    for (int i = 0; i < np; ++i) {
      const int net = scan_net(dfn_nerfh_train_param_name(i));
      if (net < 0) continue;
      sa.p[n] = params[i];
      sa.numel[n] = st->copies[i].numel;
      sa.net[n] = net;
      ++n;
    }
    sa.out = st->wmax;
    uint32_t bits[2] = {0u, 0u};
    if (hipMemsetAsync(st->wmax, 0, sizeof bits, s) != hipSuccess) return set_error(DFN_ERR_HIP, "dfn_nerfh_recommit_device: clearing the maxima failed");
    hipLaunchKernelGGL(weight_max_kernel, dim3(8, n), dim3(256), 0, s, sa);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(bits, st->wmax, sizeof bits, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
      return set_error(DFN_ERR_HIP, "dfn_nerfh_recommit_device: reading the weight maxima failed");
    float wmax[2];
    std::memcpy(wmax, bits, sizeof wmax);
    scales_from_max(wmax, in_scale, wscale);
  }

  PackArgs pa{};
  for (int i = 0; i < np; ++i) pa.src[i] = params[i];
  for (int k = 0; k < kPseudo; ++k) pa.src[np + k] = st->arena + arena_off(k, W);
  for (size_t i = 0; i < h->bufs.size(); ++i) {
    pa.dst[i] = static_cast<char*>(h->bufs[i].ptr);
    pa.wscale[i] = h->bufs[i].scale >= 0 ? wscale[h->bufs[i].scale] : 1.f;
  }
  pa.elems = st->elems;
  pa.n_elems = st->n_elems;
  pa.gen = static_cast<float*>(h->bufs[st->gen_buf].ptr);
  pa.n_seg = int(st->copies.size());
  for (int i = 0; i < pa.n_seg; ++i) {
    pa.seg_numel[i] = st->copies[i].numel;
    pa.seg_off[i] = uint32_t(st->copies[i].dst_off);
  }

  if (W == kWidth) {
    FoldSpec fs[3];
    fold_specs(h->desc, fs);
    FoldArgs fa{};
    for (int k = 0; k < 3; ++k) {
      fa.a[k] = params[fs[k].a];
      fa.F[k] = params[fs[k].F];
      fa.bF[k] = params[fs[k].bF];
      fa.bA[k] = params[fs[k].bA];
      fa.lda[k] = fs[k].lda;
    }
    fa.W = W;
    fa.arena = st->arena;
    hipLaunchKernelGGL(fold_kernel, dim3(((W / 2) * (W + 1) + 255) / 256, 3), dim3(256), 0, s, fa);
    if (hipGetLastError() != hipSuccess) return set_error(DFN_ERR_HIP, "dfn_nerfh_recommit_device: launching the fold kernel failed");
  }
  const uint32_t work = st->n_elems > 65536u ? st->n_elems : 65536u;
  uint32_t grid = (work + 255) / 256;
  grid = grid > 2048u ? 2048u : grid;
  hipLaunchKernelGGL(pack_kernel, dim3(grid, 2), dim3(256), 0, s, pa);
  if (hipGetLastError() != hipSuccess) return set_error(DFN_ERR_HIP, "dfn_nerfh_recommit_device: launching the pack kernel failed");

  for (const PackedBufInfo& b : h->bufs)
    if (b.scale >= 0) nerfh_net_at(h, b.net)->in_scale = in_scale[b.scale];
  // the host copies are now older than the packed buffers: dfn_nerfh_commit refuses until every one of them has been set again
  for (int i = 0; i < np; ++i) h->stale_params.insert(dfn_nerfh_train_param_name(i));
  return DFN_OK;
}
