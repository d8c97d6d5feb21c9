// nerfh_api.hip — the C ABI (include/dfnet_hip.h) of the NeRF-H render path: errors, render options, stage entry points and the
// whole-path dfn_render_rays / dfn_render_image drivers.  The handle's life and the host packer behind dfn_nerfh_commit are
// nerfh_pack.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/dfnet_hip.h"
#include "dfn_common.h"
#include "nerfh_handle.h"
#include "nerfh_kernels.h"
#include "nerfh_layout.h"
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

// Kernel variant: DFN_MLP_VARIANT=0..12 (A/B aid; nerfh_layout.h: kVariantFacts, kSelectedByDefault), read once.  8 to 11 are retired
// and mean 12: the same outputs bit for bit, at variant 12's speed.  What a variant means for a call is nerfh_route.h; the gradient paths (render backward, dfn_mlp_fine_saving) run the base variant's / variant 0's plain kernels on
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
  MlpLeanArgs d{};
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
    case kLaunchLean: return launch_mlp_lean(fine, d, cus, s);
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

extern "C" int dfn_ndc_rays_backward(int H, int W, float focal, float near, const float* rays_o, const float* rays_d, size_t n,
                                     const float* grad_ndc_o, const float* grad_ndc_d, float* grad_rays_o, float* grad_rays_d,
                                     void* stream) {
  if (!n) return DFN_OK;
  if (!rays_o || !rays_d || !grad_rays_o || !grad_rays_d || H < 1 || W < 1 || !(focal > 0.f))
    return set_error(DFN_ERR_ARG, "dfn_ndc_rays_backward: bad argument");
  if (!grad_ndc_o && !grad_ndc_d)
    return set_error(DFN_ERR_ARG, "dfn_ndc_rays_backward: bad argument (neither grad_ndc_o nor grad_ndc_d is given)");
  CHECK_HIP(launch_ndc_rays_backward(H, W, focal, near, rays_o, rays_d, n, grad_ndc_o, grad_ndc_d, grad_rays_o, grad_rays_d, HS(stream)),
            "dfn_ndc_rays_backward");
  return DFN_OK;
}

extern "C" int dfn_viewdirs_backward(const float* rays_d, const float* grad_viewdirs, size_t n, int accumulate, float* grad_rays_d,
                                     void* stream) {
  if (!n) return DFN_OK;
  if (!rays_d || !grad_viewdirs || !grad_rays_d) return set_error(DFN_ERR_ARG, "dfn_viewdirs_backward: bad argument (null pointer)");
  CHECK_HIP(launch_viewdirs_backward(rays_d, grad_viewdirs, n, accumulate, grad_rays_d, HS(stream)), "dfn_viewdirs_backward");
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
  const Route r = coarse_route(kPointsVariant, h->desc.width, prec, true);
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
  const Route r = fine_route(kPointsVariant, h->desc.width, prec, false, false, true);
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
