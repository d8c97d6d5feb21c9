// nerfh_kernels.h — internal launch interface between the C ABI (dfn_api.hip) and the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "nerfh_raydiv.h"

namespace dfn {

struct MlpArgs {
  const char* blob;        // packed MFMA fragments of the net (device)
  const uint32_t* tab;     // [n_units][2] = (byte offset, byte size) of each staging unit (device)
  int n_units;
  const float* rays_o;     // [n_rays,3]
  const float* rays_d;     // [n_rays,3]
  const float* z;          // fine: [n_rays, n_samples]; coarse: unused (linspace in-kernel)
  const float* ray_bias;   // fine: [n_rays, kRayBiasFloats]
  float* out;              // coarse: sigma [n_rays, n_samples]; fine: raw [n_rays, n_samples, 9]
  float* partial;          // fine, fused compositing: [n_rays * n_samples / 64][12] per-segment composites (raw unused);
                           // the render-maps flavour (launch_mlp_maps): kMapsRecFloats floats per segment
  long long n_rays;
  int n_samples;
  float near, far;
  unsigned long long* timing;  // DFN_TIMING builds: per-wave cycle counters [total, dma wait, barrier, tile inputs]
  float in_scale;          // split-f16 only: weight scale x activation scale carried by the accumulators (else 1)
  int lindisp;             // coarse: depths linear in disparity instead of depth (rendering.py:272-273)
  int dma_waves;           // waves of a workgroup that issue the weight DMA (0 = the kernel geometry's default, launch_tiles)
  int* status;             // range guard (device int, may be null): bit 0 = an f16 activation overflowed to inf, bit 1 = a
                           // split-f16 hi half saturated (DFN_RANGE_*: dfn_nerfh_range_status)
  uint32_t* masks;         // fine, split-f16, raw output: also record the ReLU signs of every hidden unit for the gradient kernel's
                           // backward-only pass ([tiles][waves][kBwdMaskWords][64 lanes], as BwdArgs::masks); null otherwise
};

constexpr int kMapsRecFloats = 16;   // segment record of the maps flavour: the 9 floats of the plain one, rgb_static at 9..11, rgb_transient at 12..14
hipError_t launch_mlp(bool fine, int prec, int variant, const MlpArgs& a, int n_cu, hipStream_t stream, int width = 128);
// The fine kernel's render-maps flavour (nerfh_mlp_maps.hip): fine = true, a.partial with kMapsRecFloats floats per segment.
hipError_t launch_mlp_maps(bool fine, int prec, int variant, const MlpArgs& a, int n_cu, hipStream_t stream, int width = 128);
// Kernel variant 5's fine kernel (nerfh_mlp_fold.hip): split-f16, netwidth 128, the blob packed along kFineFoldSeq and a.ray_bias
// written from the folded per-ray-bias weights (dfn_nerfh_s::rb_fold).  maps: the render-maps flavour, as launch_mlp_maps.
hipError_t launch_mlp_fold(bool maps, const MlpArgs& a, int n_cu, hipStream_t stream);
// Kernel variant 6 (nerfh_mlp_half.hip): variant 5's kernels with half-height head M-blocks, on the networks packed for them
// (Packer::half_heads).  Coarse (fine = false), or the fine kernel with the compositing fused (a.partial set; maps as above): the
// plain flavour leaves 0 in the segment record's beta slot.  The raw route stays with launch_mlp_fold.
hipError_t launch_mlp_half(bool fine, bool maps, const MlpArgs& a, int n_cu, hipStream_t stream);
// Kernel variant 7 (nerfh_mlp_res.hip): variant 6's coarse kernel and plain fused fine kernel with the layers of kCoarseResident /
// kFineResident held in LDS.  blob / tab / n_units describe the STREAMED units only; res_blob is the resident set in execution order,
// res_bytes = resident_bytes<PrecX3M16>(fine) (zero-padded to whole pieces).  The two fields ride behind MlpArgs in a struct of the
// new kernels' own: a longer MlpArgs would move the hidden kernel arguments (gridDim) of every other kernel and with them their code.
struct MlpResArgs : MlpArgs {
  const char* res_blob;
  uint32_t res_bytes;
};
hipError_t launch_mlp_res(bool fine, const MlpResArgs& a, int n_cu, hipStream_t stream);
// Kernel variant 12 (nerfh_mlp_lean.hip): variant 7's two kernels with per-tile work that the result does not need taken out.  What the
// caller owes them beyond variant 7's arguments:
//   tile_counter  The tiles are claimed dynamically: a workgroup starts on tile blockIdx.x and takes every later one as gridDim.x +
//                 atomicAdd(tile_counter, 1); *tile_counter (device) must be 0 when the kernel starts and belongs to this launch alone
//                 until it ends.
//   ray_bias      fine = true: the per-ray table already holds in_scale x the seeds (launch_ray_bias with scale = a.in_scale): the
//                 RAYBIAS layers take the loaded seeds as they are.  No other kernel reads such a table.
//   div           The magic number by which the kernels turn a point index into a ray index (nerfh_raydiv.h).  The caller leaves it
//                 alone: the launcher forms it from n_samples.
// The fields ride behind MlpResArgs in a struct of the kernels' own, for the reason given there.
struct MlpLeanArgs : MlpResArgs {
  uint32_t* tile_counter;
  RayDiv div;   // ray_div_of(n_samples), filled in by launch_mlp_lean
};
hipError_t launch_mlp_lean(bool fine, const MlpLeanArgs& a, int n_cu, hipStream_t stream);

// The points flavour (nerfh_mlp_pts*.hip): a.rays_o is pts [n_rays, n_samples, 3] (n_rays = query rows), a.rays_d, a.z and a.partial
// are unused (a.partial must be null: the raw route only), a.ray_bias has one row per query row.  launch_mlp_pts: f16 / exact fp32 at
// netwidth 128 (variant 0's kernels) and netwidth 256; split-f16 at netwidth 128: launch_mlp_pts_half = variant 6's coarse kernel
// (net[0][F16X3][6]), launch_mlp_pts_fold = variant 5's fine kernel (net[1][F16X3][5], a.ray_bias from rb_fold).
hipError_t launch_mlp_pts(bool fine, int prec, const MlpArgs& a, int n_cu, hipStream_t stream, int width = 128);
hipError_t launch_mlp_pts_fold(const MlpArgs& a, int n_cu, hipStream_t stream);
hipError_t launch_mlp_pts_half(const MlpArgs& a, int n_cu, hipStream_t stream);
// The coarse network's training query on points (nerfh_mlp_static_pts*.hip, nerfw.py:47-60): the fine points kernel cut off behind
// static_rgb.  a as for the points flavour; a.blob = the coarse network packed along kCoarseStaticSeq (launch_mlp_static_pts: f16 /
// exact fp32 at netwidth 128, netwidth 256) or kCoarseStaticFoldSeq (launch_mlp_static_pts_fold: split-f16 at netwidth 128);
// a.ray_bias = one row of ray_bias_floats(W) floats per query row whose table 0 holds b_dir + W_dir[:, W:W+27] . pe_dir(v) of the
// COARSE dir_encoding.0 (the folded kernel: + W_dir[:, :W] . b_final), table 1 is not read; a.out = raw4 [n_rays, n_samples, 4].
hipError_t launch_mlp_static_pts(int prec, const MlpArgs& a, int n_cu, hipStream_t stream, int width = 128);
hipError_t launch_mlp_static_pts_fold(const MlpArgs& a, int n_cu, hipStream_t stream);

// --- stages (nerfh_stages.hip)
// (frames > 1: c2w [frames,3,4], outputs [frames,H,W,3] — one launch for the frames of a mini-batch)
hipError_t launch_raygen(int H, int W, float focal, const float* c2w, float* rays_o, float* rays_d,
                         float* viewdirs, hipStream_t stream, int frames = 1);
hipError_t launch_viewdirs(const float* rays_d, size_t n, float* viewdirs, hipStream_t stream);
hipError_t launch_ndc_rays(int H, int W, float focal, float near, const float* rays_o, const float* rays_d, size_t n, float* out_o,
                           float* out_d, hipStream_t stream);
// the adjoints of ndc_rays (grad_ndc_o / grad_ndc_d: either may be nullptr = zeros; outputs must not alias inputs) and of v = d / |d|
hipError_t launch_ndc_rays_backward(int H, int W, float focal, float near, const float* rays_o, const float* rays_d, size_t n,
                                    const float* grad_ndc_o, const float* grad_ndc_d, float* grad_rays_o, float* grad_rays_d,
                                    hipStream_t stream);
hipError_t launch_viewdirs_backward(const float* rays_d, const float* grad_viewdirs, size_t n, int accumulate, float* grad_rays_d,
                                    hipStream_t stream);
hipError_t launch_posenc(const float* x, size_t n, int L, int mode, float* out, hipStream_t stream);

struct RayBiasWeights {       // device pointers, fp32
  const float* w_dir;         // [77][nout]  transposed dir_encoding.0.weight[:, W:W+77]
  const float* b_dir;         // [nout]
  const float* w_tr;          // [20][nout]  transposed transient_encoding.0.weight[:, W:W+20]
  const float* b_tr;          // [nout]
  const float* emb_a;         // [n_vocab, dim_a]
  const float* emb_t;         // [n_vocab, dim_t]
  int hist_bin, dim_a, dim_t, n_vocab;
  int nout;                   // outputs per table = netwidth / 2 (w_dir, w_tr are [*][nout]; the table row is 2 * nout floats)
};
// scale: every table entry is stored multiplied by it (1 = the seeds themselves, the kernel every route but variant 12's fused fine
// one has always run; otherwise the fine network's in_scale, a power of two: launch_mlp_lean)
hipError_t launch_ray_bias(const RayBiasWeights& w, const float* viewdirs, const float* hist,
                           size_t hist_rows, size_t n_rays, float* table, hipStream_t stream, float scale = 1.f);

hipError_t launch_coarse_weights(const float* sigma, const float* z, size_t n, int N, float* weights,
                                 hipStream_t stream);
hipError_t launch_sample_pdf(const float* bins, const float* weights, size_t n, int nb, int Ni,
                             const float* u, float* out, hipStream_t stream);
// Backward of launch_sample_pdf (grad_out [n, Ni] -> grad_bins [n, nb], grad_weights [n, nb-1], grad_u [n, Ni]; a NULL output is
// skipped).  Its LDS need is sample_pdf_backward_lds_bytes(nb, Ni) per block; a shape above kSamplePdfBackwardMaxLds (what a kernel may
// ask for without an attribute) is hipErrorInvalidValue, never a launch.
constexpr size_t kSamplePdfBackwardMaxLds = 64 * 1024;
size_t sample_pdf_backward_lds_bytes(int nb, int Ni);
hipError_t launch_sample_pdf_backward(const float* bins, const float* weights, size_t n, int nb, int Ni, const float* u,
                                      const float* grad_out, float* grad_bins, float* grad_weights, float* grad_u, hipStream_t stream);
hipError_t launch_sample_fine(const float* sigma, size_t n_rays, int Nc, int Ni, float near, float far,
                              float* z_fine, float* weights_coarse, float* z_samples, hipStream_t stream, int lindisp = 0);
hipError_t launch_composite_fine(const float* raw, const float* z, size_t n_rays, int Nf, float beta_min,
                                 int flags, float* rgb, float* disp, float* acc, float* depth,
                                 float* weights, float* beta, hipStream_t stream);

// Chains the per-64-sample segment composites written by the fused fine kernel: partial [n_rays, segs, 12].
hipError_t launch_composite_combine(const float* partial, size_t n_rays, int segs, float beta_min, int flags, float* rgb,
                                    float* disp, float* acc, hipStream_t stream);

// Render maps (dfn_render_maps): optional per-ray outputs beside rgb / disp / acc, each null when not wanted.
struct MapPtrs {
  float *depth, *depth_static, *beta, *rgb_static, *rgb_transient;
  bool any() const { return depth || depth_static || beta || rgb_static || rgb_transient; }
  MapPtrs at(size_t ray) const {   // the same maps from ray `ray` on
    return MapPtrs{depth ? depth + ray : nullptr, depth_static ? depth_static + ray : nullptr, beta ? beta + ray : nullptr,
                   rgb_static ? rgb_static + ray * 3 : nullptr, rgb_transient ? rgb_transient + ray * 3 : nullptr};
  }
};
// The maps from raw [n_rays, Nf, 9] and z [n_rays, Nf] in HBM (the non-fused routes and the stage on its own).
hipError_t launch_composite_fine_maps(const float* raw, const float* z, size_t n_rays, int Nf, float beta_min, const MapPtrs& maps,
                                      hipStream_t stream);
// launch_composite_combine over the maps flavour's records (partial [n_rays, segs, kMapsRecFloats]): the same rgb / disp / acc, and
// the requested maps.
hipError_t launch_composite_combine_maps(const float* partial, size_t n_rays, int segs, float beta_min, int flags, float* rgb,
                                         float* disp, float* acc, const MapPtrs& maps, hipStream_t stream);

// --- gradient path (nerfh_bwd.hip, nerfh_stages.hip)
struct BwdArgs {
  const char* blob;        // forward fine units followed by the backward (W^T) units
  const uint32_t* tab;
  int n_units;
  const float* rays_o;     // [n_rays,3]
  const float* rays_d;     // [n_rays,3]
  const float* viewdirs;   // [n_rays,3]
  const float* z;          // [n_rays, n_samples]
  const float* ray_bias;   // [n_rays, kRayBiasFloats]
  const float* graw;       // [n_rays, n_samples, 9]  d L / d raw
  float* gpts;             // [n_rays, n_samples, 6]  d L / d point (3), d L / d viewdir via this sample (3)
  long long n_rays;
  int n_samples;
  float in_scale;          // split-f16 forward units: scale carried by the accumulators (else 1)
  // Two-pass form (mode 1 = forward, writing raw and the ReLU masks; mode 2 = backward from them, no forward recompute):
  float* raw_out;          // mode 1: [n_rays, n_samples, 9]
  const float* raw_in;     // mode 2
  uint32_t* masks;         // [tiles][waves][kBwdMaskWords][64 lanes]: written by mode 1, read by mode 2
};
constexpr int kBwdMaskWords = 21;    // 8 trunk layers x 128 bits, dir_encoding 64, transient_encoding 4 x 64 — per point
constexpr int kBwdTilePoints = 256;  // points per workgroup tile of the split-f16 gradient kernel (8 waves x 32)
hipError_t launch_mlp_fine_backward(int prec, const BwdArgs& a, int n_cu, hipStream_t stream, int mode = 0);
// Its points flavour (nerfh_bwd_pts.hip): a.rays_o is pts [n_rays, n_samples, 3], a.rays_d and a.z are unused; the one-pass form only.
hipError_t launch_mlp_fine_backward_pts(int prec, const BwdArgs& a, int n_cu, hipStream_t stream, int mode = 0);
// The coarse network's input gradient, points flavour (nerfh_bwd_coarse_pts.hip: nerfh_coarse_backward_pts_kernel): a.blob = the coarse
// forward units followed by the backward units of kBwdCoarseSeq, a.rays_o = pts [n_rays, n_samples, 3], a.graw = d L / d sigma
// [n_rays, n_samples] (ONE float per point), a.gpts = d L / d point [n_rays, n_samples, 3]; a.rays_d, a.viewdirs, a.z and a.ray_bias are
// unused (sigma depends on the point alone).  The one-pass form only.
hipError_t launch_mlp_coarse_backward_pts(int prec, const BwdArgs& a, int n_cu, hipStream_t stream, int mode = 0);
// The input gradient of the coarse network's training query, points flavour (nerfh_bwd_coarse_static_pts.hip:
// nerfh_coarse_static_backward_pts_kernel): a.blob = the coarse network's forward units along kCoarseStaticSeq followed by the backward
// units of kBwdCoarseStaticSeq, a.rays_o = pts [n_rays, n_samples, 3], a.viewdirs [n_rays, 3], a.ray_bias = the coarse dir_encoding.0's
// seed table (launch_mlp_static_pts's, unfolded), a.graw = d L / d raw4 [n_rays, n_samples, 4], a.gpts [n_rays, n_samples, 6] as the
// fine kernel's; a.rays_d and a.z are unused.  The one-pass form only.
hipError_t launch_mlp_coarse_static_backward_pts(int prec, const BwdArgs& a, int n_cu, hipStream_t stream, int mode = 0);
// d L / d raw from d L / d rgb through the fine compositing (test-time, rgb only).  grad_raw_ext [n_rays, Nf, 9] (optional): a
// gradient that reaches raw directly, added in the same kernel (graw = d raw(compositor) + grad_raw_ext); with grad_rgb == nullptr
// graw = grad_raw_ext and the scan is skipped.  Without it: the rgb-only kernel, unchanged.
hipError_t launch_composite_fine_backward(const float* raw, const float* z, const float* grad_rgb, size_t n_rays, int Nf,
                                          float* graw, hipStream_t stream, const float* grad_raw_ext = nullptr);
// Upstream gradients of every output of the fine compositor (dfn_map_grads), each optional (null = zero): rgb, rgb_static,
// rgb_transient [n_rays,3]; the others [n_rays].
struct MapGrads {
  const float *rgb, *acc, *depth, *depth_static, *disp, *beta, *rgb_static, *rgb_transient;
  bool any() const { return rgb || acc || depth || depth_static || disp || beta || rgb_static || rgb_transient; }
};
// d L / d raw summed over all of them (nerfh_maps_bwd.hip); grad_raw_ext as in launch_composite_fine_backward.  Every pointer of g null:
// graw = grad_raw_ext (an error without it).  launch_composite_fine_backward and its kernel are not involved.
hipError_t launch_composite_fine_backward_all(const float* raw, const float* z, size_t n_rays, int Nf, float beta_min, const MapGrads& g,
                                              float* graw, hipStream_t stream, const float* grad_raw_ext = nullptr);
// Per-ray reduction of the per-sample gradients: d o = sum g, d d = sum z g (+ viewdir normalisation when
// `derive_viewdirs`), d viewdirs = sum gv (when grad_viewdirs != nullptr).  accumulate: add to what grad_o / grad_d
// (and grad_viewdirs) hold.
hipError_t launch_ray_grad_reduce(const float* gpts, const float* z, const float* rays_d, size_t n_rays, int Nf,
                                  int derive_viewdirs, float* grad_o, float* grad_d, float* grad_viewdirs,
                                  hipStream_t stream, int accumulate = 0);
// get_rays backward: d c2w[3][4] from d rays_o / d rays_d of an H x W image.
hipError_t launch_raygen_backward(int H, int W, float focal, const float* grad_o, const float* grad_d, float* grad_c2w,
                                  hipStream_t stream, int frames = 1);
// adjoint of launch_bicubic: g_out [UH,UW,C] -> g_in [H,W,C].
// (frames > 1: a batch of frames per launch; nchw: the enlarged frames — g_out for the adjoint — are planar [C,UH,UW] per frame)
hipError_t launch_bicubic_backward(const float* gout, int H, int W, int C, int UH, int UW, float* gin, hipStream_t stream, int frames = 1,
                                   bool nchw = false);
hipError_t launch_bicubic(const float* in, int H, int W, int C, int UH, int UW, float* out, hipStream_t stream, int frames = 1,
                          bool nchw = false);

}  // namespace dfn
