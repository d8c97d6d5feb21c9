// frame_post_maps.hip — render_path's per-frame back-end for the render maps (gfx950), beside frame_post.hip and in a translation
// unit of its own: frame_post.o and every render code object stay what they were.
// render(ret_maps=...) leaves five fp32 maps per frame (models/rendering.py:196-241: depth, depth_static, beta [H,W]; rgb_static,
// rgb_transient [H,W,3]).  What a user looks at, and what a PNG holds, is
//   rgb_static8, rgb_transient8 = to8b(x)                         the truncating conversion of frame_post.hip (models/nerf.py:11)
//   beta8   = to8b(beta / max(beta over the frame))               the convention of disp8
//   depth16, depth_static16 = (uint16)(int)(65535 * clip((d - near) / (far - near), 0, 1))   FIXED scale: metric, comparable across
//                                                                 frames and ranks
//   mse_static = mean((rgb_static - gt)^2)                        the PSNR of the transient-free render
// Pass 1 = per-frame maximum of beta (ordered-integer atomicMax; only when beta is asked for), pass 2 = the conversions + the squared
// error (fp64 block partials, one atomicAdd per block and frame), pass 3 = the two per-frame numbers.  Every fp32 operation is rounded
// on its own (__fsub_rn / __fmul_rn / __fdiv_rn: nothing for the compiler to contract).
// HBM-bound: at most 40 B in (two depths, beta twice, two colours) + 12 B of gt, 11 B out per pixel.  The colour planes are walked as
// flat arrays of 3 H W floats, one plane of H W elements per loop trip, so that every wave load is 256 contiguous bytes and every
// wave store 64 or 128; all accesses are 4-, 2- and 1-byte scalars: a frame starts at f H W elements, which for odd H W is aligned
// to nothing wider.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dfnet_hip.h"
#include "dfn_common.h"

namespace dfn {
namespace maps_post {

struct MapStat { unsigned max_key; unsigned pad; double sse; };   // per frame, in the caller's scratch

// order-preserving map float -> unsigned (atomicMax on the key is max on the float; NaN sorts above +inf): as frame_post.hip
__device__ __forceinline__ unsigned float_key(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_float(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__device__ __forceinline__ float clip01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }   // NaN -> 0 (fmaxf returns the number)
__device__ __forceinline__ uint8_t to8b(float x) { return (uint8_t)(int)__fmul_rn(255.f, clip01(x)); }
__device__ __forceinline__ uint16_t to16(float d, float near, float range) {
  return (uint16_t)(int)__fmul_rn(65535.f, clip01(__fdiv_rn(__fsub_rn(d, near), range)));
}

__global__ __launch_bounds__(256) void beta_max_kernel(const float* __restrict__ beta, size_t hw, MapStat* __restrict__ stat) {
  const float* b = beta + (size_t)blockIdx.y * hw;
  unsigned best = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += (size_t)gridDim.x * blockDim.x) {
    const unsigned k = float_key(b[i]);
    best = k > best ? k : best;
  }
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned o = __shfl_xor(best, off, 64);
    best = o > best ? o : best;
  }
  __shared__ unsigned wbest[4];
  if ((threadIdx.x & 63) == 0) wbest[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) best = wbest[w] > best ? wbest[w] : best;
    atomicMax(&stat[blockIdx.y].max_key, best);
  }
}

struct MapsArgs {
  const float *depth, *depth_static, *beta, *rgb_static, *rgb_transient, *gt;   // inputs (NULL = absent)
  uint16_t *depth16, *depth_static16;                                           // outputs (NULL = not wanted)
  uint8_t *beta8, *rgb_static8, *rgb_transient8;
  size_t hw, gt_stride;   // gt_stride: 3 H W with per-frame gt, 0 with one frame
  float near, far;
  int want_sse;
};

__global__ __launch_bounds__(256) void frame_post_maps_kernel(MapsArgs a, MapStat* __restrict__ stat) {
  const size_t f = blockIdx.y, hw = a.hw;
  const size_t first = (size_t)blockIdx.x * blockDim.x + threadIdx.x, step = (size_t)gridDim.x * blockDim.x;
  const float range = __fsub_rn(a.far, a.near);
  if (a.depth16) {
    const float* d = a.depth + f * hw;
    uint16_t* o = a.depth16 + f * hw;
    for (size_t i = first; i < hw; i += step) o[i] = to16(d[i], a.near, range);
  }
  if (a.depth_static16) {
    const float* d = a.depth_static + f * hw;
    uint16_t* o = a.depth_static16 + f * hw;
    for (size_t i = first; i < hw; i += step) o[i] = to16(d[i], a.near, range);
  }
  if (a.beta8) {
    const float* b = a.beta + f * hw;
    uint8_t* o = a.beta8 + f * hw;
    const float bmax = key_float(stat[f].max_key);
    for (size_t i = first; i < hw; i += step) o[i] = to8b(__fdiv_rn(b[i], bmax));
  }
  if (a.rgb_transient8) {
    const float* r = a.rgb_transient + f * hw * 3;
    uint8_t* o = a.rgb_transient8 + f * hw * 3;
    for (size_t i = first; i < hw; i += step) {
#pragma unroll
      for (int p = 0; p < 3; ++p) o[p * hw + i] = to8b(r[p * hw + i]);   // the flat [3 H W] array, plane p of H W elements
    }
  }
  if (!a.rgb_static8 && !a.want_sse) return;   // (uniform over the block)
  const float* r = a.rgb_static + f * hw * 3;
  uint8_t* o = a.rgb_static8 ? a.rgb_static8 + f * hw * 3 : nullptr;
  const float* g = a.want_sse ? a.gt + f * a.gt_stride : nullptr;
  double sse = 0.0;
  for (size_t i = first; i < hw; i += step) {
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      const float v = r[p * hw + i];
      if (o) o[p * hw + i] = to8b(v);
      if (g) {
        const float e = __fsub_rn(v, g[p * hw + i]);   // fp32 difference as numpy forms it, squared and summed in fp64
        sse += (double)e * (double)e;
      }
    }
  }
  if (!g) return;
  for (int off = 32; off >= 1; off >>= 1) sse += __shfl_xor(sse, off, 64);
  __shared__ double wsum[4];
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = sse;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(&stat[f].sse, wsum[0] + wsum[1] + wsum[2] + wsum[3]);
}

__global__ void frame_post_maps_finish_kernel(const MapStat* __restrict__ stat, int n, double inv_count, float* __restrict__ mse_static,
                                              float* __restrict__ beta_max) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n) return;
  if (mse_static) mse_static[f] = (float)(stat[f].sse * inv_count);
  if (beta_max) beta_max[f] = key_float(stat[f].max_key);
}

}  // namespace maps_post
}  // namespace dfn

extern "C" size_t dfn_frame_post_maps_scratch_bytes(int n_frames) {
  return (size_t)(n_frames > 0 ? n_frames : 1) * sizeof(dfn::maps_post::MapStat);
}

extern "C" int dfn_frame_post_maps(const dfn_render_maps* maps, const float* gt, int gt_per_frame, int n_frames, int H, int W, float near,
                                   float far, const dfn_frame_maps_out* out, float* beta_max, float* mse_static, void* scratch,
                                   void* stream) {
  using namespace dfn;
  using namespace dfn::maps_post;
  if (n_frames == 0) return DFN_OK;
  if (n_frames < 0 || n_frames > 65535 || H < 1 || W < 1 || !scratch)
    return set_error(DFN_ERR_ARG, "dfn_frame_post_maps: bad argument (1 <= n_frames <= 65535, H >= 1, W >= 1, scratch given)");
  if (!(far > near)) return set_error(DFN_ERR_ARG, "dfn_frame_post_maps: far (%g) must be greater than near (%g)", far, near);
  const dfn_render_maps none_in = {nullptr, nullptr, nullptr, nullptr, nullptr};
  const dfn_frame_maps_out none_out = {nullptr, nullptr, nullptr, nullptr, nullptr};
  const dfn_render_maps& m = maps ? *maps : none_in;
  const dfn_frame_maps_out& o = out ? *out : none_out;
  if ((o.depth16 && !m.depth) || (o.depth_static16 && !m.depth_static) || (o.rgb_static8 && !m.rgb_static) ||
      (o.rgb_transient8 && !m.rgb_transient))
    return set_error(DFN_ERR_ARG, "dfn_frame_post_maps: an output is asked for without its map");
  if ((o.beta8 || beta_max) && !m.beta) return set_error(DFN_ERR_ARG, "dfn_frame_post_maps: beta8 / beta_max need maps->beta");
  if (mse_static && (!gt || !m.rgb_static)) return set_error(DFN_ERR_ARG, "dfn_frame_post_maps: mse_static needs gt and maps->rgb_static");
  const bool want_beta = o.beta8 || beta_max;
  const bool want_main = o.depth16 || o.depth_static16 || o.beta8 || o.rgb_static8 || o.rgb_transient8 || mse_static;
  if (!want_beta && !want_main) return DFN_OK;   // nothing asked for: no launch
  hipStream_t s = static_cast<hipStream_t>(stream);
  MapStat* stat = static_cast<MapStat*>(scratch);
  if (hipMemsetAsync(stat, 0, dfn_frame_post_maps_scratch_bytes(n_frames), s) != hipSuccess)
    return set_error(DFN_ERR_HIP, "dfn_frame_post_maps: memset failed");
  const size_t hw = (size_t)H * W;
  const size_t per_block = 256 * 8;   // >= 8 pixels per thread
  const int bx = (int)((hw + per_block - 1) / per_block < 256 ? (hw + per_block - 1) / per_block : 256);
  if (want_beta) hipLaunchKernelGGL(beta_max_kernel, dim3(bx, n_frames), dim3(256), 0, s, m.beta, hw, stat);
  if (want_main) {
    MapsArgs a;
    a.depth = m.depth, a.depth_static = m.depth_static, a.beta = m.beta, a.rgb_static = m.rgb_static, a.rgb_transient = m.rgb_transient;
    a.gt = gt;
    a.depth16 = o.depth16, a.depth_static16 = o.depth_static16, a.beta8 = o.beta8, a.rgb_static8 = o.rgb_static8;
    a.rgb_transient8 = o.rgb_transient8;
    a.hw = hw, a.gt_stride = gt_per_frame ? hw * 3 : 0;
    a.near = near, a.far = far;
    a.want_sse = mse_static ? 1 : 0;
    hipLaunchKernelGGL(frame_post_maps_kernel, dim3(bx, n_frames), dim3(256), 0, s, a, stat);
  }
  if (mse_static || beta_max)
    hipLaunchKernelGGL(frame_post_maps_finish_kernel, dim3((n_frames + 63) / 64), dim3(64), 0, s, stat, n_frames, 1.0 / (double)(hw * 3),
                       mse_static, beta_max);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_error(DFN_ERR_HIP, "dfn_frame_post_maps: %s", hipGetErrorString(e));
  return DFN_OK;
}
