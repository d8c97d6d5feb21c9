// nerfh_raw2outputs.hip — raw2outputs_NeRFW as a public stage (gfx950): the compositor of models/rendering.py:132-243 in all three of
// its arithmetic modes, forward and backward, differentiable with respect to raw AND z_vals (dfn_raw2outputs,
// dfn_raw2outputs_backward).  A translation unit of its own: the compositing kernels of render() (nerfh_stages.hip,
// nerfh_maps_bwd.hip, nerfh_train_maps.hip) are not involved, except that the 9-channel forward IS launch_composite_fine.
//
//   M1  ch = 1  typ == "coarse" and test_time (:140-142, :188-193): raw = sigma; acc and weights only
//   M2  ch = 4  output_transient == False otherwise (:144-152, :173-174, :232-243): raw = (rgb, sigma)
//   M3  ch = 9  output_transient == True (:153-156, :168-171, :195-230, :241-243): static + transient field
// In every mode delta_i = z_{i+1} - z_i, the last delta is 1e2, no |d| factor (:161-166).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dfnet_hip.h"
#include "dfn_common.h"
#include "nerfh_device.h"
#include "nerfh_kernels.h"

namespace dfn {

typedef float f32x4_t __attribute__((ext_vector_type(4)));
constexpr int kStagedFlag = 8;   // launcher -> kernel, as in launch_composite_fine: raw / grad_raw rows go through LDS

// ------------------------------------------------------------------------------------------ forward, M1 and M2
// alpha = 1 - exp(-delta relu(sigma + noise_std noise)) (:173-174), w = alpha T (:176-186), rgb = sum w c (+ 1 - acc, :233-236),
// depth = sum w z, disp = 1 / max(1e-10, depth / sum w) (:241-242).  One wavefront per ray, SPL consecutive samples per lane, the
// rounding of composite_fine_kernel (every product and difference on its own).  Every output pointer is optional.
template <int SPL, int CH>
__global__ __launch_bounds__(256) void raw2outputs_static_kernel(const float* __restrict__ raw, const float* __restrict__ z,
                                                                 const float* __restrict__ noise, float noise_std, size_t n_rays,
                                                                 int N, int flags, float* __restrict__ rgb, float* __restrict__ disp,
                                                                 float* __restrict__ acc, float* __restrict__ weights,
                                                                 float* __restrict__ depth) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool white = CH == 4 && (flags & DFN_COMP_WHITE_BKGD);
  for (size_t ray = size_t(blockIdx.x) * 4 + wave; ray < n_rays; ray += size_t(gridDim.x) * 4) {
    const float* rr = raw + ray * size_t(N) * CH;
    const float* zr = z + ray * size_t(N);
    const float* nr = noise ? noise + ray * size_t(N) : nullptr;
    float v[SPL][CH], zz[SPL + 1];
#pragma unroll
    for (int k = 0; k < SPL; ++k) {
      const int i = lane * SPL + k;
      zz[k] = i < N ? zr[i] : 0.f;
#pragma unroll
      for (int c = 0; c < CH; ++c) v[k][c] = i < N ? rr[size_t(i) * CH + c] : 0.f;
      if (nr && i < N) v[k][CH - 1] = add_rn(v[k][CH - 1], mul_rn(nr[i], noise_std));
    }
    zz[SPL] = __shfl_down(zz[0], 1, 64);
    float al[SPL], p = 1.f;
#pragma unroll
    for (int k = 0; k < SPL; ++k) {
      const int i = lane * SPL + k;
      const float delta = i + 1 < N ? sub_rn(zz[k + 1], zz[k]) : 1e2f;
      al[k] = i < N ? sub_rn(1.f, expf(-mul_rn(delta, fmaxf(v[k][CH - 1], 0.f)))) : 0.f;
      p = mul_rn(p, sub_rn(1.f, al[k]));
    }
    float T = __shfl_up(wave_incl_prod(p, lane), 1, 64);
    if (lane == 0) T = 1.f;
    float s_rgb[3] = {0.f, 0.f, 0.f}, s_acc = 0.f, s_depth = 0.f;
#pragma unroll
    for (int k = 0; k < SPL; ++k) {
      const int i = lane * SPL + k;
      const float w = mul_rn(al[k], T);
      if constexpr (CH == 4) {
#pragma unroll
        for (int c = 0; c < 3; ++c) s_rgb[c] += mul_rn(w, v[k][c]);
        s_depth += mul_rn(w, zz[k]);
      }
      s_acc += w;
      if (weights && i < N) weights[ray * size_t(N) + i] = w;
      T = mul_rn(T, sub_rn(1.f, al[k]));
    }
    s_acc = wave_sum(s_acc);
    if constexpr (CH == 4) {
#pragma unroll
      for (int c = 0; c < 3; ++c) s_rgb[c] = wave_sum(s_rgb[c]);
      s_depth = wave_sum(s_depth);
    }
    if (lane == 0) {
      if (acc) acc[ray] = s_acc;
      if constexpr (CH == 4) {
        const float bg = white ? 1.f - s_acc : 0.f;
        if (rgb) {
#pragma unroll
          for (int c = 0; c < 3; ++c) rgb[ray * 3 + c] = s_rgb[c] + bg;
        }
        if (disp) disp[ray] = 1.f / fmaxf(1e-10f, s_depth / s_acc);
        if (depth) depth[ray] = s_depth;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ backward, all three modes
// Upstream gradients of the outputs raw2outputs_NeRFW returns; each optional (null = zero).  weights is dense [n_rays, N].
struct R2OGrads {
  const float *rgb, *disp, *acc, *weights, *depth, *beta;
};

// Per sample i with interval d_i, x_i = d_i s_i the exponent of the static field (s_i = relu(sigma_i + noise_i) in M1 / M2, sigma_s
// in M3) and y_i = d_i sigma_t that of the transient one (M3 only):
//   o_s = exp(-x)   o_t = exp(-y)   o = exp(-(x + y))      (1 - alpha_s, 1 - alpha_t, 1 - alpha: the exponentials themselves)
//   T_i = prod_{j<i} o_j      U_i = prod_{j<i} o_s,j  (the static field alone: the depth of test_time and static_only, :218-228)
//   rgb = sum T ((1 - o_s) c_s + (1 - o_t) c_t) [+ 1 - acc]   w_i = T_i (1 - o_i)   acc = sum w   beta = sum T (1 - o_t) b + beta_min
//   depth = sum w z,  or  sum U (1 - o_s) z  under test_time and static_only        disp = 1 / max(1e-10, depth / acc)
// disp and the white background are functions of the other outputs and are folded into their upstream gradients per ray, before the
// scans: g_acc -= sum_c g_rgb[c] (white);  where depth / acc > 1e-10, g_acc += g_disp / depth and g_depth -= g_disp acc / depth^2.
// With the per-sample coefficients
//   js = g_rgb.c_s    jt = g_rgb.c_t + g_beta b    ja = g_w,i + g_depth z_i    ss = 0       (joint depth)
//                                                  ja = g_w,i                  ss = g_depth z_i   (static-only depth)
// and the emitted terms e_i = T_i ((1 - o_s) js + (1 - o_t) jt + (1 - o) ja), f_i = U_i (1 - o_s) ss, E_i = sum_{k>i} e_k, F_i likewise:
//   d L / d x_i = T (o_s js + o ja) - E_i + g_acc T_end + U o_s ss - F_i        d L / d y_i = T (o_t jt + o ja) - E_i + g_acc T_end
// (acc = 1 - T_end in closed form: d acc / d x_i = T_end for every sample; M1 / M2 are the case y = 0, c_t = b = 0, o = o_s), then
//   d sigma_s = d_i dL/dx_i (exactly 0 behind a closed relu gate)     d sigma_t = d_i dL/dy_i
//   d delta_i = s_i dL/dx_i + sigma_t,i dL/dy_i  for i < N - 1 (the last interval is a constant)
//   d z_i = d delta_{i-1} - d delta_i + g_depth w_i    (w_i = U_i (1 - o_s,i) under the static-only depth): the one exchange with the
//           neighbouring sample, across the samples of a lane and across lanes.
// Numerical rules as in nerfh_maps_bwd.hip: nothing is divided by an exponential (opaque samples, duplicate depths and N = 1 give
// finite results), E_i and F_i are added up from the far end, and g_acc enters in its closed form only.
// With nine channels a lane's SPL samples are 9 SPL floats at a stride of 36 SPL bytes across lanes; as in composite_fine_kernel the
// ray's row of raw is therefore staged through LDS with 16-byte coalesced loads, and the row of grad_raw leaves through the same buffer
// (the launcher's decision, kStagedFlag: 16-byte aligned rows that fit the default dynamic LDS).  Four channels are one aligned
// 16 bytes per sample and need none.
template <int SPL, int CH>
__global__ __launch_bounds__(256) void raw2outputs_backward_kernel(const float* __restrict__ raw, const float* __restrict__ z,
                                                                   const float* __restrict__ noise, float noise_std, const R2OGrads g,
                                                                   size_t n_rays, int N, int flags, float* __restrict__ graw,
                                                                   float* __restrict__ gz) {
  constexpr int SG = CH == 9 ? 3 : CH - 1;   // the channel of the static sigma
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool static_depth = CH == 9 && (flags & DFN_COMP_TEST_TIME) && (flags & DFN_COMP_STATIC_ONLY);
  const bool white = CH != 1 && (flags & DFN_COMP_WHITE_BKGD);
  extern __shared__ __attribute__((aligned(16))) float r2o_rows[];   // per wave: one ray's raw, then its grad_raw [N][9] (when staged)
  const bool staged = CH == 9 && (flags & kStagedFlag);
  float* sr = r2o_rows + size_t(wave) * N * CH;
  for (size_t ray = size_t(blockIdx.x) * 4 + wave; ray < n_rays; ray += size_t(gridDim.x) * 4) {
    const float* rr = raw + ray * size_t(N) * CH;
    const float* zr = z + ray * size_t(N);
    if (staged) {
      const f32x4_t* src = reinterpret_cast<const f32x4_t*>(rr);
      f32x4_t* dst = reinterpret_cast<f32x4_t*>(sr);
      for (int i = lane; i < N * CH / 4; i += 64) dst[i] = src[i];
      wave_sync();
    }
    const float* nr = (CH != 9 && noise) ? noise + ray * size_t(N) : nullptr;
    const float* wr = g.weights ? g.weights + ray * size_t(N) : nullptr;
    float g_rgb[3] = {0.f, 0.f, 0.f}, g_depth = 0.f, g_disp = 0.f, g_beta = 0.f;
    float g_acc = g.acc ? g.acc[ray] : 0.f;
    if constexpr (CH != 1) {
#pragma unroll
      for (int c = 0; c < 3; ++c) g_rgb[c] = g.rgb ? g.rgb[ray * 3 + c] : 0.f;
      g_depth = g.depth ? g.depth[ray] : 0.f;
      g_disp = g.disp ? g.disp[ray] : 0.f;
      if (white) g_acc -= g_rgb[0] + g_rgb[1] + g_rgb[2];
    }
    if constexpr (CH == 9) g_beta = g.beta ? g.beta[ray] : 0.f;
    float v[SPL][CH], zz[SPL + 1], gw[SPL];
    bool gate[SPL];   // M1 / M2: the relu of sigma + noise is open
#pragma unroll
    for (int k = 0; k < SPL; ++k) {
      const int i = lane * SPL + k;
      zz[k] = i < N ? zr[i] : 0.f;
      gw[k] = (wr && i < N) ? wr[i] : 0.f;
#pragma unroll
      for (int c = 0; c < CH; ++c) v[k][c] = i < N ? (staged ? sr[i * CH + c] : rr[size_t(i) * CH + c]) : 0.f;
      if constexpr (CH != 9) {
        if (nr && i < N) v[k][SG] = add_rn(v[k][SG], mul_rn(nr[i], noise_std));
        gate[k] = v[k][SG] > 0.f;
        v[k][SG] = fmaxf(v[k][SG], 0.f);
      } else {
        gate[k] = true;
      }
    }
    if (staged) wave_sync();   // the row is in registers: the buffer is free for grad_raw
    zz[SPL] = __shfl_down(zz[0], 1, 64);
    float dl[SPL], os[SPL], ot[SPL], om[SPL];
    float pj = 1.f, ps = 1.f;
#pragma unroll
    for (int k = 0; k < SPL; ++k) {
      const int i = lane * SPL + k;
      const bool ok = i < N;
      dl[k] = i + 1 < N ? sub_rn(zz[k + 1], zz[k]) : 1e2f;
      os[k] = ok ? expf(-mul_rn(dl[k], v[k][SG])) : 1.f;
      if constexpr (CH == 9) {
        ot[k] = ok ? expf(-mul_rn(dl[k], v[k][7])) : 1.f;
        om[k] = ok ? expf(-mul_rn(dl[k], add_rn(v[k][3], v[k][7]))) : 1.f;
        ps = mul_rn(ps, os[k]);
      } else {
        ot[k] = 1.f;
        om[k] = os[k];
      }
      pj = mul_rn(pj, om[k]);
    }
    const float incl = wave_incl_prod(pj, lane);
    const float T_end = __shfl(incl, 63, 64);   // the transmittance behind the last sample
    float Tj = __shfl_up(incl, 1, 64), Us = 1.f;
    if constexpr (CH == 9) Us = __shfl_up(wave_incl_prod(ps, lane), 1, 64);
    if (lane == 0) Tj = Us = 1.f;
    float T[SPL], U[SPL];
#pragma unroll
    for (int k = 0; k < SPL; ++k) {
      T[k] = Tj;
      U[k] = Us;
      Tj = mul_rn(Tj, om[k]);
      if constexpr (CH == 9) Us = mul_rn(Us, os[k]);
    }
    if (CH != 1 && g.disp) {   // (uniform) disp = acc / depth where depth / acc > 1e-10: fold its gradient into those two
      float s_acc = 0.f, s_dep = 0.f;
#pragma unroll
      for (int k = 0; k < SPL; ++k) {
        s_acc += (1.f - om[k]) * T[k];
        s_dep += (static_depth ? (1.f - os[k]) * U[k] : (1.f - om[k]) * T[k]) * zz[k];
      }
      s_acc = wave_sum(s_acc);
      s_dep = wave_sum(s_dep);
      if (g_disp != 0.f && s_dep / s_acc > 1e-10f) {
        const float inv = 1.f / s_dep;
        g_acc += g_disp * inv;
        g_depth -= g_disp * s_acc * inv * inv;
      }
    }
    const float tail = g_acc * T_end;
    const float gd_j = static_depth ? 0.f : g_depth, gd_s = static_depth ? g_depth : 0.f;   // g_depth on the joint / static-only weights
    float e[SPL], f[SPL], esum = 0.f, fsum = 0.f;
#pragma unroll
    for (int k = 0; k < SPL; ++k) {
      const float ja = gw[k] + gd_j * zz[k];
      if constexpr (CH == 9) {
        const float js = g_rgb[0] * v[k][0] + g_rgb[1] * v[k][1] + g_rgb[2] * v[k][2];
        const float jt = g_rgb[0] * v[k][4] + g_rgb[1] * v[k][5] + g_rgb[2] * v[k][6] + g_beta * v[k][8];
        e[k] = T[k] * ((1.f - os[k]) * js + (1.f - ot[k]) * jt + (1.f - om[k]) * ja);
        f[k] = U[k] * (1.f - os[k]) * (gd_s * zz[k]);
      } else {
        float j = ja;
        if constexpr (CH == 4) j += g_rgb[0] * v[k][0] + g_rgb[1] * v[k][1] + g_rgb[2] * v[k][2];
        e[k] = T[k] * (1.f - om[k]) * j;
        f[k] = 0.f;
      }
      esum += e[k];
      fsum += f[k];
    }
    // E_i, F_i: sums over the samples strictly after i, added up from the far end (never `total - prefix`); e / f are overwritten.
    {
      float le = __shfl_down(wave_incl_suffix_sum(esum, lane), 1, 64);   // the lanes after this one
      float lf = CH == 9 ? __shfl_down(wave_incl_suffix_sum(fsum, lane), 1, 64) : 0.f;
      if (lane == 63) le = lf = 0.f;
#pragma unroll
      for (int k = SPL - 1; k >= 0; --k) {
        const float ek = e[k], fk = f[k];
        e[k] = le;
        f[k] = lf;
        le += ek;
        lf += fk;
      }
    }
    const bool want_z = gz != nullptr;   // (uniform)
    float dd[SPL], dzw[SPL];   // d L / d delta_i (0 for the last, constant interval and beyond the ray); g_depth x the depth's weight
#pragma unroll
    for (int k = 0; k < SPL; ++k) {
      const int i = lane * SPL + k;
      const float ja = gw[k] + gd_j * zz[k];
      const float w = T[k] * (1.f - om[k]);
      float r[CH], dxs, dxt = 0.f;
      if constexpr (CH == 9) {
        const float js = g_rgb[0] * v[k][0] + g_rgb[1] * v[k][1] + g_rgb[2] * v[k][2];
        const float jt = g_rgb[0] * v[k][4] + g_rgb[1] * v[k][5] + g_rgb[2] * v[k][6] + g_beta * v[k][8];
        const float ws = T[k] * (1.f - os[k]), wt = T[k] * (1.f - ot[k]), us = U[k] * (1.f - os[k]);
        dxs = T[k] * (os[k] * js + om[k] * ja) - e[k] + tail + (U[k] * os[k] * (gd_s * zz[k]) - f[k]);
        dxt = T[k] * (ot[k] * jt + om[k] * ja) - e[k] + tail;
        r[0] = g_rgb[0] * ws; r[1] = g_rgb[1] * ws; r[2] = g_rgb[2] * ws;
        r[3] = dl[k] * dxs;
        r[4] = g_rgb[0] * wt; r[5] = g_rgb[1] * wt; r[6] = g_rgb[2] * wt;
        r[7] = dl[k] * dxt;
        r[8] = g_beta * wt;
        dd[k] = want_z ? v[k][3] * dxs + v[k][7] * dxt : 0.f;
        dzw[k] = want_z ? (static_depth ? g_depth * us : g_depth * w) : 0.f;
      } else {
        float j = ja;
        if constexpr (CH == 4) {
          j += g_rgb[0] * v[k][0] + g_rgb[1] * v[k][1] + g_rgb[2] * v[k][2];
          r[0] = g_rgb[0] * w; r[1] = g_rgb[1] * w; r[2] = g_rgb[2] * w;
        }
        dxs = T[k] * om[k] * j - e[k] + tail;
        r[SG] = gate[k] ? dl[k] * dxs : 0.f;
        dd[k] = want_z ? v[k][SG] * dxs : 0.f;
        dzw[k] = want_z ? g_depth * w : 0.f;
      }
      if (i + 1 >= N) dd[k] = 0.f;
      if (graw && i < N) {
        float* o = staged ? sr + i * CH : graw + (ray * size_t(N) + i) * CH;
#pragma unroll
        for (int c = 0; c < CH; ++c) o[c] = r[c];
      }
    }
    if (staged && graw) {
      wave_sync();
      const f32x4_t* src = reinterpret_cast<const f32x4_t*>(sr);
      f32x4_t* dst = reinterpret_cast<f32x4_t*>(graw + ray * size_t(N) * CH);
      for (int i = lane; i < N * CH / 4; i += 64) dst[i] = src[i];
      wave_sync();   // the next ray's staging overwrites the buffer
    }
    if (want_z) {
      float prev = __shfl_up(dd[SPL - 1], 1, 64);   // d delta_{i-1} of this lane's first sample: the last sample of the lane before
      if (lane == 0) prev = 0.f;
#pragma unroll
      for (int k = 0; k < SPL; ++k) {
        const int i = lane * SPL + k;
        if (i < N) gz[ray * size_t(N) + i] = (prev - dd[k]) + dzw[k];
        prev = dd[k];
      }
    }
  }
}

namespace {

dim3 ray_grid(size_t n_rays) {
  const size_t quads = (n_rays + 3) / 4;
  return dim3(unsigned(quads < 256 * 16 ? quads : 256 * 16));
}

// The samples-per-lane instantiations of the other compositing kernels: 1, 2, 3, 4, 6, 8 (N <= 512).
#define DFN_R2O_SPL(LAUNCH)         \
  do {                              \
    const int spl = (N + 63) / 64;  \
    if (spl <= 1) LAUNCH(1);        \
    else if (spl == 2) LAUNCH(2);   \
    else if (spl == 3) LAUNCH(3);   \
    else if (spl == 4) LAUNCH(4);   \
    else if (spl <= 6) LAUNCH(6);   \
    else if (spl <= 8) LAUNCH(8);   \
    else return hipErrorInvalidValue; \
  } while (0)

template <int CH>
hipError_t launch_static(const float* raw, const float* z, const float* noise, float noise_std, size_t n_rays, int N, int flags,
                         float* rgb, float* disp, float* acc, float* weights, float* depth, hipStream_t stream) {
#define DFN_R2O_FWD(S)                                                                                                           \
  hipLaunchKernelGGL((raw2outputs_static_kernel<S, CH>), ray_grid(n_rays), dim3(256), 0, stream, raw, z, noise, noise_std, n_rays, \
                     N, flags, rgb, disp, acc, weights, depth)
  DFN_R2O_SPL(DFN_R2O_FWD);
#undef DFN_R2O_FWD
  return hipGetLastError();
}

template <int CH>
hipError_t launch_backward(const float* raw, const float* z, const float* noise, float noise_std, const R2OGrads& g, size_t n_rays, int N,
                           int flags, float* graw, float* gz, hipStream_t stream) {
  // nine channels: stage the rows through LDS when they are whole 16-byte pieces at 16-byte addresses and four of them fit 64 KB
  size_t lds = size_t(4) * N * CH * sizeof(float);
  flags &= ~kStagedFlag;
  if (CH == 9 && (N & 3) == 0 && ((reinterpret_cast<uintptr_t>(raw) | reinterpret_cast<uintptr_t>(graw)) & 15) == 0 && lds <= 64 * 1024)
    flags |= kStagedFlag;
  else
    lds = 0;
#define DFN_R2O_BWD(S)                                                                                                                \
  hipLaunchKernelGGL((raw2outputs_backward_kernel<S, CH>), ray_grid(n_rays), dim3(256), lds, stream, raw, z, noise, noise_std, g, n_rays, \
                     N, flags, graw, gz)
  DFN_R2O_SPL(DFN_R2O_BWD);
#undef DFN_R2O_BWD
  return hipGetLastError();
}
#undef DFN_R2O_SPL

// The checks the two entries share; 0 or the error already recorded.
int check_mode(const char* who, const void* raw, const void* z, const void* noise, int ch, int N, int flags) {
  if (!raw || !z) return set_error(DFN_ERR_ARG, "%s: bad argument (raw or z_vals NULL)", who);
  if (N < 1 || N > 512) return set_error(DFN_ERR_ARG, "%s: bad argument (1 <= N <= 512, got %d)", who, N);
  if (ch != 1 && ch != 4 && ch != 9)
    return set_error(DFN_ERR_ARG, "%s: bad argument (ch = %d: 1 = sigma of the coarse test-time mode, 4 = (rgb, sigma), 9 = static + transient)",
                     who, ch);
  const bool coarse_test = (flags & DFN_COMP_COARSE) && (flags & DFN_COMP_TEST_TIME);
  if ((ch == 1) != coarse_test)
    return set_error(DFN_ERR_ARG, "%s: bad argument (ch = 1 goes with DFN_COMP_COARSE | DFN_COMP_TEST_TIME and only with them: that mode "
                                  "reads the sigma channel alone)", who);
  if (ch == 9 && noise) return set_error(DFN_ERR_ARG, "%s: bad argument (noise with ch = 9: the transient mode draws none)", who);
  return DFN_OK;
}

}  // namespace
}  // namespace dfn

using namespace dfn;

#define HS(s) reinterpret_cast<hipStream_t>(s)
#define CHECK_HIP(expr, what)                                                                   \
  do {                                                                                          \
    hipError_t e_ = (expr);                                                                     \
    if (e_ != hipSuccess) return set_error(DFN_ERR_HIP, "%s: %s", what, hipGetErrorString(e_)); \
  } while (0)

extern "C" int dfn_raw2outputs(const float* raw, int ch, const float* z_vals, const float* noise, float noise_std, size_t n_rays, int N,
                               float beta_min, int flags, float* rgb, float* disp, float* acc, float* weights, float* depth, float* beta,
                               void* stream) {
  if (int rc = check_mode("dfn_raw2outputs", raw, z_vals, noise, ch, N, flags)) return rc;
  if (ch == 9 && (!rgb || !disp || !acc))
    return set_error(DFN_ERR_ARG, "dfn_raw2outputs: bad argument (ch = 9 writes rgb, disp and acc: none of them may be NULL)");
  if (!n_rays) return DFN_OK;
  if (ch == 9)
    CHECK_HIP(launch_composite_fine(raw, z_vals, n_rays, N, beta_min,
                                    flags & (DFN_COMP_TEST_TIME | DFN_COMP_STATIC_ONLY | DFN_COMP_WHITE_BKGD), rgb, disp, acc, depth, weights,
                                    beta, HS(stream)), "dfn_raw2outputs");
  else if (ch == 4)
    CHECK_HIP(launch_static<4>(raw, z_vals, noise, noise_std, n_rays, N, flags, rgb, disp, acc, weights, depth, HS(stream)),
              "dfn_raw2outputs");
  else
    CHECK_HIP(launch_static<1>(raw, z_vals, noise, noise_std, n_rays, N, flags, nullptr, nullptr, acc, weights, nullptr, HS(stream)),
              "dfn_raw2outputs");
  return DFN_OK;
}

extern "C" int dfn_raw2outputs_backward(const float* raw, int ch, const float* z_vals, const float* noise, float noise_std, size_t n_rays,
                                        int N, float beta_min, int flags, const dfn_raw2outputs_grads* grads, float* grad_raw,
                                        float* grad_z, void* stream) {
  (void)beta_min;   // a constant added to beta: it reaches no gradient
  if (int rc = check_mode("dfn_raw2outputs_backward", raw, z_vals, noise, ch, N, flags)) return rc;
  R2OGrads g{};
  if (grads) {   // the outputs the mode has: M1 acc and weights; M2 no beta (a constant)
    g.acc = grads->acc;
    g.weights = grads->weights;
    if (ch != 1) { g.rgb = grads->rgb; g.disp = grads->disp; g.depth = grads->depth; }
    if (ch == 9) g.beta = grads->beta;
  }
  if (!g.rgb && !g.disp && !g.acc && !g.weights && !g.depth && !g.beta)
    return set_error(DFN_ERR_ARG, "dfn_raw2outputs_backward: bad argument (no upstream gradient on an output of this mode)");
  if (!grad_raw && !grad_z) return set_error(DFN_ERR_ARG, "dfn_raw2outputs_backward: bad argument (grad_raw and grad_z both NULL)");
  if (!n_rays) return DFN_OK;
  if (ch == 9)
    CHECK_HIP(launch_backward<9>(raw, z_vals, nullptr, 0.f, g, n_rays, N, flags, grad_raw, grad_z, HS(stream)), "dfn_raw2outputs_backward");
  else if (ch == 4)
    CHECK_HIP(launch_backward<4>(raw, z_vals, noise, noise_std, g, n_rays, N, flags, grad_raw, grad_z, HS(stream)),
              "dfn_raw2outputs_backward");
  else
    CHECK_HIP(launch_backward<1>(raw, z_vals, noise, noise_std, g, n_rays, N, flags, grad_raw, grad_z, HS(stream)),
              "dfn_raw2outputs_backward");
  return DFN_OK;
}
