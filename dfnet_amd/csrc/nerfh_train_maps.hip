// nerfh_train_maps.hip — compositing backward of the TRAINING render for EVERY output of its two compositors (gfx950): rgb0, acc0, depth0,
// disp0 of the coarse pass and rgb, beta, acc, depth, disp of the fine one (models/rendering.py:161-243 with test_time=False, both typ;
// under autograd in the reference all of them are torch expressions of the networks' outputs).  What dfn_nerfh_train_backward_maps /
// _backward_rays_maps run where composite_coarse_backward / composite_fine_backward_train (nerfh_train.hip, untouched: rgb0 / rgb, beta
// and transient_sigma, what NerfWLoss uses) run in the default step (the coarse stage keeps composite_coarse_backward for its rgb0 term).  Same shape as those two: one wave per ray, four rays per block,
// samples in 64-wide blocks with a carried transmittance, suffix sums from the far end in fixed order, no atomics, pre-activation
// gradients out.  The test-time counterpart (static-only depth under disp, the render maps) is nerfh_maps_bwd.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nerfh_device.h"
#include "nerfh_train.h"

namespace dfn {
namespace train {

static inline int ray_grid(size_t R) {
  const size_t g = (R + 3) / 4;
  return int(g < size_t(256 * 16) ? (g ? g : 1) : size_t(256 * 16));
}

// disp = 1 / max(1e-10, depth / acc) is a function of two other outputs of the same ray: where the clamp is inactive disp = acc / depth,
// d disp / d depth = -acc / depth^2 (= -disp^2 / acc), d disp / d acc = 1 / depth (= disp / acc); elsewhere (and for a ray without any
// weight, 0 / 0) nothing.  A zero g_disp leaves the other two untouched, bit for bit.
DFN_DEV void fold_disp(float g_disp, float acc, float depth, float& g_acc, float& g_depth) {
  if (g_disp != 0.f && depth / acc > 1e-10f) {
    const float inv = 1.f / depth;
    g_acc += g_disp * inv;
    g_depth -= g_disp * acc * inv * inv;
  }
}

// ------------------------------------------------------------------------------------------ coarse pass, all outputs
// rendering.py:161-193,231-243 (typ="coarse", test_time=False): s_i = sigma_i + noise_i std, alpha_i = 1 - exp(-delta_i relu(s_i)),
// T_i = prod_{j<i} (1 - alpha_j), w_i = alpha_i T_i; rgb0 = sum w c, acc0 = sum w, depth0 = sum w z, disp0 = 1 / max(1e-10, depth0 / acc0).
// The gradient is linear in the upstream gradients, and the stage (composite_coarse_backward_maps below) is two launches:
//   * the rgb0 term by composite_coarse_backward_kernel itself, the kernel of the default step.  The coarse network's gradients are sums
//     that cancel to ~1e-3 of their terms (the sigma head's to |g| = 3e-7 at random-init weights), so one ulp per sample of gpre moves them
//     by ~1e-4 — measured: a second kernel with the same source expressions for the rgb0 term, which the compiler contracts differently,
//     sat 7e-5 (exact step) / 1e-4 (fused) from the default step on static_sigma.  This way a map term added to NerfWLoss changes the coarse
//     gradients by the map term alone, and where the new entries are given the NerfWLoss operands they return the default step's coarse
//     gradients bit for bit;
//   * the three map outputs by the kernel below, which writes gpre or adds onto what the first launch wrote.  With v_i = g_depth0 z_i
//     (g_disp0 folded into g_depth0 and g_acc0 first):
//       d s_i = [s_i > 0] delta_i ((1 - alpha_i) T_i v_i - S_i + g_acc0 T_end),   S_i = sum_{k>i} w_k v_k;   d c_i = 0.
// acc0 = 1 - T_end (T_end: the transmittance behind the last sample), so d acc0 / d s_i = [s_i > 0] delta_i T_end in closed form; carried
// through v_i it would be T_{i+1} - sum_{k>i} w_k, two numbers near T_{i+1} whose round-off dwarfs T_end.  T_end is the product of the
// exponentials themselves, not of the forward's 1 - alpha, which is 0 below 6e-8 — at the far end of a ray (interval 1e2) that is the
// common case, and torch's exp backward multiplies by the exponential too.  1 - alpha is never divided by: an opaque sample gives finite
// gradients.  z carries no gradient.  A null upstream pointer is read as zeros by the same instructions.  Out: gpre [R,Nc,4],
// pre-activation (x (1 - exp(-sigma))).  LDS: 2 Nc floats per wave.
__global__ __launch_bounds__(256) void composite_coarse_backward_maps_kernel(const float* __restrict__ raw_c, const float* __restrict__ z_c,
                                                                             const float* __restrict__ noise, float noise_std,
                                                                             const TrainMapGrads g, size_t R, int Nc, int accumulate,
                                                                             float* __restrict__ gpre) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* s_T = sm + size_t(wave) * 2 * Nc;
  float* s_al = s_T + Nc;
  for (size_t ray = size_t(blockIdx.x) * 4 + wave; ray < R; ray += size_t(gridDim.x) * 4) {
    float g_acc = g.acc0 ? g.acc0[ray] : 0.f, g_depth = g.depth0 ? g.depth0[ray] : 0.f;
    const float* rr = raw_c + ray * size_t(Nc) * 4;
    const float* zr = z_c + ray * size_t(Nc);
    const float* nr = noise ? noise + ray * size_t(Nc) : nullptr;
    float carry = 1.f, T_end = 1.f, sa = 0.f, sd = 0.f;
    for (int c0 = 0; c0 < Nc; c0 += 64) {
      const int i = c0 + lane;
      float alpha = 0.f, om = 1.f, zi = 0.f;
      if (i < Nc) {
        const float sg = rr[size_t(i) * 4 + 3];
        const float se = nr ? add_rn(sg, mul_rn(nr[i], noise_std)) : sg;
        zi = zr[i];
        const float delta = i + 1 < Nc ? sub_rn(zr[i + 1], zi) : 1e2f;
        om = expf(-mul_rn(delta, fmaxf(se, 0.f)));
        alpha = sub_rn(1.f, om);
      }
      T_end *= __shfl(wave_incl_prod(om, lane), 63, 64);
      const float incl = wave_incl_prod(sub_rn(1.f, alpha), lane);
      float excl = __shfl_up(incl, 1, 64);
      if (lane == 0) excl = 1.f;
      if (i < Nc) {
        const float T = mul_rn(carry, excl);
        s_T[i] = T;
        s_al[i] = alpha;
        const float w = mul_rn(alpha, T);
        sa += w;
        sd += mul_rn(w, zi);
      }
      carry = mul_rn(carry, __shfl(incl, 63, 64));
    }
    if (g.disp0) fold_disp(g.disp0[ray], wave_sum(sa), wave_sum(sd), g_acc, g_depth);   // (uniform branch)
    const float tail_acc = g_acc * T_end;
    wave_sync();
    float tail = 0.f;
    for (int c0 = ((Nc - 1) / 64) * 64; c0 >= 0; c0 -= 64) {
      const int i = c0 + lane;
      float T = 0.f, al = 0.f, v = 0.f, zi = 0.f;
      if (i < Nc) {
        T = s_T[i];
        al = s_al[i];
        zi = zr[i];
        v = g_depth * zi;
      }
      const float suf = wave_incl_suffix_sum(al * T * v, lane);   // from the far end: eps x |S_i|, not eps x the block total (0 beyond the ray)
      const float blk = __shfl(suf, 0, 64);
      float later = __shfl_down(suf, 1, 64);
      if (lane == 63) later = 0.f;
      const float S = tail + later;          // strictly after i
      if (i < Nc) {
        const float sg = rr[size_t(i) * 4 + 3];
        const float se = nr ? add_rn(sg, mul_rn(nr[i], noise_std)) : sg;
        const float delta = i + 1 < Nc ? sub_rn(zr[i + 1], zi) : 1e2f;
        const float ds = se > 0.f ? delta * ((1.f - al) * T * v - S + tail_acc) : 0.f;
        float* o = gpre + (ray * size_t(Nc) + i) * 4;
        if (accumulate) {
          o[3] = add_rn(o[3], ds * -expm1f(-sg));
        } else {
          o[0] = o[1] = o[2] = 0.f;
          o[3] = ds * -expm1f(-sg);
        }
      }
      tail += blk;
    }
    wave_sync();
  }
}

// rgb0 through the default step's kernel, the map outputs written or added by the kernel above (see there).
hipError_t composite_coarse_backward_maps(const float* raw_c, const float* z_c, const float* noise, float noise_std,
                                          const TrainMapGrads& g, size_t R, int Nc, float* gpre, hipStream_t s) {
  if (!R) return hipSuccess;
  const bool maps = g.acc0 || g.depth0 || g.disp0;
  if (g.rgb0) {
    const hipError_t e = composite_coarse_backward(raw_c, z_c, noise, noise_std, g.rgb0, R, Nc, gpre, s);
    if (e != hipSuccess || !maps) return e;
  }
  hipLaunchKernelGGL(composite_coarse_backward_maps_kernel, dim3(ray_grid(R)), dim3(256), size_t(4) * 2 * Nc * sizeof(float), s, raw_c, z_c,
                     noise, noise_std, g, R, Nc, g.rgb0 ? 1 : 0, gpre);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------ fine pass (training compositor), all outputs
// rendering.py:168-209,241-242 with test_time=False: a_s = 1 - exp(-delta sigma_s), a_t = 1 - exp(-delta sigma_t), om = exp(-delta (sigma_s
// + sigma_t)) = 1 - a, T_i = prod_{j<i} om_j (joint);  rgb = sum T (a_s c_s + a_t c_t), beta = sum T a_t b + beta_min,
// acc = sum a T, depth = sum a T z, disp = 1 / max(1e-10, depth / acc).  With js = g_rgb.c_s, jt = g_rgb.c_t + g_beta b, ja = g_depth z
// (g_disp folded into g_depth and g_acc first) and e_i = T_i (a_s js + a_t jt + a ja), S_i = sum_{k>i} e_k:
//   d c_s = g_rgb T a_s,  d c_t = g_rgb T a_t,  d b = g_beta T a_t,
//   d sigma_s = delta ((1 - a_s) T js - S + om T ja + g_acc T_end),   d sigma_t = delta ((1 - a_t) T jt - S + om T ja + g_acc T_end) + g_tsigma
// (acc = 1 - T_end in closed form, as in the coarse kernel; the rgb / beta terms are formed as composite_fine_backward_train_kernel forms
// them — a_s, a_t from the forward's 1 - exp, 1 - a_s and 1 - a_t from those — so that the two kernels differ by the new terms alone).
// gext [R,Nf,9] (nullable) is added to d L / d raw before the activation derivatives: it generalises the dense channel-7 operand of
// composite_fine_backward_train.  Out: gpre [R,Nf,9].  LDS: Nf floats per wave.
__global__ __launch_bounds__(256) void composite_fine_backward_train_maps_kernel(const float* __restrict__ raw, const float* __restrict__ z,
                                                                                 const TrainMapGrads g, float g_tsigma,
                                                                                 const float* __restrict__ gext, size_t R, int Nf,
                                                                                 float* __restrict__ gpre) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* s_T = sm + size_t(wave) * Nf;
  for (size_t ray = size_t(blockIdx.x) * 4 + wave; ray < R; ray += size_t(gridDim.x) * 4) {
    const float g0 = g.rgb ? g.rgb[ray * 3] : 0.f, g1 = g.rgb ? g.rgb[ray * 3 + 1] : 0.f, g2 = g.rgb ? g.rgb[ray * 3 + 2] : 0.f;
    const float gb = g.beta ? g.beta[ray] : 0.f;
    float g_acc = g.acc ? g.acc[ray] : 0.f, g_depth = g.depth ? g.depth[ray] : 0.f;
    const float* rr = raw + ray * size_t(Nf) * 9;
    const float* zr = z + ray * size_t(Nf);
    const float* xr = gext ? gext + ray * size_t(Nf) * 9 : nullptr;
    float carry = 1.f, sa = 0.f, sd = 0.f;
    for (int c0 = 0; c0 < Nf; c0 += 64) {
      const int i = c0 + lane;
      float om = 1.f, zi = 0.f;
      if (i < Nf) {
        const float* v = rr + size_t(i) * 9;
        zi = zr[i];
        const float delta = i + 1 < Nf ? sub_rn(zr[i + 1], zi) : 1e2f;
        om = expf(-mul_rn(delta, add_rn(v[3], v[7])));
      }
      const float incl = wave_incl_prod(om, lane);
      float excl = __shfl_up(incl, 1, 64);
      if (lane == 0) excl = 1.f;
      if (i < Nf) {
        const float T = carry * excl;
        s_T[i] = T;
        const float w = sub_rn(1.f, om) * T;
        sa += w;
        sd += w * zi;
      }
      carry *= __shfl(incl, 63, 64);
    }
    if (g.disp) fold_disp(g.disp[ray], wave_sum(sa), wave_sum(sd), g_acc, g_depth);   // (uniform branch)
    const float tail_acc = g_acc * carry;   // carry = T_end
    wave_sync();
    float tail = 0.f;
    for (int c0 = ((Nf - 1) / 64) * 64; c0 >= 0; c0 -= 64) {
      const int i = c0 + lane;
      float T = 0.f, delta = 0.f, a_s = 0.f, a_t = 0.f, om = 1.f, js = 0.f, jt = 0.f, ja = 0.f;
      if (i < Nf) {
        const float* v = rr + size_t(i) * 9;
        const float zi = zr[i];
        delta = i + 1 < Nf ? sub_rn(zr[i + 1], zi) : 1e2f;
        a_s = sub_rn(1.f, expf(-mul_rn(delta, v[3])));
        a_t = sub_rn(1.f, expf(-mul_rn(delta, v[7])));
        om = expf(-mul_rn(delta, add_rn(v[3], v[7])));
        T = s_T[i];
        js = g0 * v[0] + g1 * v[1] + g2 * v[2];
        jt = g0 * v[4] + g1 * v[5] + g2 * v[6] + gb * v[8];
        ja = g_depth * zi;
      }
      const float e = T * (a_s * js + a_t * jt + sub_rn(1.f, om) * ja);   // 0 beyond the ray (T = 0)
      const float suf = wave_incl_suffix_sum(e, lane);
      const float blk = __shfl(suf, 0, 64);
      float later = __shfl_down(suf, 1, 64);
      if (lane == 63) later = 0.f;
      const float S = tail + later;
      if (i < Nf) {
        const float* v = rr + size_t(i) * 9;
        const float ws = T * a_s, wt = T * a_t;
        float r[9];
        r[0] = g0 * ws; r[1] = g1 * ws; r[2] = g2 * ws;
        const float joint = om * T * ja + tail_acc;   // what depth and acc add to both densities
        r[3] = delta * ((1.f - a_s) * T * js - S + joint);
        r[4] = g0 * wt; r[5] = g1 * wt; r[6] = g2 * wt;
        r[7] = delta * ((1.f - a_t) * T * jt - S + joint) + g_tsigma;
        r[8] = gb * wt;
        if (xr) {
          const float* x = xr + size_t(i) * 9;
#pragma unroll
          for (int c = 0; c < 9; ++c) r[c] = add_rn(r[c], x[c]);
        }
        float* o = gpre + (ray * size_t(Nf) + i) * 9;
        o[0] = r[0] * v[0] * (1.f - v[0]);
        o[1] = r[1] * v[1] * (1.f - v[1]);
        o[2] = r[2] * v[2] * (1.f - v[2]);
        o[3] = r[3] * -expm1f(-v[3]);
        o[4] = r[4] * v[4] * (1.f - v[4]);
        o[5] = r[5] * v[5] * (1.f - v[5]);
        o[6] = r[6] * v[6] * (1.f - v[6]);
        o[7] = r[7] * -expm1f(-v[7]);
        o[8] = r[8] * -expm1f(-v[8]);
      }
      tail += blk;
    }
    wave_sync();
  }
}

hipError_t composite_fine_backward_train_maps(const float* raw, const float* z, const TrainMapGrads& g, float g_tsigma, const float* gext,
                                              size_t R, int Nf, float* gpre, hipStream_t s) {
  if (!R) return hipSuccess;
  hipLaunchKernelGGL(composite_fine_backward_train_maps_kernel, dim3(ray_grid(R)), dim3(256), size_t(4) * Nf * sizeof(float), s, raw, z, g,
                     g_tsigma, gext, R, Nf, gpre);
  return hipGetLastError();
}

}  // namespace train
}  // namespace dfn
