// nerfh_fused_points.hip — the two per-row kernels in front of a training query on points (dfn_nerfh_points_train_forward,
// nerfh_fused_api.hip), for ONE network: what train_ray_prep_kernel (nerfh_train.hip) and ray_bias_train_kernel (nerfh_fused_wgrad.hip)
// do for both networks of a step, on view directions that are GIVEN — run_network_NeRFW embeds input_dirs as they come
// (models/nerfw.py:47-95), only render() normalises rays_d — and without stratified depths.  Same expressions in the same order as
// those two, so a row's inputs and its bias table are the step's bit for bit.  A translation unit of its own: the step's objects stay
// as they are.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nerfh_fused_train.h"
#include "nerfh_kernels.h"
#include "nerfh_layout.h"

namespace dfn {
namespace fused {

// dir_in[r] = [pe_dir(viewdirs[r]) (27) | embedding_a[hist] (emb_a != nullptr: the fine network) | 0 padding], t_in[r] =
// [embedding_t[hist] | 0 padding] (t_in != nullptr); one thread clears the query's range word.
__global__ __launch_bounds__(128) void points_row_prep_kernel(PointsRowPrepArgs a) {
  if (blockIdx.x == 0 && threadIdx.x == 0 && a.range_word) *a.range_word = 0;
  const int na = a.emb_a ? a.hist_bin * a.dim_a : 0, nt = a.t_in ? a.hist_bin * a.dim_t : 0;
  for (size_t row = blockIdx.x; row < a.R; row += gridDim.x) {
    const float* hrow = a.hist ? a.hist + (a.hist_rows == 1 ? 0 : row) * a.hist_bin : nullptr;
    for (int c = threadIdx.x; c < a.ld_dir; c += blockDim.x) {
      float v = 0.f;
      if (c < kChDir) {
        const int coord = c < 3 ? c : (c - 3) % 3;
        const float x = a.viewdirs[row * 3 + coord];
        if (c < 3) v = x;
        else {
          const int k = (c - 3) / 6;
          const float arg = x * float(1 << k);
          v = ((c - 3) % 6) >= 3 ? cosf(arg) : sinf(arg);
        }
      } else if (c < kChDir + na) {
        const int j = c - kChDir;
        long long idx = (long long)hrow[j / a.dim_a];   // .long() truncation (nerfw.py:69)
        idx = idx < 0 ? 0 : (idx >= a.n_vocab ? a.n_vocab - 1 : idx);
        v = a.emb_a[idx * a.dim_a + j % a.dim_a];
      }
      a.dir_in[row * a.ld_dir + c] = v;
    }
    if (a.t_in)
      for (int c = threadIdx.x; c < a.ld_t; c += blockDim.x) {
        float v = 0.f;
        if (c < nt) {
          long long idx = (long long)hrow[c / a.dim_t];
          idx = idx < 0 ? 0 : (idx >= a.n_vocab ? a.n_vocab - 1 : idx);
          v = a.emb_t[idx * a.dim_t + c % a.dim_t];
        }
        a.t_in[row * a.ld_t + c] = v;
      }
  }
}
hipError_t launch_points_row_prep(const PointsRowPrepArgs& a, hipStream_t s) {
  if (!a.R) return hipSuccess;
  if (((a.emb_a || a.t_in) && !a.hist) || (a.t_in && !a.emb_t)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(points_row_prep_kernel, dim3(unsigned(a.R < 4096 ? a.R : 4096)), dim3(128), 0, s, a);
  return hipGetLastError();
}

// table[row][tbl][mb][h][r] (C-fragment order) = b[f] + sum_j W[f, 128 + j] in[row, j] for one network: tbl 0 = dir_encoding.0 on dir_in,
// tbl 1 = transient_encoding.0 on t_in (w_te == nullptr, the coarse network: zeros, never read).  ray_bias_train_kernel for one table pair.
__global__ __launch_bounds__(128) void points_row_bias_kernel(PointsRowBiasArgs a, size_t R) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const float* __restrict__ w_dir = a.w_dir; const float* __restrict__ b_dir = a.b_dir; const int ldw_dir = a.ldw_dir, kd = a.kd;
  const float* __restrict__ dir_in = a.dir_in; const int ld_dir = a.ld_dir;
  const float* __restrict__ w_te = a.w_te; const float* __restrict__ b_te = a.b_te; const int ldw_te = a.ldw_te, nt = a.nt;
  const float* __restrict__ t_in = a.t_in; const int ld_t = a.ld_t;
  float* __restrict__ table = a.table;
  float* s_wd = sm;               // [kd][64]
  float* s_wt = sm + kd * 64;     // [nt][64]
  float* s_in = s_wt + (w_te ? nt * 64 : 0);   // [kd + nt] the row's inputs
  auto stage = [&](const float* __restrict__ wsrc, int ldw, int k, float* dst) {   // coalesced reads, transposed in the LDS store
    const int n = k * 64, bd = blockDim.x;
    for (int base = threadIdx.x; base < n; base += bd * 8) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int i = base + u * bd, f = i / k, jj = i - f * k;
        v[u] = i < n ? wsrc[size_t(f) * ldw + kWidth + jj] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int i = base + u * bd, f = i / k, jj = i - f * k;
        if (i < n) dst[jj * 64 + f] = v[u];
      }
    }
  };
  stage(w_dir, ldw_dir, kd, s_wd);
  if (w_te) stage(w_te, ldw_te, nt, s_wt);
  __syncthreads();
  const int tbl = threadIdx.x >> 6, f = threadIdx.x & 63;
  const int mb = f >> 5, row = f & 31, hh = (row >> 2) & 1, r = (row & 3) + 4 * (row >> 3);
  const int slot = ((tbl * 2 + mb) * 2 + hh) * 16 + r;
  const float bias = tbl == 0 ? b_dir[f] : (w_te ? b_te[f] : 0.f);
  for (size_t ray = blockIdx.x; ray < R; ray += gridDim.x) {
    for (int i = threadIdx.x; i < kd + (w_te ? nt : 0); i += blockDim.x) s_in[i] = i < kd ? dir_in[ray * ld_dir + i] : t_in[ray * ld_t + (i - kd)];
    __syncthreads();
    float acc = bias;
    if (tbl == 0) {
      for (int jj = 0; jj < kd; ++jj) acc = fmaf(s_wd[jj * 64 + f], s_in[jj], acc);
    } else if (w_te) {
      for (int jj = 0; jj < nt; ++jj) acc = fmaf(s_wt[jj * 64 + f], s_in[kd + jj], acc);
    }
    table[ray * kRayBiasFloats + slot] = acc;
    __syncthreads();   // (the next row's inputs overwrite s_in)
  }
}
hipError_t launch_points_row_bias(const PointsRowBiasArgs& a, size_t R, hipStream_t s) {
  if (!R) return hipSuccess;
  const size_t k = size_t(a.kd) + (a.w_te ? a.nt : 0);
  const size_t lds = (k * 64 + k) * sizeof(float);
  if (lds > 64 * 1024) return hipErrorInvalidValue;
  hipLaunchKernelGGL(points_row_bias_kernel, dim3(unsigned(R < 256 ? R : 256)), dim3(128), lds, s, a, R);
  return hipGetLastError();
}

}  // namespace fused
}  // namespace dfn
