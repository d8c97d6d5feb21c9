// nerfh_fused_train.h — the register-resident NeRF-H TRAINING chain (netwidth 128): launch interface and data layout shared by
// nerfh_fused_chain.hip (forward / data-gradient chains), nerfh_fused_wgrad.hip (weight-gradient stream, reductions, per-step
// weight packing) and nerfh_train_api.hip (orchestration).
//
// What one optimisation step of the reference needs (script/run_nerf.py:32-80, loss.backward() over models/nerfw.py:297-354) and
// how it is laid out here:
//   * forward chain  — both networks exactly as the test-time kernels run them (nerfh_mlp_core.h: weights = MFMA A operand,
//     32 points per wavefront carried through every layer in registers, split-f16 products = fp32-grade), additionally storing
//     every layer INPUT X_l as the split-f16 B-operand registers it already is, plus one ReLU sign bit per hidden unit;
//   * backward chain — the transposed chain of nerfh_bwd.hip from the pre-activation gradients of the heads, ReLU gates from the
//     sign bits, storing every layer's pre-activation gradient G_l as the B-operand registers it already is; a wavefront's 32
//     points share ONE power-of-two scale per stored array (recorded per wave-tile), so the halves stay in f16's range whatever
//     the gradient magnitude;
//   * weight gradients — dW_l[n, k] = sum_p G_l[p, n] X_l[p, k] as a pure stream: the stored arrays are DMA-ed into LDS and read
//     back TRANSPOSED (ds_read_b64_tr_b16: [point][feature] image -> [feature][point] MFMA operands), three f16 MFMAs per
//     product, fp32 accumulation per wave-tile folded into a master accumulator at the tile's scale; fixed point chunks ->
//     partial sums -> fixed-order reduction (deterministic) scattered straight into the torch .grad tensors.
// Nothing but X_l / G_l (2 bytes per element for the fine network, 4 for the coarse one; written once, read once) and 84 bytes
// of sign bits per point touches HBM.
//
// Stored array layout ("wave-tile" wt = 32 consecutive points = one wavefront of a chain tile):
//   array[wt][chunk c][plane 0 = hi | 1 = lo][point p (32)][half h (2)][slot j (8)]   f16, 1024 bytes per plane and chunk
// (fine network: ONE plane = f16(hi + lo) unless DFN_TRAIN_FUSED_SPLIT; coarse network: both — planes_of() below)
// chunk c, half h, slot j = contraction slot s = 8 c + j of half h of the B operand (nerfh_layout.h: hidden_feature /
// pe_xyz_feature give the feature index).  A plane is 1 KiB = one wave-wide 16-byte store / LDS-DMA.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

struct dfn_nerfh_s;

namespace dfn {
namespace train {
struct CompGrads;   // nerfh_train.h
}
}

namespace dfn {
namespace fused {

constexpr int kTilePoints = 256;   // points per workgroup tile of the chain kernels (8 waves x 32)
constexpr int kWaveTile = 32;
constexpr int kMaskWords = 21;     // as nerfh_kernels.h: 8 x 128 + 64 + 4 x 64 sign bits per point
// Planes stored per chunk: 2 = hi | lo (the chains' split-f16 operand registers as they are, 4 bytes per element); 1 = ONE f16
// plane, round-to-nearest of hi + lo (2 bytes per element).  The weight gradient is a sum over ~10^5 points of products whose f16
// rounding errors are unbiased and independent.  Measured against the exact-fp32 step (tools/gpu_n1_planes.sh, LABBOOK R5.6):
//   * FINE network (295 k points per 1 536-ray step, gradients from every loss term): random-init weights — every gradient tensor
//     stays where two planes had it (worst 2.6e-5 against 2.4e-5); trained-like weights (gradients cancel to a small residual) —
//     hidden-layer tensors move from 3e-5 to 3e-4 of their norm, under the tensors both forms already have at 2e-3 (gate flips)
//     and under the 5e-4 the tests hold the random-weight step to -> ONE plane by default (DFN_TRAIN_FUSED), both on request
//     (DFN_TRAIN_FUSED_SPLIT);
//   * COARSE network (its gradient arrives only through the rgb0 term and cancels to ~1e-3 of its terms even at random init): one
//     plane moved the worst tensor from 1.5e-4 to 3.0e-4 (7e-4 at perturb 0, over the tests' 5e-4) -> always BOTH planes.
constexpr int kPlanesCoarse = 2;
inline int planes_of(bool fine, bool split_fine) { return fine ? (split_fine ? 2 : 1) : kPlanesCoarse; }

// ---- stored arrays
// X arrays (forward-layer inputs).  Coarse net: XA_PE .. XA_DE.
enum XArr { XA_PE = 0, XA_H1, XA_H2, XA_H3, XA_H4, XA_H5, XA_H6, XA_H7, XA_H8, XA_FIN, XA_DE, XA_T0, XA_T1, XA_T2, XA_T3, XA_COUNT };
constexpr int kXChunks[XA_COUNT] = {4, 8, 8, 8, 8, 8, 8, 8, 8, 8, 4, 4, 4, 4, 4};
constexpr int kXCountCoarse = XA_DE + 1;
// G arrays (pre-activation gradients = inputs of the backward layers).  GA_L1..GA_L8: d h_l (pre-activation); GA_CAT2:
// [d final (8 chunks); slot 64 of half 0 = d sigma_s]; GA_CAT: fine [d t0 (4); d dir_h (4)], coarse [d dir_h (4)];
// GA_DRGB: d rgb_s; GA_T1..GA_T3: d t1..t3; GA_DTH: [d rgb_t(3), d sigma_t, -, -, -, -, d beta].
enum GArr { GA_L1 = 0, GA_L2, GA_L3, GA_L4, GA_L5, GA_L6, GA_L7, GA_L8, GA_CAT2, GA_CAT, GA_DRGB, GA_T1, GA_T2, GA_T3, GA_DTH, GA_COUNT };
constexpr int kGChunksFine[GA_COUNT] = {8, 8, 8, 8, 8, 8, 8, 8, 10, 8, 2, 4, 4, 4, 2};
constexpr int kGChunksCoarse[GA_COUNT] = {8, 8, 8, 8, 8, 8, 8, 8, 10, 4, 2, 0, 0, 0, 0};
constexpr int kGCountCoarse = GA_DRGB + 1;

struct ChainArgs {
  const char* blob;        // packed units of this pass (forward or backward) in execution order
  const uint32_t* tab;     // [n_units][2] = (byte offset, bytes)
  int n_units;
  const float* rays_o;     // [n_rays,3]
  const float* rays_d;     // [n_rays,3]
  const float* z;          // [n_rays, n_samples]
  const float* ray_bias;   // [n_rays, kRayBiasFloats] C-fragment order (coarse: table 0 only)
  float* raw_out;          // forward: [P, 9] (fine) / [P, 4] (coarse: rgb, sigma)
  const float* gpre;       // backward: [P, 9] / [P, 4] d L / d PRE-activation head outputs
  uint32_t* masks;         // [n_wt][kMaskWords][64]
  char* arrays;            // base of the stored arrays (forward: X, backward: G)
  size_t arr_off[16];      // byte offset of each array (forward: XArr, backward: GArr)
  float* gscale;           // backward: [GA_COUNT][n_wt] scale carried by each stored wave-tile (stored = true x scale)
  long long n_rays;
  int n_samples;
  float in_scale;          // split-f16: weight scale x activation scale carried by the accumulators
  int* status;             // range guard (as MlpArgs::status)
};
hipError_t launch_train_forward_chain(bool fine, int planes, const ChainArgs& a, int n_cu, hipStream_t s);
hipError_t launch_train_backward_chain(bool fine, int planes, const ChainArgs& a, int n_cu, hipStream_t s);
// both networks' data-gradient chains as the two halves of one grid (nerfh_fused_chain.hip: train_bwd_chain_pair_kernel)
hipError_t launch_train_backward_chain_pair(int planes_fine, const ChainArgs& fine, const ChainArgs& coarse, int n_cu, hipStream_t s);
size_t chain_wave_tiles(long long n_points);   // wave-tiles the chain kernels write (whole tiles)
// The chains on GIVEN points, one network at a time (nerfh_fused_chain_pts.hip; dfn_nerfh_points_train_*).  Same ChainArgs, read
// differently: rays_o = pts [P, 3] (rays_d, z unused); n_rays = rows, n_samples = points per row; backward: gpre = d L / d raw
// (POST-activation, [P, 9] / [P, 4]) and raw_out = the forward's raw, read only — the chain forms the pre-activation seed itself.
hipError_t launch_points_forward_chain(bool fine, int planes, const ChainArgs& a, int n_cu, hipStream_t s);
hipError_t launch_points_backward_chain(bool fine, int planes, const ChainArgs& a, int n_cu, hipStream_t s);
// ... and the two per-row kernels in front of them (nerfh_fused_points.hip).  Row inputs of ONE network from view directions as given
// (not normalised: nerfw.py:47-95 embeds input_dirs as they come): dir_in[r] = [pe_dir(v) | embedding_a[hist] (emb_a != nullptr)],
// t_in[r] = embedding_t[hist] (t_in != nullptr), padding zeroed; *range_word = 0.
struct PointsRowPrepArgs {
  const float* viewdirs; size_t R;
  const float* hist; size_t hist_rows; const float* emb_a; const float* emb_t; int hist_bin, dim_a, dim_t, n_vocab;
  float* dir_in; int ld_dir; float* t_in; int ld_t;
  int* range_word;
};
hipError_t launch_points_row_prep(const PointsRowPrepArgs& a, hipStream_t s);
// one network's bias table, as launch_ray_bias_train_pair below forms two (w_te == nullptr: table 0 only)
struct PointsRowBiasArgs {
  const float* w_dir; const float* b_dir; int ldw_dir; int kd; const float* dir_in; int ld_dir;
  const float* w_te; const float* b_te; int ldw_te; int nt; const float* t_in; int ld_t;
  float* table;
};
hipError_t launch_points_row_bias(const PointsRowBiasArgs& a, size_t R, hipStream_t s);

// ---- weight-gradient stream
struct WJob {
  const char* g;           // G array: [n_wt][kcg][chunk bytes]
  const char* x0;          // X array(s): [n_wt][kcx0][chunk bytes] (, [n_wt][kcx1][chunk bytes])
  const char* x1;
  const float* gscale;     // [n_wt]
  float* partial;          // [n_chunks][n_blocks][1024]
  int kcg, kcx0, kcx1;
  int g_stride;            // chunks per wave-tile of the G array (the job reads chunks [g_chunk0, g_chunk0 + kcg) of them)
  int g_chunk0;
  int nb_g, nb_x;          // 32-feature blocks on either side; blocks = nb_g x (nb_x + has_bias): the extra column block = bias sums
  int has_bias;
  int wt_per_chunk, n_chunks;
  int first_wg;            // first workgroup of this job in the launch
  int map_off;             // offset (ints) of this job's destination map inside the map table
};
constexpr int kMaxJobs = 20;
struct WgradArgs {
  WJob job[kMaxJobs];
  int n_jobs;
  int n_wt;
};
// (the reduction reads a few fields of a job only: a compact record, so that BOTH networks' jobs — 17 + 13 — fit one launch's arguments)
struct RJob { const float* partial; int nb_g, nb_x, has_bias, n_chunks, map_off; };
constexpr int kMaxReduceJobs = 2 * kMaxJobs;
struct ReduceArgs {
  RJob job[kMaxReduceJobs];
  int n_jobs;
  const int* map;          // per job: [n_blocks][1024] destination (param << 20 | offset) or -1, index r * 64 + lane
  float* grads[64];        // the step's gradient tensors in canonical order (dfn_nerfh_train_param_name)
};
hipError_t launch_wgrad_stream(const WgradArgs& a, int total_wgs, int planes, hipStream_t s);
hipError_t launch_wgrad_reduce(const ReduceArgs& a, hipStream_t s);
constexpr uint32_t kWgradLdsBytes = 81920;    // staging ring of one stream workgroup (two per CU)

// ---- per-step packing of the master weights into the chain kernels' staging units
struct PackElem { uint32_t off; int32_t src; };    // f16 element: hi at blob + off, lo at + 1024; src = param << 20 | index, < 0: zero
// the four unit blobs of a step (coarse / fine x forward / backward) in ONE launch: blockIdx.y = blob
struct PackBlob { const PackElem* welem; int n_welem; const PackElem* belem; int n_belem; char* blob; float wscale, bscale; };
struct PackArgs4 { PackBlob b[4]; const float* params[64]; int* status; };
hipError_t launch_pack4(const PackArgs4& a, hipStream_t s);

// The step's range word (dfn_nerfh_s::range_flag + 2: raised by this step's pack / chain kernels only) decides what the step leaves in
// the gradient tensors: non-zero -> every gradient is ZEROED (a skipped step, as a loss scaler skips a step whose gradients
// overflowed: the optimizer sees zeros, never clamped or NaN gradients) and the bits are ORed into the handle's range flag, where
// dfn_nerfh_range_status(_async) finds them.  Last launch of the backward pass.
struct GuardArgs {
  float* grads[64];
  uint32_t numel[64];
  int n;
  int* step_flag;
  int* range_flag;
};
hipError_t launch_grads_guard(const GuardArgs& a, hipStream_t s);

// table[ray][tbl][mb][h][r] (C-fragment order, nerfh_layout.h) = b[f] + sum_j W[f, 128 + j] in[ray, j]; tbl 0 = dir_encoding.0
// on dir_in [R, ld_dir] (kd columns), tbl 1 = transient_encoding.0 on t_in (nt columns; w_te == nullptr: table 0 only).
hipError_t launch_ray_bias_train_pair(const float* w_dir_c, const float* b_dir_c, int ldw_dir_c, int kd_c, const float* dir_in_c, int ld_dir_c,
                                      float* table_c, const float* w_dir, const float* b_dir, int ldw_dir, int kd, const float* dir_in,
                                      int ld_dir, const float* w_te, const float* b_te, int ldw_te, int nt, const float* t_in, int ld_t,
                                      float* table_f, size_t R, hipStream_t s);
// out[r][feat] (feat < 16 kc) = sum over the ray's samples of the stored gradient array (true scale), feature order = slot order
// mapped through hidden_feature() per 32-slot group: out[r][64 (s >> 5) + hidden_feature(h, s & 31)].
hipError_t launch_frag_ray_sum(const char* arr, int kc, int planes, const float* gscale, size_t R, int Ns, float* out, int ldo, hipStream_t s);
hipError_t launch_frag_ray_sum_pair(const char* arr_f, int kc_f, int planes_f, const float* gscale_f, int Ns_f, float* out_f, int ldo_f,
                                    const char* arr_c, int kc_c, const float* gscale_c, int Ns_c, float* out_c, int ldo_c, size_t R,
                                    hipStream_t s);


// ---- host side (nerfh_fused_api.hip), called by dfn_nerfh_train_* when the handle runs the register-resident kernels
struct State;
bool available(const dfn_nerfh_s* h);
size_t workspace_bytes(const dfn_nerfh_s* h, size_t n_rays, int Nc, int Ni);
// fn: the calling entry's name (messages); viewdirs [n_rays,3]: view directions used as given, nullptr = rays_d normalised
int train_forward(const char* fn, dfn_nerfh_s* h, const float* const* params, const float* rays_o, const float* rays_d,
                  const float* viewdirs, const float* hist, size_t hist_rows, size_t n_rays, int Nc, int Ni, float near, float far, const float* t_rand, const float* noise, float raw_noise_std,
                  const float* u, float* rgb, float* disp, float* acc, float* raw, float* rgb0, float* disp0, float* acc0, float* z_std,
                  float* beta, void* workspace, size_t workspace_bytes, hipStream_t s);
// fn: the calling entry's name (messages); cg: what the compositing-backward stage starts from (train::composite_backward) — everything
// after that stage is the same for dfn_nerfh_train_backward and dfn_nerfh_train_backward_maps.
int train_backward(const char* fn, dfn_nerfh_s* h, const float* const* params, const float* hist, size_t hist_rows, size_t n_rays, int Nc,
                   int Ni, const float* noise, float raw_noise_std, const float* raw, const train::CompGrads& cg, float* const* grads,
                   void* workspace, size_t workspace_bytes, hipStream_t s);
// Where the forward left the fine depths and the coarse depth sum w z in its workspace (dfn_nerfh_train_depths).
int train_depth_state(dfn_nerfh_s* h, size_t n_rays, int Nc, int Ni, void* workspace, size_t workspace_bytes, const float** z_fine,
                      const float** depth0);
void destroy_state(dfn_nerfh_s* h);

}  // namespace fused
}  // namespace dfn
