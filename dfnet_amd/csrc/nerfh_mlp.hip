// nerfh_mlp.hip — the NeRF-H MLP on the CDNA4 matrix cores (gfx950 only).
//
// Persistent workgroups (variant 1: two 4-wave workgroups per CU, running unsynchronised so one's
// epilogue VALU overlaps the other's MFMAs; variant 0: one 8-wave workgroup).  Each wavefront owns NB blocks of 32 sample
// points and carries their activations through the WHOLE network in registers: a Linear layer
// is computed transposed (weights = MFMA A operand, activations = B operand, see
// nerfh_layout.h), so the fp32 C fragments of layer l, after bias/ReLU and conversion, are the
// B operand of layer l+1 — no LDS or HBM round trip for activations.  Positional encoding,
// the point o + d*z, Softplus/Sigmoid heads are fused in.  Only the weights move: every
// layer's pre-permuted MFMA A-fragments stream L2 -> LDS with direct-to-LDS DMA
// (global_load_lds_dwordx4) into a double buffer shared by the workgroup's waves, one barrier per staging unit.
//
// Replaces (reference, /root/reference/script/): models/rendering.py:269-292,305-313 (points),
// models/nerfw.py:15-95 (run_network_NeRFW), :105-133 (Embedder.embed), :297-354 (NeRFW.forward).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "nerfh_device.h"
#include "nerfh_kernels.h"
#include "nerfh_layout.h"
#include "mfma_frag.h"

#include "nerfh_mlp_core.h"
#include "nerfh_mask.h"
#include "nerfh_raydiv.h"

namespace dfn {

// One translation unit (= one code object) per flavour: a wrapper file (nerfh_mlp_{maps,fold,half,res,lean,pts,pts_fold,pts_half}.hip)
// sets DFN_MLP_*_TU flags and includes this file, and gets the kernels and the launcher named below and nothing else, so the code
// objects of the other units do not change by a token when a unit is added.  The flags are cumulative (nerfh_layout.h "Kernel variants"):
//   DFN_MLP_MAPS_TU   launch_mlp_maps: the MAPS instantiations of the plain fine kernels (the render-maps segment record)
//   DFN_MLP_FOLD_TU   variant 5: the fine kernel with the folded tail (kFineFoldSeq)
//   DFN_MLP_HALF_TU   variant 6, on FOLD: half-height head M-blocks (layer<..., HALF>), coarse and fine
//   DFN_MLP_RES_TU    variant 7, on HALF: small layers resident in LDS (layer<..., RES>), MlpResArgs
//   DFN_MLP_LEAN_TU   variant 12, on RES: the lean unit (nerfh_mlp_lean.hip lists its techniques), coarse and fine: tiles claimed from a
//                     device counter (Stager::claim / next), the positional encoding kept for the skip concat (trunk(): kEncodingKept),
//                     the fine kernel's per-ray seeds stored at the accumulators' scale (layer(): RAYBIAS takes them as loaded), uniform
//                     values formed at their use (wave_here / args_here below, stage_issue_at), one select per head value (layer(): the
//                     candidates behind an opaque copy), the packed head activations (kLeanAct4), point -> ray by a magic number
//                     (DFN_RAY_OF) and the range guard by maximum3 (X3Piece::C); MlpLeanArgs = MlpResArgs + the tile counter + the
//                     magic number
//   DFN_MLP_PTS_TU    the points flavour, on none, FOLD or HALF: the inputs are loaded from pts [n_rows, n_samples, 3] (MlpArgs::rays_o)
//                     instead of being formed as o + d z; the raw route only (no depths, so no compositing)
//   DFN_MLP_STATIC_TU the coarse network's training query (nerfw.py:47-60, 326-343), on PTS, plain or FOLD: the fine kernel cut off
//                     behind static_rgb (kCoarseStaticSeq / kCoarseStaticFoldSeq), 4 floats per point; the unit has that kernel alone
// Kernels: nerfh_{fine,coarse}[_fold|_half|_res|_lean][_pts]_kernel; launcher: launch_mlp[_maps][_pts][_fold|_half|_res|_lean];
// DFN_MLP_STATIC_TU: nerfh_coarse_static[_fold]_pts_kernel, launch_mlp_static_pts[_fold].
#if defined(DFN_MLP_STATIC_TU) && (!defined(DFN_MLP_PTS_TU) || defined(DFN_MLP_HALF_TU) || defined(DFN_MLP_MAPS_TU))
#error "the static query exists in the points flavour, plain or folded"
#endif
#if defined(DFN_MLP_RES_TU) && (!defined(DFN_MLP_HALF_TU) || defined(DFN_MLP_PTS_TU))
#error "the resident layers exist in the half-height render kernels"
#endif
#if defined(DFN_MLP_LEAN_TU) && !defined(DFN_MLP_RES_TU)
#error "the lean unit's techniques exist in the kernels with resident layers"
#endif
#if defined(DFN_MLP_LEAN_TU)
#define DFN_TU_TAG _lean
#define DFN_MLP_KARGS MlpLeanArgs
#elif defined(DFN_MLP_RES_TU)
#define DFN_TU_TAG _res
#define DFN_MLP_KARGS MlpResArgs
#elif defined(DFN_MLP_HALF_TU)
#define DFN_TU_TAG _half
#elif defined(DFN_MLP_FOLD_TU)
#define DFN_TU_TAG _fold
#else
#define DFN_TU_TAG
#endif
#ifndef DFN_MLP_KARGS
#define DFN_MLP_KARGS MlpArgs
#endif
#ifdef DFN_MLP_PTS_TU
#define DFN_TU_PTS _pts
#else
#define DFN_TU_PTS
#endif
#ifdef DFN_MLP_MAPS_TU
#define DFN_TU_MAPS _maps
#else
#define DFN_TU_MAPS
#endif
#define DFN_PASTE4_(a, b, c, d) a##b##c##d
#define DFN_PASTE4(a, b, c, d) DFN_PASTE4_(a, b, c, d)
#define DFN_FINE_KERNEL DFN_PASTE4(nerfh_fine, DFN_TU_TAG, DFN_TU_PTS, _kernel)
#if defined(DFN_MLP_FOLD_TU) && !defined(DFN_MLP_HALF_TU) && !defined(DFN_MLP_PTS_TU)
#define DFN_COARSE_KERNEL nerfh_coarse_kernel   // nerfh_mlp_fold.hip has no coarse kernel: the template keeps the plain name
#else
#define DFN_COARSE_KERNEL DFN_PASTE4(nerfh_coarse, DFN_TU_TAG, DFN_TU_PTS, _kernel)
#endif
#define DFN_LAUNCH_MLP DFN_PASTE4(launch_mlp, DFN_TU_MAPS, DFN_TU_PTS, DFN_TU_TAG)
#ifdef DFN_MLP_STATIC_TU   // the truncated fine kernel under a name of its own
#undef DFN_FINE_KERNEL
#undef DFN_LAUNCH_MLP
#define DFN_FINE_KERNEL DFN_PASTE4(nerfh_coarse_static, DFN_TU_TAG, DFN_TU_PTS, _kernel)
#define DFN_LAUNCH_MLP DFN_PASTE4(launch_mlp_static, DFN_TU_MAPS, DFN_TU_PTS, DFN_TU_TAG)
#endif
#ifdef DFN_MLP_MAPS_TU
constexpr bool kMapsTU = true;
#else
constexpr bool kMapsTU = false;
#endif
#ifdef DFN_MLP_HALF_TU
constexpr bool kHalfHeads = true;
#else
constexpr bool kHalfHeads = false;
#endif
#ifdef DFN_MLP_RES_TU
constexpr bool kResident = true;
#else
constexpr bool kResident = false;
#endif
// What the lean unit (DFN_MLP_LEAN_TU) does differently at the tile seam; every other unit takes the #else forms.
//   DFN_NEXT_TILE: the tile a workgroup computes after `tile` (inside the kernels' tile loops): claimed (Stager::next), or dealt.
//   wave_here / args_here: uniform values the tile loop needs once per tile are formed where they are used.  As loop invariants LLVM
//   hoists them to the prologue, where the scalar file cannot hold them all: they are parked in VGPR lanes and every use costs a
//   v_readlane_b32 on the vector pipe (79 parked SGPRs and 231 lane reads per tile in the fine kernel without this).  wave_here: the
//   wave index behind an opaque copy, so that what is derived from it (LDS slot addresses) is scalar arithmetic at the use.  args_here:
//   the kernel arguments read from the kernarg segment at the use (one s_load) instead of held, or parked, for the whole kernel.
//   kLeanAct4: the packed head activations of the fused fine kernel (the transient branch's end).
//   DFN_RAY_OF: the ray of point q (q < 2^31: launch_tiles), by multiply-high and shift with the launch's magic number
//   (nerfh_raydiv.h; MlpLeanArgs::div, two SGPRs) where the other units divide: about 16 vector instructions per lane and point, one
//   of them a quarter-rate reciprocal, at the tile seam.
#ifdef DFN_MLP_LEAN_TU
#define DFN_NEXT_TILE (static_cast<long long>(st.next))
DFN_DEV int wave_here(const Stager& st) {
  int w = st.wave;
  asm volatile("" : "+s"(w));
  return w;
}
typedef const DFN_MLP_KARGS __attribute__((address_space(4))) const_kargs;
DFN_DEV const_kargs* args_here() {
  uint64_t p = reinterpret_cast<uint64_t>(__builtin_amdgcn_kernarg_segment_ptr());   // the argument struct is the kernel's only parameter: offset 0
  asm volatile("" : "+s"(p));
  return reinterpret_cast<const_kargs*>(p);
}
#define DFN_ARGS_HERE(a) (*args_here())
constexpr bool kLeanAct4 = true;
#define DFN_RAY_OF(a, q) ray_div(q, RayDiv{(a).div.magic, (a).div.shift})
#else
#define DFN_NEXT_TILE (tile + gridDim.x)
DFN_DEV int wave_here(const Stager& st) { return st.wave; }
#define DFN_ARGS_HERE(a) (a)
constexpr bool kLeanAct4 = false;
#define DFN_RAY_OF(a, q) ((q) / uint32_t((a).n_samples))
#endif

// Head activations per arithmetic mode: f16 = hardware transcendentals (1e-6), split-f16 = the fp32-grade hardware forms
// (exp_hw / rcp_nr, 1.5e-7: nerfh_device.h), exact fp32 = libm.
template <class P, bool FAST> DFN_DEV float head_softplus(float v) { return FAST ? softplus_fast(v) : (P::kSplit ? softplus_hw(v) : softplus(v)); }
template <class P, bool FAST> DFN_DEV float head_sigmoid(float v) { return FAST ? sigmoid_fast(v) : (P::kSplit ? sigmoid_hw(v) : sigmoid(v)); }
template <class P, bool FAST> DFN_DEV float head_exp(float v) { return FAST ? __expf(v) : (P::kSplit ? exp_hw(v) : expf(v)); }

// three staging buffers in the ring (a ring of four with the DMA issued BEFORE the mid-unit barrier by the early waves fits the
// split-f16 units and was measured: +0.4 %, not kept)
template <class P, int W> constexpr uint32_t ring_slots() { return 3; }
// staging ring + per-wave next-tile input slots (8 dwords x 64 lanes per 64 points: z, o, d, next z)
template <class P, int UMB, int WAVES, int NB, int W = kWidth> constexpr uint32_t lds_bytes() {
  return ring_slots<P, W>() * max_unit_bytes<P>(UMB, W) + WAVES * ((NB * 32 + 63) / 64) * 8 * 256;
}

// Kernel variant 7: the resident region lies behind the input slots.  LDS byte offset of resident layer `id` there; -1 = the layer is
// streamed (every layer, in the units that keep no layers resident).
template <class P, int UMB, int WAVES, int NB, int W, bool FINE> constexpr int res_base(int id) {
  return kResident && layer_resident(FINE, id) ? int(lds_bytes<P, UMB, WAVES, NB, W>() + resident_offset<P>(FINE, id)) : -1;
}
// the layers the kernels below can run out of the resident region (a table entry outside this list would silently be dropped)
constexpr bool resident_set_supported(bool fine) {
  for (int i = 0; i < resident_count(fine); ++i) {
    const int id = resident_at(fine, i);
    const bool ok = id == LY_L1 || id == LY_SIG || (fine && (id == LY_RGB || (id >= LY_TE1 && id <= LY_THEAD)));
    if (!ok) return false;
  }
  return true;
}
static_assert(resident_set_supported(false) && resident_set_supported(true), "a resident layer the kernels stream");
// ring 3 x 33 792 + input slots 8 x 2 048 = 117 760 B; + 33 792 (fine) / 41 984 (coarse) resident = 151 552 / 159 744 of the CU's 163 840
static_assert(lds_bytes<PrecX3M16, unit_mb<PrecX3M16>(0), 8, 1>() + resident_bytes<PrecX3M16>(true) <= kLdsBytes &&
              lds_bytes<PrecX3M16, unit_mb<PrecX3M16>(0), 8, 1>() + resident_bytes<PrecX3M16>(false) <= kLdsBytes,
              "ring + input slots + resident layers must fit the LDS of a CU");
// The lean unit: the word the claimed tile is published through, behind the resident region (16 bytes keep the region's alignment)
constexpr uint32_t kClaimBytes = 16;
static_assert(lds_bytes<PrecX3M16, unit_mb<PrecX3M16>(0), 8, 1>() + resident_bytes<PrecX3M16>(true) + kClaimBytes <= kLdsBytes &&
              lds_bytes<PrecX3M16, unit_mb<PrecX3M16>(0), 8, 1>() + resident_bytes<PrecX3M16>(false) + kClaimBytes <= kLdsBytes,
              "ring + input slots + resident layers + the claimed-tile word must fit the LDS of a CU");

// Workgroups per CU the register allocation is sized for.  netwidth 256 in split-f16 / exact fp32 holds 2 x 128 registers of
// activations per point block: four waves per workgroup, ONE workgroup per CU (512 registers per lane).
template <class P, int WAVES, int NB, int W> constexpr int mlp_min_blocks() {
  if (W > kWidth && (P::kSplit || P::kSlotsPerChunk == 1 || NB >= 2)) return 1;
  return WAVES * NB >= 12 ? (WAVES == 8 ? 2 : 1) : 2;
}

// ------------------------------------------------------------------------------------------
template <class P, bool FAST, int WAVES, int UMB, int NB, bool PIPE, int W = kWidth>
__global__ __launch_bounds__(WAVES * 64, (mlp_min_blocks<P, WAVES, NB, W>())) void DFN_COARSE_KERNEL(DFN_MLP_KARGS a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int PPT = WAVES * NB * 32;
  using F = typename FragOf<P>::type;
  Stager st;
  st.blob = a.blob; st.tab = a.tab; st.n_units = a.n_units; st.u = 0;
  st.waves = WAVES;
  st.dma_waves = a.dma_waves > 0 && a.dma_waves < WAVES ? a.dma_waves : WAVES;
  st.in_scale = a.in_scale;
  st.out_scale = 1.f / a.in_scale;
  st.lane_mul = 1.f;
  st.rmax = 0;
  st.t_sync = st.t_wait = 0;
  st.trace = nullptr;
  st.n_trace = 0;
  st.lane = threadIdx.x & 63;
  st.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#ifdef DFN_TIMING
  const unsigned long long t_begin = __builtin_amdgcn_s_memtime();
  unsigned long long t_pro = 0;
  if (a.timing && blockIdx.x == 7) st.trace = a.timing + 8192 * 4 + st.wave * 192;  // after the per-wave totals
#endif
  const int p = st.lane & 31, h = st.lane >> 5;
  const long long n_pts = (long long)a.n_rays * a.n_samples;
  const long long n_tiles = (n_pts + PPT - 1) / PPT;
  long long tile = blockIdx.x;
  if (tile >= n_tiles) return;
#ifdef DFN_MLP_RES_TU
  stage_resident(st, smem, a.res_blob, resident_bytes<P>(false), lds_bytes<P, UMB, WAVES, NB, W>());
#endif
  stage_prime(st, smem, max_unit_bytes<P>(UMB, W), ring_slots<P, W>());
#ifdef DFN_MLP_LEAN_TU
  // claimed tiles: blockIdx.x first, then gridDim.x + (the counter before this workgroup's add); see Stager.  A workgroup without a
  // first tile has returned above without claiming.
  st.claim = 0; st.grid = gridDim.x; st.next = 0; st.n_tiles = uint32_t(n_tiles); st.more = false;
  st.claim_lds = lds_bytes<P, UMB, WAVES, NB, W>() + resident_bytes<P>(false);
  for (; tile < n_tiles; tile = st.next) {
    if (st.wave == 0 && st.lane == 0) st.claim = claim_tile(a.tile_counter);
    st.claiming = true;
#else
  for (; tile < n_tiles; tile += gridDim.x) {
    st.more = tile + gridDim.x < n_tiles;
#endif
    constexpr int LP = lane_pts<P>(NB);
    float x[LP][3];
    uint32_t pt[NB];   // launch_tiles() bounds a launch to < 2^31 points: 32-bit indices (64-bit ones cost 2 registers each and spilled)
    const uint32_t npts = uint32_t(n_pts);
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) pt[nb] = uint32_t(tile) * uint32_t(PPT) + st.wave * (NB * 32) + nb * 32 + p;   // the lane's output
#pragma unroll
    for (int n = 0; n < LP; ++n) {   // the lane's MLP inputs (PrecX3M16: point 16 n + (lane & 15) of the wave)
      const uint32_t pn = P::kM16 ? uint32_t(tile) * uint32_t(PPT) + st.wave * 32 + 16 * n + (st.lane & 15) : pt[n];
      const uint32_t q = pn < npts ? pn : npts - 1;
#ifdef DFN_MLP_PTS_TU
#pragma unroll
      for (int c = 0; c < 3; ++c) x[n][c] = a.rays_o[size_t(q) * 3 + c];   // pts [n_rows, n_samples, 3]
#else
      const uint32_t ray = DFN_RAY_OF(a, q);
      const int i = int(q - ray * uint32_t(a.n_samples));
      const float z = coarse_z_at(i, a.n_samples, a.near, a.far, a.lindisp != 0);
#pragma unroll
      for (int c = 0; c < 3; ++c)
        x[n][c] = add_rn(a.rays_o[ray * 3 + c], mul_rn(a.rays_d[ray * 3 + c], z));
#endif
    }
    constexpr bool CY = PIPE && P::kSlotsPerChunk == 8, MERGE = UMB >= 8;
    F hid[NB][chunks_of<P>(W / 2)];
    f32x16 carry[NB];
    constexpr int R_L1 = res_base<P, UMB, WAVES, NB, W, false>(LY_L1), R_SIG = res_base<P, UMB, WAVES, NB, W, false>(LY_SIG);
    trunk<P, UMB, PIPE, FAST, NB, W, NoTrunkHook, R_L1>(st, smem, x, hid, carry);
    f32x16 head[NB];
    F dummy[NB][chunks_of<P>(16)];
    const float* const norb[LP] = {};
    layer<P, UMB, PIPE, NB, chunks_of<P>(W / 2), 0, false, true, false, !MERGE && R_SIG < 0, (CY ? 6 : -1), true, false, false, false, true, kHalfHeads, R_SIG>(st, smem, hid, dummy, head, norb, carry);
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
      if (h == 0 && pt[nb] < npts) a.out[pt[nb]] = head_softplus<P, FAST>(head[nb][0]);
  }
  range_report<P>(st.rmax, a.status);
}

// MASKS: the saving forward of the gradient path (dfn_mlp_fine_saving): the same kernel, recording one ReLU sign bit per hidden unit
// for nerfh_fine_backward_kernel's backward-only pass (its own forward-only mode ran without the pipelined conversion: 3.64 ms for the
// DFNet_dm step's 3.7 M points against this kernel's 3.1).
// MAPS: the render-maps flavour of the fused compositing epilogue (dfn_render_*_maps): the segment record grows from 12 to
// kMapsRecFloats floats by the static-only and the transient colour sums.  Its own instantiation: the kernels without it are unchanged.
template <class P, bool FAST, int WAVES, int UMB, int NB, bool PIPE, int W = kWidth, bool MASKS = false, bool MAPS = false>
__global__ __launch_bounds__(WAVES * 64, (mlp_min_blocks<P, WAVES, NB, W>())) void DFN_FINE_KERNEL(DFN_MLP_KARGS a) {
  static_assert(!MASKS || (P::kSplit && !P::kM16 && NB == 1 && WAVES == 8 && W == kWidth), "the sign masks follow the gradient kernel's tile geometry");
  static_assert(!MAPS || (!MASKS && W == kWidth && NB <= 2), "the maps flavour exists where the fused compositing does");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int PPT = WAVES * NB * 32;
  constexpr int HC = chunks_of<P>(W / 2), QC = chunks_of<P>(W / 4);
  constexpr int MBW = W / 32, MBQ = W / 64;       // M-blocks of a W-wide / a W/2-wide layer
  constexpr uint32_t USTRIDE = max_unit_bytes<P>(UMB, W);
  constexpr int PF_ROUNDS = (NB * 32 + 63) / 64;  // 64-point rounds of the next-tile input prefetch
  constexpr int LP = lane_pts<P>(NB);             // points whose inputs a lane carries (PrecX3M16: 16 n + (lane & 15), n = 0, 1)
  // kernel variant 6, compositing fused and no maps: transient_beta (head value 4, on half 1 of the transient head block) reaches no
  // output -- composite_combine_kernel does not read the record's beta slot -- so the block is half-height too and the slot holds 0
  constexpr bool NOBETA = kHalfHeads && !MAPS;
  // kernel variant 7: LDS offsets of the resident layers (-1 = streamed; all of them outside nerfh_mlp_res.hip)
  constexpr int R_L1 = res_base<P, UMB, WAVES, NB, W, true>(LY_L1);
  constexpr int R_SIG = res_base<P, UMB, WAVES, NB, W, true>(LY_SIG), R_RGB = res_base<P, UMB, WAVES, NB, W, true>(LY_RGB),
                R_TE1 = res_base<P, UMB, WAVES, NB, W, true>(LY_TE1), R_TE2 = res_base<P, UMB, WAVES, NB, W, true>(LY_TE2),
                R_TE3 = res_base<P, UMB, WAVES, NB, W, true>(LY_TE3), R_THEAD = res_base<P, UMB, WAVES, NB, W, true>(LY_THEAD);
  using F = typename FragOf<P>::type;
  Stager st;
  st.blob = a.blob; st.tab = a.tab; st.n_units = a.n_units; st.u = 0;
  st.waves = WAVES;
  st.dma_waves = a.dma_waves > 0 && a.dma_waves < WAVES ? a.dma_waves : WAVES;
  st.in_scale = a.in_scale;
  st.out_scale = 1.f / a.in_scale;
  st.lane_mul = 1.f;
  st.rmax = 0;
  st.t_sync = st.t_wait = 0;
  st.trace = nullptr;
  st.n_trace = 0;
  st.lane = threadIdx.x & 63;
  st.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#ifdef DFN_TIMING
  const unsigned long long t_begin = __builtin_amdgcn_s_memtime();
  unsigned long long t_pro = 0;
  if (a.timing && blockIdx.x == 7) st.trace = a.timing + 8192 * 4 + st.wave * 192;  // after the per-wave totals
#endif
  const int p = st.lane & 31, h = st.lane >> 5;
  const long long n_pts = (long long)a.n_rays * a.n_samples;
  const long long n_tiles = (n_pts + PPT - 1) / PPT;
  long long tile = blockIdx.x;
  if (tile >= n_tiles) return;
#ifdef DFN_MLP_RES_TU
  static_assert(!MAPS && !MASKS, "the resident set is the plain fused fine kernel's");
  stage_resident(st, smem, a.res_blob, resident_bytes<P>(true), lds_bytes<P, UMB, WAVES, NB, W>());
#endif
  stage_prime(st, smem, USTRIDE, ring_slots<P, W>());
  // Tile inputs.  The first tile's are loaded normally; every later tile's are PREFETCHED during the
  // previous tile's small layers with direct-to-LDS loads and only
  // waited for at the end of that tile, so the HBM latency of z / o / d is off the critical path.
#ifdef DFN_MLP_PTS_TU
  float xin[LP][3];   // the points themselves: pts [n_rows, n_samples, 3] in a.rays_o
#else
  float zin[LP], znext[LP], oin[LP][3], din[LP][3];
#endif
  // launch_tiles() guarantees n_pts < 2^31: point / ray indices are 32-bit (as 64-bit values and as per-ray table POINTERS held
  // across the trunk they cost 16 registers at NB = 2 and the f16 kernel spilled them: any scratch use costs this kernel clock)
  uint32_t pt[LP], ray_of[LP];
  const uint32_t npts = uint32_t(n_pts);
  auto tile_coords = [&](long long t) {
    uint32_t lp = st.lane;
    asm volatile("" : "+v"(lp));   // the lane's offset inside the tile is formed here (hoisted as a loop invariant, it was spilled)
#pragma unroll
    for (int nb = 0; nb < LP; ++nb) {
      pt[nb] = uint32_t(t) * uint32_t(PPT) + st.wave * (NB * 32) + (P::kM16 ? 16 * nb + (lp & 15) : nb * 32 + (lp & 31));
      const uint32_t q = pt[nb] < npts ? pt[nb] : npts - 1;
      ray_of[nb] = DFN_RAY_OF(a, q);
    }
  };
  tile_coords(tile);
#pragma unroll
  for (int nb = 0; nb < LP; ++nb) {
    const uint32_t q = pt[nb] < npts ? pt[nb] : npts - 1;
#ifdef DFN_MLP_PTS_TU
#pragma unroll
    for (int c = 0; c < 3; ++c) xin[nb][c] = a.rays_o[size_t(q) * 3 + c];
#else
    zin[nb] = a.z[q];
    znext[nb] = a.z[q + 1 < npts ? q + 1 : q];
#pragma unroll
    for (int c = 0; c < 3; ++c) { oin[nb][c] = a.rays_o[ray_of[nb] * 3 + c]; din[nb][c] = a.rays_d[ray_of[nb] * 3 + c]; }
#endif
  }
#ifdef DFN_MLP_LEAN_TU
  // claimed tiles, as in the coarse kernel: st.next replaces tile + gridDim.x in the three places that name the next tile -- st.more
  // (mid_sync), the input prefetch behind LY_TE0F's mid_sync and tile_coords at the tile's end, all far behind the tile's first mid_sync
  st.claim = 0; st.grid = gridDim.x; st.next = 0; st.n_tiles = uint32_t(n_tiles); st.more = false;
  st.claim_lds = lds_bytes<P, UMB, WAVES, NB, W>() + resident_bytes<P>(true);
  for (; tile < n_tiles; tile = st.next) {
    if (st.wave == 0 && st.lane == 0) st.claim = claim_tile(DFN_ARGS_HERE(a).tile_counter);
    st.claiming = true;
#else
  for (; tile < n_tiles; tile += gridDim.x) {
    st.more = tile + gridDim.x < n_tiles;
#endif
    float x[LP][3];
    uint32_t pt_cur[LP], ray_cur[LP];
#pragma unroll
    for (int nb = 0; nb < LP; ++nb) {
      pt_cur[nb] = pt[nb];
      ray_cur[nb] = ray_of[nb];
#pragma unroll
#ifdef DFN_MLP_PTS_TU
      for (int c = 0; c < 3; ++c) x[nb][c] = xin[nb][c];
#else
      for (int c = 0; c < 3; ++c) x[nb][c] = add_rn(oin[nb][c], mul_rn(din[nb][c], zin[nb]));
#endif
    }
    // per-ray table rows: the pointers are formed where they are used (opaque ray index: not hoisted above the trunk)
    auto ray_table = [&](const float* (&rb)[LP], int half_table) {
#pragma unroll
      for (int nb = 0; nb < LP; ++nb) {
        uint32_t r = ray_cur[nb];
        asm volatile("" : "+v"(r));
        rb[nb] = DFN_ARGS_HERE(a).ray_bias + (size_t)r * ray_bias_floats(W) + half_table * (ray_bias_floats(W) / 2);
      }
    };
    const float* const norb[LP] = {};
    F hid[NB][HC];
#ifdef DFN_TIMING
    {
      const unsigned long long c0 = __builtin_amdgcn_s_memtime();
      float keep = 0.f;
      for (int nb = 0; nb < LP; ++nb) keep += x[nb][0] + x[nb][1] + x[nb][2];
      asm volatile("" ::"v"(keep));   // inputs have arrived
      t_pro += __builtin_amdgcn_s_memtime() - c0;
    }
#endif
    constexpr bool CY = PIPE && P::kSlotsPerChunk == 8, MERGE = UMB >= 8;
    f32x16 carry[NB];
    [[maybe_unused]] uint32_t* mwords = nullptr;
    if constexpr (MASKS) mwords = a.masks + (size_t(tile) * WAVES + st.wave) * (kBwdMaskWords * 64) + st.lane;
    // sign words: trunk layer l -> 2l, 2l + 1; dir_encoding 16; transient_encoding.{0,2,4,6} 17..20 (nerfh_bwd.hip reads them back)
    auto sign128 = [&](int l, F (&h)[HC]) {
      if constexpr (MASKS) {
        uint32_t m[2];
        relu_mask<P, HC>(h, m);
        mwords[(2 * l) * 64] = m[0];
        mwords[(2 * l + 1) * 64] = m[1];
      }
    };
    auto sign64 = [&](int word, F (&h)[QC]) {
      if constexpr (MASKS) {
        uint32_t m[1];
        relu_mask<P, QC>(h, m);
        mwords[word * 64] = m[0];
      }
    };
    if constexpr (MASKS) trunk<P, UMB, PIPE, FAST, NB, W>(st, smem, x, hid, carry, sign128);
    else trunk<P, UMB, PIPE, FAST, NB, W, NoTrunkHook, R_L1>(st, smem, x, hid, carry);
    f32x16 head[NB];
#ifdef DFN_MLP_FOLD_TU
    // static_sigma alone on h8, as the coarse kernel's last layer: it completes h8 (the carry-in of layer 8's last M-block) on the way.
    // `final` is never formed: dir_encoding.0 and transient_encoding.0 below read h8 through the folded weights (LY_DIRF, LY_TE0F)
    // and the per-ray seeds that carry W[:, :128] . b_final.  The carry-in and the head M-block sit where they sit in the coarse
    // kernel, and dir_encoding.0 follows a head M-block as it follows xyz_encoding_final's: the read-hazard rules of layer() hold
    // for this sequence by the same counts.
    static_assert(P::kM16 && !MASKS && W == kWidth, "the folded tail exists for the split-f16 16x16x32 render kernel");
    F (&fin)[NB][HC] = hid;
    {
      F dummy[NB][chunks_of<P>(16)];
      layer<P, UMB, PIPE, NB, HC, 0, false, true, false, R_SIG < 0, (CY ? 6 : -1), true, false, false, false, true, kHalfHeads, R_SIG>(st, smem, hid, dummy, head, norb, carry);
    }
#else
    // xyz_encoding_final (no activation) + static_sigma
    F fin[NB][HC];
    layer<P, UMB, PIPE, NB, HC, MBW, false, true, false, true, (CY ? 6 : -1), true, false>(st, smem, hid, fin, head, norb, carry);
#endif
    sign128(7, hid[0]);   // layer 8's output, completed inside the layer above
    float o[NB][9];
    // the lean unit (kLeanAct4): the four static pre-activations, kept until the transient head's are there (the transient branch's end)
    [[maybe_unused]] float pre_s[NB][4];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      if constexpr (kLeanAct4) pre_s[nb][3] = head[nb][0];
      else o[nb][3] = head_softplus<P, FAST>(head[nb][0]);
    }
    // dir_encoding (per-ray bias = b + W[:,128:] [pe_dir, a]) -> static_rgb
    {
      F de[NB][QC], dummy[NB][chunks_of<P>(16)];
      const float* rb_dir[LP];
      ray_table(rb_dir, 0);
      layer<P, UMB, PIPE, NB, HC, MBQ, true, false, true, true, -1, true, CY>(st, smem, fin, de, head, rb_dir, carry);
#ifdef DFN_MLP_STATIC_TU
      // The next tile's points, prefetched by LDS-DMA as in the fine kernel, whose place for it (behind transient_encoding.0's mid_sync)
      // does not exist here: behind dir_encoding.0's.  In the merged layout (f16: kCoarseStaticGroup puts static_rgb into this unit)
      // that is the tile's LAST mid_sync, so nothing waits for these loads before the tile's end.  In the one- and two-M-block layouts
      // static_rgb opens a unit and its mid_sync's vmcnt(0) covers them together with the weight DMA this unit's mid_sync issued just
      // before them -- what transient_encoding.2's mid_sync does in the fine kernel; no wait in front of a weight DMA is added.
      // layer()'s read-hazard counts for the pair around it: dir_encoding.0 hands its last M-block to static_rgb in `carry` (COUT ->
      // CIN = 2), exactly the pair the fine kernel runs back to back.  The counts there are MFMA issues between an accumulator's last
      // write and the conversion piece that reads it, all of them inside the two layer() bodies; the loads here are VMEM / SALU
      // instructions between the bodies, which add wait states and take no MFMA issue away, and the branch around them is
      // wave-uniform (st.more).  The fine kernel has the same block between a COUT layer and a CIN = 2 layer (t0 -> t1).
      static_assert(!MAPS && !MASKS, "the static query has no maps and saves no masks");
      if (st.more) {
        const uint32_t base = uint32_t(DFN_NEXT_TILE) * uint32_t(PPT) + st.wave * (NB * 32);
        char* slot = smem + ring_slots<P, W>() * USTRIDE + st.wave * (PF_ROUNDS * 8 * 256);
#pragma unroll
        for (int r = 0; r < PF_ROUNDS; ++r) {
          const uint32_t ptn = base + r * 64 + st.lane;
          const uint32_t q = ptn < npts ? ptn : npts - 1;
#pragma unroll
          for (int c = 0; c < 3; ++c) lds_dma_b32(a.rays_o + size_t(q) * 3 + c, slot + (r * 8 + c) * 256);
        }
      }
#endif
      layer<P, UMB, PIPE, NB, QC, 0, false, true, false, !MERGE && R_RGB < 0, (CY ? 2 : -1), true, false, false, false, true, kHalfHeads, R_RGB>(st, smem, de, dummy, head, norb, carry);
      sign64(16, de[0]);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          if constexpr (kLeanAct4) pre_s[nb][c] = head[nb][c];
          else o[nb][c] = head_sigmoid<P, FAST>(head[nb][c]);
        }
    }
#ifndef DFN_MLP_STATIC_TU   // the static query ends behind static_rgb
    // transient branch
    {
      F t0[NB][QC], t1[NB][QC], dummy[NB][chunks_of<P>(16)];
      const float* rb_tr[LP];
      ray_table(rb_tr, 1);
      layer<P, UMB, PIPE, NB, HC, MBQ, true, false, true, true, -1, true, CY>(st, smem, fin, t0, head, rb_tr, carry);
      if (st.more) {
        // Prefetch the next tile's inputs by LDS-DMA (no destination registers).  Issued AFTER this unit's mid_sync so
        // that nothing younger than a weight DMA is ever waited for before the tile's end:
        // lane l of round r fetches z, o, d and the next sample's z of the wave's point 64 r + l into this wave's LDS slot.
        const int wv = wave_here(st);
        const auto& pa = DFN_ARGS_HERE(a);   // rays_o, rays_d, z
        const uint32_t base = uint32_t(DFN_NEXT_TILE) * uint32_t(PPT) + wv * (NB * 32);
        char* slot = smem + ring_slots<P, W>() * USTRIDE + wv * (PF_ROUNDS * 8 * 256);
#pragma unroll
        for (int r = 0; r < PF_ROUNDS; ++r) {
          const uint32_t ptn = base + r * 64 + st.lane;
          const uint32_t q = ptn < npts ? ptn : npts - 1;
#ifdef DFN_MLP_PTS_TU
          // points flavour: the three coordinates of the wave's point 64 r + l (dwords 0..2 of the round's eight)
#pragma unroll
          for (int c = 0; c < 3; ++c) lds_dma_b32(pa.rays_o + size_t(q) * 3 + c, slot + (r * 8 + c) * 256);
#else
          const uint32_t ray = DFN_RAY_OF(a, q);
          lds_dma_b32(pa.z + q, slot + (r * 8) * 256);
          lds_dma_b32(pa.z + (q + 1 < npts ? q + 1 : q), slot + (r * 8 + 7) * 256);
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            lds_dma_b32(pa.rays_o + ray * 3 + c, slot + (r * 8 + 1 + c) * 256);
            lds_dma_b32(pa.rays_d + ray * 3 + c, slot + (r * 8 + 4 + c) * 256);
          }
#endif
        }
      }
      layer<P, UMB, PIPE, NB, QC, MBQ, true, false, false, !MERGE && R_TE1 < 0, (CY ? 2 : -1), true, CY, false, false, true, false, R_TE1>(st, smem, t0, t1, head, norb, carry);
      sign64(17, t0[0]);
      layer<P, UMB, PIPE, NB, QC, MBQ, true, false, false, !MERGE && R_TE2 < 0, (CY ? 2 : -1), true, CY, false, false, true, false, R_TE2>(st, smem, t1, t0, head, norb, carry);
      sign64(18, t1[0]);
      layer<P, UMB, PIPE, NB, QC, MBQ, true, false, false, !MERGE && R_TE3 < 0, (CY ? 2 : -1), true, CY, false, false, true, false, R_TE3>(st, smem, t0, t1, head, norb, carry);
      sign64(19, t0[0]);
      layer<P, UMB, PIPE, NB, QC, 0, false, true, false, !MERGE && R_THEAD < 0, (CY ? 2 : -1), true, false, false, false, true, NOBETA, R_THEAD>(st, smem, t1, dummy, head, norb, carry);
      sign64(20, t1[0]);
#ifdef DFN_MLP_LEAN_TU
      if constexpr (kLeanAct4) {
        // Eight head activations evaluated as four.  A head value of sample p is valid on lane p of half 0 and lanes 32..63 carry no
        // sample from here on: everything below reads o[][] under `live` / `h == 0` (the alphas, s_rgb, the raw store).  So the static
        // pre-activation of sample (lane - 32) is put on lanes 32..63 beside the transient one on lanes 0..31 (v_permlane32_swap_b32 t, s:
        // lanes 32..63 of t <-> lanes 0..31 of s), one sigmoid covers a colour pair and one softplus the two densities, and a second
        // swap against the first one's dead second operand brings the static results back to lanes 0..31.  Per-lane functions of the
        // same arguments: the bits of the separate evaluations.
        static_assert(NOBETA && P::kM16, "the packed activations are the plain fused 16x16x32 kernel's");
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            // (every element goes through a scalar copy: __builtin_bit_cast applied to an ELEMENT of an ext_vector_type value reads element 0)
            const float tv = head[nb][c], sv = pre_s[nb][c];
            const auto in = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(uint32_t, tv), __builtin_bit_cast(uint32_t, sv), false, false);
            const uint32_t in_t = in[0], in_s = in[1];
            const float v = __builtin_bit_cast(float, in_t);
            const float r = c < 3 ? head_sigmoid<P, FAST>(v) : head_softplus<P, FAST>(v);
            const auto out = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(uint32_t, r), in_s, false, false);
            const uint32_t out_t = out[0], out_s = out[1];
            o[nb][4 + c] = __builtin_bit_cast(float, out_t);
            o[nb][c] = __builtin_bit_cast(float, out_s);
          }
          o[nb][8] = 0.f;
        }
      } else
#endif
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
#pragma unroll
        for (int c = 0; c < 3; ++c) o[nb][4 + c] = head_sigmoid<P, FAST>(head[nb][c]);
        o[nb][7] = head_softplus<P, FAST>(head[nb][3]);
        if constexpr (NOBETA) o[nb][8] = 0.f;
        else o[nb][8] = head_softplus<P, FAST>(head[nb][4]);  // C register 4 of half 0 = row 8 = transient_beta
      }
    }
#endif
    // the lane's own sample (sample p on lane p of half 0, as the heads): PrecX3M16 lane 16 g + (l & 15) carries it as point n = g & 1
#ifdef DFN_MLP_PTS_TU
    // points have no depths: the raw store below is the only epilogue (launch_mlp_pts refuses a.partial)
    uint32_t pt_own[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      if constexpr (P::kM16) pt_own[nb] = (st.lane & 16) != 0 ? pt_cur[1] : pt_cur[0];
      else pt_own[nb] = pt_cur[nb];
    }
    {
#else
    uint32_t pt_own[NB], ray_own[NB];
    float z_own[NB], zn_own[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      if constexpr (P::kM16) {
        const bool n1 = (st.lane & 16) != 0;
        pt_own[nb] = n1 ? pt_cur[1] : pt_cur[0];
        ray_own[nb] = n1 ? ray_cur[1] : ray_cur[0];
        z_own[nb] = n1 ? zin[1] : zin[0];
        zn_own[nb] = n1 ? znext[1] : znext[0];
      } else {
        pt_own[nb] = pt_cur[nb]; ray_own[nb] = ray_cur[nb]; z_own[nb] = zin[nb]; zn_own[nb] = znext[nb];
      }
    }
    if (DFN_ARGS_HERE(a).partial) {
      // Fused compositing (n_samples % (32 NB) == 0): this wave holds 32 NB consecutive samples of ONE ray, sample
      // 32 nb + p on lane p of half 0.  Transmittance factorises over segments, so the wave composites its
      // segment locally (products P and sums relative to the segment start) and a tiny combine pass chains
      // the segments of a ray (nerfh_stages.hip: composite_combine_kernel).  `raw` never reaches HBM.
      const bool live = h == 0;
      float Pj = 1.f, Ps = 1.f;                    // running products through the previous blocks of the segment
      float s_rgb[3] = {0.f, 0.f, 0.f}, s_acc = 0.f, s_dso = 0.f, s_dj = 0.f, s_beta = 0.f;
      [[maybe_unused]] float s_rs[3] = {0.f, 0.f, 0.f}, s_rt[3] = {0.f, 0.f, 0.f};   // MAPS: static-only / transient colour
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        const uint32_t smp = pt_own[nb] - ray_own[nb] * uint32_t(a.n_samples);
        const float delta = smp + 1 == uint32_t(a.n_samples) ? 1e2f : sub_rn(zn_own[nb], z_own[nb]);
        const float sg_s = o[nb][3], sg_t = o[nb][7];
        const float as = live ? sub_rn(1.f, head_exp<P, FAST>(-mul_rn(delta, sg_s))) : 0.f;
        const float at = live ? sub_rn(1.f, head_exp<P, FAST>(-mul_rn(delta, sg_t))) : 0.f;
        const float aj = live ? sub_rn(1.f, head_exp<P, FAST>(-mul_rn(delta, add_rn(sg_s, sg_t)))) : 0.f;
        // scans over the block's 32 samples on the DPP crossbar (lanes 32..63 carry alpha = 0: the identity), five VALU
        // instructions each instead of six dependent ds_bpermute round trips (nerfh_device.h)
        const float ij = scan32_prod(1.f - aj), is = scan32_prod(1.f - as);
        const float ej = lane_shr1(ij, 1.f), es = lane_shr1(is, 1.f);   // exclusive products (lane 0: 1)
        const float Tj = Pj * ej, Ts = Ps * es;
        const float ws = as * Tj, wt = at * Tj, wj = aj * Tj;
#pragma unroll
        for (int c = 0; c < 3; ++c) s_rgb[c] += live ? ws * o[nb][c] + wt * o[nb][4 + c] : 0.f;
        s_acc += wj;
        s_dso += as * Ts * z_own[nb];
        s_dj += wj * z_own[nb];
        if constexpr (!NOBETA) s_beta += live ? wt * o[nb][8] : 0.f;
        if constexpr (MAPS) {
          // rendering.py:218-227 (the static field under its own transmittance), :201-203 (the transient layer under the joint one).
          // The transient weight goes through an opaque copy: its products must not be shared with s_rgb's, whose rounding
          // (and so the bits of rgb) stays that of the kernel without the maps.
          float wt_m = wt;
          asm volatile("" : "+v"(wt_m));
          const float wso = as * Ts;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            s_rs[c] += live ? wso * o[nb][c] : 0.f;
            s_rt[c] += live ? wt_m * o[nb][4 + c] : 0.f;
          }
        }
        Pj *= read_lane31(ij);   // lane 31 holds the block's full product
        Ps *= read_lane31(is);
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) s_rgb[c] = read_lane31(scan32_sum(s_rgb[c]));   // lanes 32..63 contribute zeros
      s_acc = read_lane31(scan32_sum(s_acc)); s_dso = read_lane31(scan32_sum(s_dso));
      s_dj = read_lane31(scan32_sum(s_dj));
      if constexpr (!NOBETA) s_beta = read_lane31(scan32_sum(s_beta));
      if constexpr (MAPS) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { s_rs[c] = read_lane31(scan32_sum(s_rs[c])); s_rt[c] = read_lane31(scan32_sum(s_rt[c])); }
      }
      if (st.lane == 0 && pt_own[0] < npts) {
        constexpr int REC = MAPS ? kMapsRecFloats : 12;
        f32x4* dst = reinterpret_cast<f32x4*>(DFN_ARGS_HERE(a).partial + (size_t)(pt_own[0] / uint32_t(NB * 32)) * REC);   // one segment per wave
        dst[0] = f32x4{s_rgb[0], s_rgb[1], s_rgb[2], s_acc};
        dst[1] = f32x4{s_dso, s_dj, s_beta, Pj};
        if constexpr (MAPS) {
          dst[2] = f32x4{Ps, s_rs[0], s_rs[1], s_rs[2]};
          dst[3] = f32x4{s_rt[0], s_rt[1], s_rt[2], 0.f};
        } else {
          dst[2] = f32x4{Ps, 0.f, 0.f, 0.f};
        }
      }
    } else {
#endif
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
        if (h == 0 && pt_own[nb] < npts) {
#ifdef DFN_MLP_STATIC_TU
          float* dst = a.out + (size_t)pt_own[nb] * 4;   // raw4 = (rgb_s, sigma_s); no alignment beyond a float's is asked of the caller
#pragma unroll
          for (int c = 0; c < 4; ++c) dst[c] = o[nb][c];
#else
          float* dst = a.out + (size_t)pt_own[nb] * 9;
#pragma unroll
          for (int c = 0; c < 9; ++c) dst[c] = o[nb][c];
#endif
        }
    }
    if (st.more) {  // pick up the prefetched inputs of the next tile (this wave's own LDS slot: no barrier needed)
      __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
      asm volatile("" ::: "memory");
      tile_coords(DFN_NEXT_TILE);
      const char* slot = smem + ring_slots<P, W>() * USTRIDE + st.wave * (PF_ROUNDS * 8 * 256);
#pragma unroll
      for (int nb = 0; nb < LP; ++nb) {
        int loc = P::kM16 ? 16 * nb + (st.lane & 15) : nb * 32 + p;
        asm volatile("" : "+v"(loc));   // formed here: as a loop invariant it was hoisted to the prologue and spilled
        const int r = loc >> 6, l = loc & 63;
        const float* f = reinterpret_cast<const float*>(slot + r * 8 * 256) + l;
#ifdef DFN_MLP_PTS_TU
#pragma unroll
        for (int c = 0; c < 3; ++c) xin[nb][c] = f[c * 64];
#else
        zin[nb] = f[0];
        znext[nb] = f[7 * 64];
#pragma unroll
        for (int c = 0; c < 3; ++c) { oin[nb][c] = f[(1 + c) * 64]; din[nb][c] = f[(4 + c) * 64]; }
#endif
      }
    }
  }
  range_report<P>(st.rmax, a.status);
#ifdef DFN_TIMING
  if (a.timing && st.lane == 0) {
    unsigned long long* t = a.timing + (blockIdx.x * WAVES + st.wave) * 4;
    t[0] = __builtin_amdgcn_s_memtime() - t_begin;
    t[1] = st.t_wait;
    t[2] = st.t_sync;
    t[3] = t_pro;
  }
#endif
}

// ------------------------------------------------------------------------------------------
// The launch every launcher below ends in.  kern: the kernel the launcher picked, null where it refuses the arguments (an empty launch
// succeeds before that is looked at); attr_done: the launcher's flag of this kernel, so that its LDS size is set once per kernel.
static int dma_waves_env() {   // DFN_DMA_WAVES=n: A/B aid, read once
  static int env = -1;
  if (env < 0) { const char* e = getenv("DFN_DMA_WAVES"); env = e ? atoi(e) : 0; }
  return env;
}
template <class A, int PPT, int WG_PER_CU, int WAVES>
static hipError_t launch_tiles(void (*kern)(A), bool& attr_done, uint32_t lds, const A& a, int n_cu, hipStream_t stream) {
  const long long n_pts = (long long)a.n_rays * a.n_samples;
  if (n_pts <= 0) return hipSuccess;
  if (n_pts >= (1LL << 31) || !kern) return hipErrorInvalidValue;  // kernels index points with 32 bits; callers chunk
  const long long n_tiles = (n_pts + PPT - 1) / PPT;
  const long long slots = (long long)n_cu * WG_PER_CU;  // resident workgroups
  const int grid = int(n_tiles < slots ? n_tiles : slots);
  if (!attr_done) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
    if (e != hipSuccess) return e;
    attr_done = true;
  }
  A b = a;
  // 8-wave workgroups: the four older waves idle a third of their time at the unit barriers
  if (b.dma_waves == 0) b.dma_waves = dma_waves_env() > 0 ? dma_waves_env() : (WAVES == 8 ? 4 : WAVES);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(WAVES * 64), lds, stream, b);
  return hipGetLastError();
}
// the geometry of the PrecX3M16 kernels of variants 5 to 12: variant 4's (launch_one<PrecX3M16, false, 8, 2, 1, 1, true> below)
using PM = PrecX3M16;
constexpr int kMWaves = 8, kMUmb = unit_mb<PM>(0), kMNb = 1, kMPpt = kMWaves * kMNb * 32;

#if defined(DFN_MLP_PTS_TU)
// The points flavour's launchers.  One geometry per (unit, arithmetic), the one the raw route of the ray entries runs at the default
// kernel variant, so that a point equal to o + d z gives the bits the ray entry gives.
template <class P, bool FAST, int WAVES, int UMB, int NB, bool PIPE, int W, bool FINE>
static hipError_t launch_pts_one(const MlpArgs& a, int n_cu, hipStream_t stream) {
  void (*kern)(MlpArgs) = nullptr;
  if constexpr (FINE) kern = DFN_FINE_KERNEL<P, FAST, WAVES, UMB, NB, PIPE, W>;
  else kern = DFN_COARSE_KERNEL<P, FAST, WAVES, UMB, NB, PIPE, W>;
  if (a.masks || a.partial || !a.rays_o || !a.out) kern = nullptr;   // raw route only: points have no depths to composite along
  static bool attr_done = false;
  return launch_tiles<MlpArgs, WAVES * NB * 32, 1, WAVES>(kern, attr_done, lds_bytes<P, UMB, WAVES, NB, W>(), a, n_cu, stream);
}
#if defined(DFN_MLP_STATIC_TU)
// The coarse network's training query: the geometries of the fine point query per (arithmetic, width), on the networks packed along
// kCoarseStaticSeq / kCoarseStaticFoldSeq; a.ray_bias = the coarse dir_encoding.0's seed table (one row per query row, table 0 only).
#if defined(DFN_MLP_FOLD_TU)
// launch_mlp_static_pts_fold: split-f16, netwidth 128 (PrecX3M16, the folded tail)
hipError_t DFN_LAUNCH_MLP(const MlpArgs& a, int n_cu, hipStream_t stream) {
  if (!a.ray_bias) return hipErrorInvalidValue;
  return launch_pts_one<PM, false, kMWaves, kMUmb, kMNb, true, kWidth, true>(a, n_cu, stream);
}
#else
// launch_mlp_static_pts: f16 and exact fp32 at netwidth 128, the three plain kernels of netwidth 256
hipError_t DFN_LAUNCH_MLP(int prec, const MlpArgs& a, int n_cu, hipStream_t stream, int width) {
  if (!a.ray_bias) return hipErrorInvalidValue;
  if (width == 256) {
    if (prec == 0) return launch_pts_one<PrecF16, true, 8, unit_mb_w256<PrecF16>(), 1, false, 256, true>(a, n_cu, stream);
    if (prec == 2) return launch_pts_one<PrecX3, false, 4, unit_mb_w256<PrecX3>(), 1, false, 256, true>(a, n_cu, stream);
    return launch_pts_one<PrecF32, false, 4, unit_mb_w256<PrecF32>(), 1, false, 256, true>(a, n_cu, stream);
  }
  if (width != kWidth || prec == 2) return hipErrorInvalidValue;   // split-f16 at netwidth 128: launch_mlp_static_pts_fold
  if (prec == 0) return launch_pts_one<PrecF16, true, 8, 8, 2, true, kWidth, true>(a, n_cu, stream);
  return launch_pts_one<PrecF32, false, 8, 1, 1, false, kWidth, true>(a, n_cu, stream);
}
#endif
#elif defined(DFN_MLP_HALF_TU)
// launch_mlp_pts_half: split-f16, netwidth 128, coarse: variant 6's half-height kernel on net[0][F16X3][6]
hipError_t DFN_LAUNCH_MLP(const MlpArgs& a, int n_cu, hipStream_t stream) {
  return launch_pts_one<PM, false, kMWaves, kMUmb, kMNb, true, kWidth, false>(a, n_cu, stream);
}
#elif defined(DFN_MLP_FOLD_TU)
// launch_mlp_pts_fold: split-f16, netwidth 128, fine: variant 5's folded kernel on net[1][F16X3][5], a.ray_bias from rb_fold
hipError_t DFN_LAUNCH_MLP(const MlpArgs& a, int n_cu, hipStream_t stream) {
  return launch_pts_one<PM, false, kMWaves, kMUmb, kMNb, true, kWidth, true>(a, n_cu, stream);
}
#else
// launch_mlp_pts: f16 and exact fp32 at netwidth 128 (their variant-0 kernels) and the three plain kernels of netwidth 256, as
// launch_mlp picks them
hipError_t DFN_LAUNCH_MLP(bool fine, int prec, const MlpArgs& a, int n_cu, hipStream_t stream, int width) {
  if (width == 256) {
    if (prec == 0) {
      return fine ? launch_pts_one<PrecF16, true, 8, unit_mb_w256<PrecF16>(), 1, false, 256, true>(a, n_cu, stream)
                  : launch_pts_one<PrecF16, true, 8, unit_mb_w256<PrecF16>(), 1, false, 256, false>(a, n_cu, stream);
    }
    if (prec == 2) {
      return fine ? launch_pts_one<PrecX3, false, 4, unit_mb_w256<PrecX3>(), 1, false, 256, true>(a, n_cu, stream)
                  : launch_pts_one<PrecX3, false, 4, unit_mb_w256<PrecX3>(), 1, false, 256, false>(a, n_cu, stream);
    }
    return fine ? launch_pts_one<PrecF32, false, 4, unit_mb_w256<PrecF32>(), 1, false, 256, true>(a, n_cu, stream)
                : launch_pts_one<PrecF32, false, 4, unit_mb_w256<PrecF32>(), 1, false, 256, false>(a, n_cu, stream);
  }
  if (width != kWidth) return hipErrorInvalidValue;
  if (prec == 0) {
    return fine ? launch_pts_one<PrecF16, true, 8, 8, 2, true, kWidth, true>(a, n_cu, stream)
                : launch_pts_one<PrecF16, true, 8, 8, 2, true, kWidth, false>(a, n_cu, stream);
  }
  if (prec == 2) return hipErrorInvalidValue;   // split-f16 at netwidth 128: launch_mlp_pts_half (coarse), launch_mlp_pts_fold (fine)
  return fine ? launch_pts_one<PrecF32, false, 8, 1, 1, false, kWidth, true>(a, n_cu, stream)
              : launch_pts_one<PrecF32, false, 8, 1, 1, false, kWidth, false>(a, n_cu, stream);
}
#endif
#elif defined(DFN_MLP_RES_TU)
// launch_mlp_res: variant 7's kernels, variant 6's geometry with the resident region behind the input slots.  coarse; fine with the
// compositing fused, plain flavour -- the maps flavour stays with launch_mlp_half, the raw route with launch_mlp_fold.
// launch_mlp_lean (this body in nerfh_mlp_lean.hip): variant 12's kernels, the same with the claimed-tile word behind the region.  The
// grid is variant 7's: min(tiles, CUs) workgroups, each starting on tile blockIdx.x; *a.tile_counter is 0 at the start (the caller's
// memset); a.ray_bias holds in_scale x the seeds; the magic number of a.n_samples is formed here.
#ifdef DFN_MLP_LEAN_TU
hipError_t DFN_LAUNCH_MLP(bool fine, const MlpLeanArgs& in, int n_cu, hipStream_t stream) {
  MlpLeanArgs a = in;
  a.div = ray_div_of(uint32_t(in.n_samples > 0 ? in.n_samples : 1));
#else
hipError_t DFN_LAUNCH_MLP(bool fine, const MlpResArgs& a, int n_cu, hipStream_t stream) {
#endif
  void (*kern)(DFN_MLP_KARGS) = fine ? DFN_FINE_KERNEL<PM, false, kMWaves, kMUmb, kMNb, true> : DFN_COARSE_KERNEL<PM, false, kMWaves, kMUmb, kMNb, true>;
  uint32_t lds = lds_bytes<PM, kMUmb, kMWaves, kMNb>() + resident_bytes<PM>(fine);
  if (a.masks || (fine && !a.partial)) kern = nullptr;
  if (!a.res_blob || a.res_bytes != resident_bytes<PM>(fine)) kern = nullptr;   // the kernels copy exactly this many bytes
#ifdef DFN_MLP_LEAN_TU
  if (!a.tile_counter) kern = nullptr;
  lds += kClaimBytes;
#endif
  static bool attr_done[2] = {false, false};
  return launch_tiles<DFN_MLP_KARGS, kMPpt, 1, kMWaves>(kern, attr_done[fine], lds, a, n_cu, stream);
}
#elif defined(DFN_MLP_HALF_TU)
// launch_mlp_half: variant 6's kernels.  coarse; fine with the compositing fused, plain or render-maps flavour -- the raw route
// (a.partial == nullptr) stays with launch_mlp_fold.
hipError_t DFN_LAUNCH_MLP(bool fine, bool maps, const MlpArgs& a, int n_cu, hipStream_t stream) {
  void (*kern)(MlpArgs) = !fine ? nerfh_coarse_half_kernel<PM, false, kMWaves, kMUmb, kMNb, true>
                          : maps ? nerfh_fine_half_kernel<PM, false, kMWaves, kMUmb, kMNb, true, kWidth, false, true>
                                 : nerfh_fine_half_kernel<PM, false, kMWaves, kMUmb, kMNb, true>;
  if (a.masks || (fine && !a.partial) || (maps && !fine)) kern = nullptr;
  static bool attr_done[3] = {false, false, false};
  return launch_tiles<MlpArgs, kMPpt, 1, kMWaves>(kern, attr_done[fine ? (maps ? 2 : 1) : 0], lds_bytes<PM, kMUmb, kMWaves, kMNb>(), a, n_cu, stream);
}
#elif defined(DFN_MLP_FOLD_TU)
// launch_mlp_fold: variant 5's fine kernel, plain or render-maps flavour
hipError_t DFN_LAUNCH_MLP(bool maps, const MlpArgs& a, int n_cu, hipStream_t stream) {
  void (*kern)(MlpArgs) = maps ? nerfh_fine_fold_kernel<PM, false, kMWaves, kMUmb, kMNb, true, kWidth, false, true>
                               : nerfh_fine_fold_kernel<PM, false, kMWaves, kMUmb, kMNb, true>;
  if (a.masks || (maps && !a.partial)) kern = nullptr;
  static bool attr_done[2] = {false, false};
  return launch_tiles<MlpArgs, kMPpt, 1, kMWaves>(kern, attr_done[maps], lds_bytes<PM, kMUmb, kMWaves, kMNb>(), a, n_cu, stream);
}
#else
template <class P, bool FAST, int WAVES, int UMB, int NB, int WG_PER_CU, bool PIPE, int W = kWidth>
static hipError_t launch_one(bool fine, const MlpArgs& a, int n_cu, hipStream_t stream) {
  void (*kern)(MlpArgs) = nullptr;
  int slot = fine ? 1 : 0;
  if constexpr (kMapsTU) {
    // render maps: the fused fine kernel with the kMapsRecFloats-float segment record, where the fused compositing exists at all
    if constexpr (W == kWidth && NB <= 2) {
      if (fine && a.partial && !a.masks) kern = nerfh_fine_kernel<P, FAST, WAVES, UMB, NB, PIPE, W, false, true>;
    }
  } else {
    kern = fine ? nerfh_fine_kernel<P, FAST, WAVES, UMB, NB, PIPE, W> : nerfh_coarse_kernel<P, FAST, WAVES, UMB, NB, PIPE, W>;
    if constexpr (P::kSplit && !P::kM16 && NB == 1 && WAVES == 8 && W == kWidth && PIPE) {
      if (fine && a.masks) { kern = nerfh_fine_kernel<P, FAST, WAVES, UMB, NB, PIPE, W, true>; slot = 2; }
    } else if (a.masks) kern = nullptr;
  }
  static bool attr_done[3] = {false, false, false};
  return launch_tiles<MlpArgs, WAVES * NB * 32, WG_PER_CU, WAVES>(kern, attr_done[slot], lds_bytes<P, UMB, WAVES, NB, W>(), a, n_cu, stream);
}

// variant 0: 8 waves x NB 2, 1 WG/CU, unit = layer, epilogue pipelined into the next M-block's MFMAs
// variant 1: 4 waves x NB 2, 2 WG/CU, unit = 2 M-blocks  (2 waves/SIMD from different workgroups)
// variant 2: 4 waves x NB 3, 1 WG/CU, unit = layer      (1 wave/SIMD, 512 registers, pipelined epilogue)
// variant 3: variant 0 without the pipelined epilogue (A/B reference)
// variant 4: split-f16 as variant 0 on 16x16x32 MFMAs (PrecX3M16); f16 and exact fp32 run their variant-0 kernels
// launch_mlp_maps (this body in nerfh_mlp_maps.hip): the fine kernels' render-maps flavour (fused compositing only: fine, a.partial
// with kMapsRecFloats floats per segment; the 3-block f16 variant and netwidth 256 have none and are refused).
// netwidth 256: the plain variants (one point block per wave, no pipelined epilogue); staging units of 2 M-blocks (f16) /
// 1 M-block (f32, split-f16) keep three buffers inside the 160 KB of LDS (a 256 x 256 f16 layer is 128 KB).
hipError_t DFN_LAUNCH_MLP(bool fine, int prec, int variant, const MlpArgs& a, int n_cu, hipStream_t stream, int width) {
  if (width == 256) {
    if (prec == 0) {
      return launch_one<PrecF16, true, 8, unit_mb_w256<PrecF16>(), 1, 1, false, 256>(fine, a, n_cu, stream);
    }
    if (prec == 2) return launch_one<PrecX3, false, 4, unit_mb_w256<PrecX3>(), 1, 1, false, 256>(fine, a, n_cu, stream);
    return launch_one<PrecF32, false, 4, unit_mb_w256<PrecF32>(), 1, 1, false, 256>(fine, a, n_cu, stream);
  }
  if (width != kWidth) return hipErrorInvalidValue;
  if (variant == 4 && prec != 2) variant = 0;
  if (prec == 0) {
    if (variant == 0) return launch_one<PrecF16, true, 8, 8, 2, 1, true>(fine, a, n_cu, stream);
    if (variant == 1) return launch_one<PrecF16, true, 4, 2, 2, 1, true>(fine, a, n_cu, stream);
    if (variant == 2) return launch_one<PrecF16, true, 4, 8, 3, 1, true>(fine, a, n_cu, stream);
    return launch_one<PrecF16, true, 8, 8, 2, 1, false>(fine, a, n_cu, stream);
  }
  if (prec == 2) {  // split-f16: variant 3 = without the pipelined epilogue (A/B reference), every other variant with it
    if (variant == 3) return launch_one<PrecX3, false, 8, unit_mb<PrecX3>(0), 1, 1, false>(fine, a, n_cu, stream);
    if (variant == 4) return launch_one<PrecX3M16, false, 8, unit_mb<PrecX3M16>(0), 1, 1, true>(fine, a, n_cu, stream);
    return launch_one<PrecX3, false, 8, unit_mb<PrecX3>(0), 1, 1, true>(fine, a, n_cu, stream);
  }
  if (variant == 1) return launch_one<PrecF32, false, 4, 1, 1, 1, false>(fine, a, n_cu, stream);
  return launch_one<PrecF32, false, 8, 1, 1, 1, false>(fine, a, n_cu, stream);
}
#endif  // DFN_MLP_FOLD_TU

}  // namespace dfn
