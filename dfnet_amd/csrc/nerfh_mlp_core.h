// nerfh_mlp_core.h — device building blocks of the register-resident NeRF-H MLP, shared by the forward kernels
// (nerfh_mlp.hip) and the input-gradient kernel (nerfh_bwd.hip): weight staging (Stager / begin_unit), the
// generic MFMA layer, the positional encoding and the 8-layer trunk.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mfma_frag.h"
#include "nerfh_device.h"
#include "nerfh_kernels.h"
#include "nerfh_layout.h"

#ifndef DFN_PF
#define DFN_PF 3  // f16 A fragments in flight per wave
#endif

namespace dfn {

// chunks (B-operand registers groups) per 32 produced features / per n slots
template <class P> constexpr int chunks_of(int slots) { return slots / P::kSlotsPerChunk; }
// sample points per lane and point block: PrecX3M16 lanes carry one point of each 16-point N-block (16 nb + (lane & 15))
template <class P> constexpr int lane_pts(int NB) { return P::kM16 ? 2 : NB; }
// Split-f16 result pair i (accumulator registers 2i, 2i + 1 of an M-block) -> B chunk (2 mb + x3_chunk) and position x3_pos, x3_pos + 1
// of the next layer's operand: 32x32 = rows of the two 16-K halves; PrecX3M16 = fragment q = i >> 1 (N-block q & 1, rows 16 (q >> 1) ..)
template <class P> DFN_HD constexpr int x3_chunk(int i) { return P::kM16 ? (i >> 1) & 1 : i >> 2; }
template <class P> DFN_HD constexpr int x3_pos(int i) { return P::kM16 ? 4 * (i >> 2) + 2 * (i & 1) : 2 * (i & 3); }

template <class P, int KC>
DFN_DEV void set_slot(typename FragOf<P>::type (&arr)[KC], int s, float v) {
  if constexpr (P::kSplit) {
    _Float16 hi, lo;
    x3_split(v, hi, lo);
    arr[s >> 3].hi[s & 7] = hi;
    arr[s >> 3].lo[s & 7] = lo;
  } else if constexpr (P::kSlotsPerChunk == 8) arr[s >> 3][s & 7] = (_Float16)v;
  else arr[s] = v;
}

// ------------------------------------------------------------------------------------------
// Weight staging: the packed blob is a sequence of units (offset, bytes) in execution order.
struct Stager {
  const char* blob;
  const uint32_t* tab;
  int n_units;
  int u;               // unit that the NEXT open_unit() returns
  uint32_t slot;       // ring slot holding (or receiving) unit u
  uint32_t ring;       // staging buffers in the ring (3)
  uint32_t ustride;    // bytes per ring slot
  int lane, wave, waves;
  int dma_waves;       // the first dma_waves waves issue the weight DMA (the older wave of each SIMD idles at the unit barriers anyway)
  uint32_t ubase, uoff;      // LDS offset of the open unit / bytes of it consumed by the layers so far
  uint32_t pf_off, pf_size;  // table entry of the unit the NEXT mid_sync() will start streaming (prefetched)
  unsigned long long t_sync, t_wait, t_last;  // DFN_TIMING: cycles in unit waits / barrier
  unsigned long long* trace;
  int n_trace;
  bool more;           // another tile follows this one (wave-uniform)
#ifdef DFN_MLP_LEAN_TU
  // The lean unit (nerfh_mlp_lean.hip): the tile after this one is CLAIMED -- lane 0 of wave 0 issues a returning atomic add on the
  // launch's tile counter at the top of the tile; the first mid_sync() of the tile publishes the result through one LDS word around
  // its barrier and sets `next` and `more` in every wave.  `more` is first read by the mid_sync() of the tile's second-to-last
  // streamed unit (the wrap to the next tile), many units later.
  uint32_t claim;      // lane 0 of wave 0: the counter's value before the add (pending until the first mid_sync's vmcnt(0))
  uint32_t grid;       // gridDim.x: tile = grid + claim
  uint32_t next;       // the tile this workgroup computes after the current one (wave-uniform; >= n_tiles: none)
  uint32_t n_tiles;
  uint32_t claim_lds;  // LDS byte offset of the published word (behind the resident region)
  bool claiming;       // a claim was issued at the top of this tile and is not published yet (wave-uniform)
#endif
  float in_scale, out_scale;  // split-f16: accumulators carry in_scale x the true value (MlpArgs), out_scale = 1 / in_scale
  float lane_mul;             // split-f16: extra per-LANE power-of-two factor on the next layer's outputs (gradient renormalisation)
  uint32_t rmax;              // range guard: running unsigned maximum of the packed f16 activations (hi halves for split-f16) this
                              // lane has produced, sign bits cleared: >= 0x7c00 = an inf, 0x7bff = the saturation value
};

// Range guard of the narrow arithmetic modes.  A ReLU output is a non-negative f16, so its bit pattern orders like the value: one
// v_pk_max_u16 per converted register keeps the largest pattern seen; layers without ReLU clear the sign bits first.  Checked
// once per kernel (range_report): f16 conversions overflow to inf (0x7c00), the split-f16 hi halves are truncating conversions
// that saturate at 65504 (0x7bff).
DFN_DEV uint32_t pk_max_u16(uint32_t a, uint32_t b) {
  uint32_t r;
  asm("v_pk_max_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
DFN_DEV void range_track(uint32_t& rmax, uint32_t packed, bool nonneg) {
  rmax = pk_max_u16(rmax, nonneg ? packed : (packed & 0x7fff7fffu));
}
template <class P>
DFN_DEV void range_report(uint32_t rmax, int* status) {
  if constexpr (P::kSlotsPerChunk == 8) {
    const uint32_t thr = P::kSplit ? 0x7bffu : 0x7c00u;
    if (status && ((rmax & 0xffffu) >= thr || (rmax >> 16) >= thr)) atomicOr(status, P::kSplit ? 2 : 1);
  }
}

// Direct-to-LDS DMA, issued as inline asm ON PURPOSE.  With the builtin, LLVM cannot tell which LDS bytes a DMA
// writes and makes EVERY later ds_read wait for vmcnt(0) (SIInsertWaitcnts, LDS-DMA aliasing): the first A-fragment
// read after a unit's DMA was issued then stalls for the whole L2 round trip, every unit (measured: 20 % of the
// kernel).  Here the landing is awaited explicitly (mid_sync: counted vmcnt + barrier) before any wave reads it.
// The compiler's own vmcnt bookkeeping stays safe: memory returns in order and it can only under-count loads that
// are in flight, so its waits are at worst longer than needed.  wave-contiguous: lane l writes 16 (4) bytes at
// lds_off + 16 l (4 l).
DFN_DEV void lds_dma_b128(const void* gptr, const char* lds_dst) {
  const uint32_t off = (uint32_t)(size_t)DFN_LDS_PTR(lds_dst);
  asm volatile("s_mov_b32 m0, %1\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(gptr), "s"(off) : "memory");
}
DFN_DEV void lds_dma_b32(const void* gptr, const char* lds_dst) {
  const uint32_t off = (uint32_t)(size_t)DFN_LDS_PTR(lds_dst);
  asm volatile("s_mov_b32 m0, %1\n\tglobal_load_lds_dword %0, off" ::"v"(gptr), "s"(off) : "memory");
}
#ifdef DFN_MLP_LEAN_TU
// The lean unit: one lane's claim, a returning device-scope atomic add whose result nobody waits for here (mid_sync's vmcnt(0) does).
// The pointer goes through an opaque vector register: on an address it can prove wave-uniform LLVM's atomic optimiser rewrites the add
// as a wave reduction + v_readfirstlane of the result, and with that a wait for the whole L2 round trip right behind the atomic.
// Named a GLOBAL address again behind it: a flat atomic counts in vmcnt and lgkmcnt both and turns every counted wait behind it into 0.
// The LDS word the claim is published through, named in the LDS address space (through the generic pointer it is a flat access).
typedef volatile uint32_t __attribute__((address_space(3))) lds_vu32;
DFN_DEV lds_vu32* claim_word(char* smem, uint32_t off) { return reinterpret_cast<lds_vu32*>(DFN_LDS_PTR(smem + off)); }
DFN_DEV uint32_t claim_tile(uint32_t* counter) {
  typedef uint32_t __attribute__((address_space(1))) global_u32;
  uint64_t p = reinterpret_cast<uint64_t>(counter);
  asm volatile("" : "+v"(p));
  return __hip_atomic_fetch_add(reinterpret_cast<global_u32*>(p), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
#endif

DFN_DEV void stage_issue_at(const Stager& st, char* smem, uint32_t off, uint32_t size, uint32_t lds_off) {
  const char* src = st.blob + off + st.lane * 16;
#ifdef DFN_MLP_LEAN_TU
  // the lean unit: whether this wave issues DMA and where its first piece lies are formed HERE from the wave index.  As loop
  // invariants of the tile loop the condition (a 64-bit lane mask) and the 64-bit offset (wave * kPiece, 0) were hoisted to the
  // prologue, parked in VGPR lanes and read back by v_readlane_b32 pairs in front of every unit's DMA: 88 of the 223 reads of parked
  // SGPRs per tile in the fine kernel without this.  Behind the opaque copy they are one scalar compare and one scalar shift per unit.
  uint32_t w = st.wave;
  asm volatile("" : "+s"(w));
  if (int(w) >= st.dma_waves) return;
  for (uint32_t p = w * kPiece; p < size; p += st.dma_waves * kPiece) lds_dma_b128(src + p, smem + lds_off + p);
#else
  if (st.wave >= st.dma_waves) return;
  for (uint32_t p = st.wave * kPiece; p < size; p += st.dma_waves * kPiece) lds_dma_b128(src + p, smem + lds_off + p);
#endif
}
// The unit table is read through the CONSTANT address space so that the loads are scalar (s_load, lgkmcnt): as
// vector loads they would sit in the vmcnt queue behind the DMA and every wait for them would wait for the DMA too.
typedef const uint32_t __attribute__((address_space(4))) const_u32;
DFN_DEV uint32_t tab_entry(const Stager& st, int i) {
  return reinterpret_cast<const_u32*>(reinterpret_cast<uint64_t>(st.tab))[i];
}
DFN_DEV void stage_issue(const Stager& st, char* smem, int unit, uint32_t lds_off) {
  stage_issue_at(st, smem, tab_entry(st, 2 * unit), tab_entry(st, 2 * unit + 1), lds_off);
}

// Three staging buffers rotate: while unit u is computed out of `lds_nn`... (see below) the DMA of unit u+1 is
// landing and unit u+2's is issued.  Synchronisation happens in the MIDDLE of a unit, not at its boundary:
//   open_unit()  no wait at all: the unit it returns was made visible by the mid_sync() of the previous unit;
//   mid_sync()   called once while a unit is being computed: wait for this wave's share of the NEXT unit (issued
//                a whole unit ago), barrier (every share landed; every wave has left the unit before this one),
//                then start the DMA of the unit after next into the buffer the previous unit occupied.
// So a wave flows from one layer into the next without stopping, and the barrier falls where both waves of a
// SIMD still have MFMAs queued on either side of it.
// What the ablations say about the remaining cost of streaming (fine kernel, one run): no barrier +4 %, no DMA
// +21 %, same DMA instructions with a quarter of the bytes +19 %, half the pieces +16 %, every piece from one
// cached KiB +2 %; staggering the two waves of a SIMD, or staging through VGPRs + ds_write_b128 instead of the
// DMA: no gain / -2.5 %.  The cost follows the BYTES landing in LDS, not instructions, waits or L2; a third of
// it is shader cycles, two thirds is clock (the traffic is paid in power: DESIGN.md section 3.1).
DFN_DEV void stage_prime(Stager& st, char* smem, uint32_t unit_stride, uint32_t ring = 3) {
  st.slot = 0; st.ring = ring; st.ustride = unit_stride;
  st.u = 0;
  stage_issue(st, smem, 0, 0);
  stage_issue(st, smem, st.n_units > 1 ? 1 : 0, unit_stride);
  const int n2 = st.n_units > 2 ? 2 : 0;
  st.pf_off = tab_entry(st, 2 * n2);
  st.pf_size = tab_entry(st, 2 * n2 + 1);
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
  asm volatile("" ::: "memory");
  __syncthreads();
}

// Kernel variant 7: the resident layers (nerfh_layout.h: kFineResident / kCoarseResident) are copied into LDS ONCE per workgroup, by the
// same DMA spread over the DMA waves, and read there by every tile.  Called right before stage_prime(), whose vmcnt(0) + barrier makes
// the copy visible together with the first two units.  `bytes` is a whole number of pieces (the blob is zero-padded).
// The ring needs no new argument: mid_sync() of streamed unit u still issues streamed unit u + 2 into the slot that held the previous
// STREAMED unit, which every wave has left once it is past u's barrier -- a resident layer between two streamed units is computed
// out of this region and touches no ring slot, and `st.u == 0` still names the tile's last streamed unit whether or not resident
// layers follow it, so the wrap to the next tile (units 0 and 1 issued from the last two streamed units' mid_sync) is unchanged.
// The lean unit's claimed tiles leave this as it is too: units 0 and 1 are the same bytes whichever tile comes next, so the wrap
// asks only WHETHER a tile follows (st.more), never which; st.more is set by the tile's first mid_sync (streamed unit 0 or 1 of 14 / 22)
// and read from the second-to-last streamed unit's on, st.u == 0 names the same unit, and a workgroup whose claim is past the last
// tile sees more == false exactly where the static deal's last tile did: nothing is issued into a ring nobody will read.
DFN_DEV void stage_resident(const Stager& st, char* smem, const char* res_blob, uint32_t bytes, uint32_t lds_off) {
  const char* src = res_blob + st.lane * 16;
  if (st.wave >= st.dma_waves) return;
  for (uint32_t p = st.wave * kPiece; p < bytes; p += st.dma_waves * kPiece) lds_dma_b128(src + p, smem + lds_off + p);
}

// Returns the LDS byte offset of unit st.u (already visible) and advances the rotation.
DFN_DEV uint32_t open_unit(Stager& st) {
  const uint32_t cur = st.slot * st.ustride;
  st.slot = st.slot + 1 == st.ring ? 0u : st.slot + 1;   // now: the slot of the unit after the one just opened (landing / landed)
  int nxt = st.u + 1;
  if (nxt == st.n_units) nxt = 0;
  st.u = nxt;
  return cur;
}

// Once per unit, between two of its MFMA chunks.  After open_unit(): st.u = the unit after the open one.
DFN_DEV void mid_sync(Stager& st, char* smem) {
#ifdef DFN_TIMING
  const unsigned long long c0 = __builtin_amdgcn_s_memtime();
#endif
  // this wave's share of the next unit has landed
  // (the builtin, not asm: LLVM's waitcnt pass then knows its own older loads — the per-ray bias — have landed and
  // does not re-wait for them later with a count that the untracked DMA loads would turn into a wait for the DMA)
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
  asm volatile("" ::: "memory");
#ifdef DFN_MLP_LEAN_TU
  // the tile's first mid_sync: the claim issued at the top of the tile has returned with the wait above.  Wave 0 puts the claimed tile
  // into the LDS word and sees it written (lgkmcnt(0)) BEFORE it signals this unit's barrier; no barrier is added.  The word is
  // rewritten one tile later, behind every barrier of this tile: every wave has read it by then (it reads right behind this barrier).
  if (st.claiming && st.wave == 0) {
    if (st.lane == 0) *claim_word(smem, st.claim_lds) = st.grid + st.claim;
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0)
    asm volatile("" ::: "memory");
  }
#endif
#ifdef DFN_TIMING
  const unsigned long long c1 = __builtin_amdgcn_s_memtime();
#endif
  // unit after next: open unit index is st.u - 1, so this is st.u + 1 (possibly in the next tile); it goes to the slot after
  // the next unit's, which held the unit BEFORE the open one: free once every wave is inside the open unit, i.e. after the barrier
  int n2 = st.u + 1;
  bool next_tile = st.u == 0;   // the open unit is the tile's last: both st.u and st.u + 1 belong to the next tile
  if (n2 >= st.n_units) { n2 -= st.n_units; next_tile = true; }
  const uint32_t dst = (st.slot + 1 == st.ring ? 0u : st.slot + 1) * st.ustride;
  __builtin_amdgcn_s_barrier();   // every share landed; every wave is inside the open unit
  asm volatile("" ::: "memory");
#ifdef DFN_TIMING
  const unsigned long long c2 = __builtin_amdgcn_s_memtime();
  st.t_wait += c1 - c0;
  st.t_sync += c2 - c1;
  if (st.trace && st.n_trace < 96 && st.lane == 0) {  // timeline of the first units: (enter, after barrier)
    st.trace[2 * st.n_trace] = c0;
    st.trace[2 * st.n_trace + 1] = c2;
  }
  ++st.n_trace;
#endif
#ifdef DFN_MLP_LEAN_TU
  if (st.claiming) {   // every wave, behind the barrier wave 0 wrote in front of
    st.next = __builtin_amdgcn_readfirstlane(*claim_word(smem, st.claim_lds));
    st.more = st.next < st.n_tiles;
    st.claiming = false;
  }
#endif
  if (!next_tile || st.more) stage_issue_at(st, smem, st.pf_off, st.pf_size, dst);
  {  // fetch the table entry needed by the next call now, so its scalar-load latency is off the critical path
    int n3 = n2 + 1;
    if (n3 >= st.n_units) n3 -= st.n_units;
    st.pf_off = tab_entry(st, 2 * n3);
    st.pf_size = tab_entry(st, 2 * n3 + 1);
  }
}

// ------------------------------------------------------------------------------------------
// One 32-row M-block: acc[nb] += W_mb * Bin[nb] over KC chunks.  `wb` = LDS byte offset of the
// block's first A fragment, already including lane * kLaneBytes.
template <class P>
DFN_DEV typename FragOf<P>::type load_afrag(const char* p);

template <class P, int NB, int KC>
DFN_DEV void mblock_mma(const char* smem, uint32_t wb, const typename FragOf<P>::type (&Bin)[NB][KC],
                        f32x16 (&acc)[NB]) {
  using F = typename FragOf<P>::type;
#pragma unroll
  for (int kc = 0; kc < KC; ++kc) {
    const F a = load_afrag<P>(smem + wb + kc * 64 * P::kLaneBytes);
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[nb] = mfma<P>(a, Bin[nb][kc], acc[nb]);
  }
}

template <class P>
DFN_DEV typename FragOf<P>::type load_afrag(const char* p) {
  if constexpr (P::kSplit) {
    half8x2 f;
    f.hi = *reinterpret_cast<const half8*>(p);
    f.lo = *reinterpret_cast<const half8*>(p + 1024);
    return f;
  } else {
    return *reinterpret_cast<const typename FragOf<P>::type*>(p);
  }
}

DFN_DEV f32x16 load16(const float* p) {
  const f32x4* q = reinterpret_cast<const f32x4*>(p);
  f32x4 a = q[0], b = q[1], c = q[2], d = q[3];
  f32x16 r;
#pragma unroll
  for (int i = 0; i < 4; ++i) { r[i] = a[i]; r[4 + i] = b[i]; r[8 + i] = c[i]; r[12 + i] = d[i]; }
  return r;
}
// PrecX3M16 bias fragment of an M-block: the unit's 128-byte bias block is [g][ms][r] (Packer::pack_blocks), p = its lane group's 8
// floats; registers 4 ms + r (ms = 0, 1) are the seed of both N-blocks' fragments q = 2 ms + nb.
DFN_DEV f32x16 load_bias_m16(const float* p) {
  const f32x4* q = reinterpret_cast<const f32x4*>(p);
  const f32x4 a = q[0], b = q[1];
  f32x16 r = {};
#pragma unroll
  for (int i = 0; i < 4; ++i) { r[i] = a[i]; r[4 + i] = b[i]; }
  return r;
}
// PrecX3M16 per-ray seeds of M-block mb: the ray-bias table keeps the 32x32 order [mb][h][r] (ray_bias_kernel), in which row
// 16 ms + 4 g + r sits at h = g & 1, r' = r + 4 (2 ms + (g >> 1)); fragment q = 2 ms + nb takes the row of N-block nb's own ray.
DFN_DEV f32x16 load_raybias_m16(const float* const (&rb)[2], int mb, int g) {
  f32x16 r;
#pragma unroll
  for (int nb = 0; nb < 2; ++nb) {
    const f32x4* q = reinterpret_cast<const f32x4*>(rb[nb] + mb * 32 + (g & 1) * 16 + 4 * (g >> 1));
    const f32x4 a = q[0], b = q[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) { r[4 * nb + i] = a[i]; r[8 + 4 * nb + i] = b[i]; }
  }
  return r;
}
DFN_DEV f32x4 sub4(const f32x16& v, int o) { return f32x4{v[o], v[o + 1], v[o + 2], v[o + 3]}; }
DFN_DEV void put4(f32x16& v, int o, const f32x4& x) { v[o] = x[0]; v[o + 1] = x[1]; v[o + 2] = x[2]; v[o + 3] = x[3]; }

// C fragment -> B-operand registers of the next layer (ReLU optional).
template <class P, bool RELU, int OC>
DFN_DEV void store_hidden(const f32x16& acc, typename FragOf<P>::type (&out)[OC], int mb, float oscale, uint32_t& rmax) {
  if constexpr (P::kSplit) {
    // two values per conversion (v_cvt_pkrtz_f16_f32): hi is the TRUNCATED f16 of the scaled value — any f16 within an ulp will do,
    // the lo half takes the exact remainder — so a pair costs 2 packed converts + 2 mixed-precision subtractions
    typedef __fp16 pk2 __attribute__((ext_vector_type(2)));
    const float os = oscale * kX3ActScale;
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int j = 0; j < 8; j += 2) {
        float x0 = acc[8 * c + j] * os, x1 = acc[8 * c + j + 1] * os;      // true values x the operand scale (one power-of-two product)
        if (RELU) { x0 = fmaxf(x0, 0.f); x1 = fmaxf(x1, 0.f); }
        const pk2 h = __builtin_amdgcn_cvt_pkrtz(x0, x1);
        // remainders x - hi in fp32 with the f16 halves read in place (v_fma_mix_f32; hipcc converts and subtracts otherwise)
        const uint32_t hb = __builtin_bit_cast(uint32_t, h);
        float r0, r1;
        asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(r0) : "v"(hb), "v"(x0));
        asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r1) : "v"(hb), "v"(x1));
        const pk2 l = __builtin_amdgcn_cvt_pkrtz(r0, r1);
        range_track(rmax, hb, RELU);
        const int oc = 2 * mb + x3_chunk<P>(4 * c + j / 2), oj = x3_pos<P>(4 * c + j / 2);
        out[oc].hi[oj] = (_Float16)h[0]; out[oc].hi[oj + 1] = (_Float16)h[1];
        out[oc].lo[oj] = (_Float16)l[0]; out[oc].lo[oj + 1] = (_Float16)l[1];
      }
  } else if constexpr (P::kSlotsPerChunk == 8) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      half8 v;
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (_Float16)acc[8 * c + j];
      if (RELU) {
        const half8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
        v = __builtin_elementwise_max(v, zero);
      }
      {   // range guard: one packed maximum over the four registers, then one update of the running maximum
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        u32x4 w = __builtin_bit_cast(u32x4, v);
        if (!RELU) w &= 0x7fff7fffu;
        rmax = pk_max_u16(rmax, pk_max_u16(pk_max_u16(w[0], w[1]), pk_max_u16(w[2], w[3])));
      }
      out[2 * mb + c] = v;
    }
  } else {
#pragma unroll
    for (int r = 0; r < 16; ++r) out[16 * mb + r] = RELU ? fmaxf(acc[r], 0.f) : acc[r];
  }
}

template <class P, bool RELU, int OC>
DFN_DEV void store_hidden(const f32x16& acc, typename FragOf<P>::type (&out)[OC], int mb, float oscale = 1.f) {
  uint32_t unused = 0;
  store_hidden<P, RELU>(acc, out, mb, oscale, unused);
}

// One eighth of store_hidden: output register pair i (0..7) of an M-block's C fragment.  The two empty
// asm statements anchor the conversion at this point of the instruction stream: without them LLVM treats the
// pure arithmetic as freely movable and sinks it out from between the MFMAs it is meant to hide behind.
template <class P, bool RELU, int OC>
DFN_DEV void store_hidden_piece(const f32x16& acc, typename FragOf<P>::type (&out)[OC], int mb, int i, float oscale, uint32_t& rmax) {
  if constexpr (P::kSplit) {
    // split-f16: piece i = two consecutive results -> one register of the hi plane + one of the lo plane (the arithmetic of
    // store_hidden: scale, ReLU, truncating hi pair, exact remainders by v_fma_mix_f32, lo pair), as ONE volatile asm block so
    // that its eight VALU instructions stay between the MFMAs they hide behind.  `oscale` already holds out_scale x kX3ActScale.
    typedef _Float16 half2v __attribute__((ext_vector_type(2)));
    const int c = i >> 2, j = (i & 3) * 2;
    uint32_t hb, lb;
    float t0, t1;
    if (RELU)
      asm volatile("v_mul_f32 %2, %4, %6\n\tv_mul_f32 %3, %5, %6\n\tv_max_f32 %2, %2, 0\n\tv_max_f32 %3, %3, 0\n\t"
                   "v_cvt_pkrtz_f16_f32 %0, %2, %3\n\t"
                   "v_fma_mix_f32 %2, %0, -1.0, %2 op_sel_hi:[1,0,0]\n\t"
                   "v_fma_mix_f32 %3, %0, -1.0, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"
                   "v_cvt_pkrtz_f16_f32 %1, %2, %3"
                   : "=&v"(hb), "=&v"(lb), "=&v"(t0), "=&v"(t1) : "v"(acc[8 * c + j]), "v"(acc[8 * c + j + 1]), "v"(oscale));
    else
      asm volatile("v_mul_f32 %2, %4, %6\n\tv_mul_f32 %3, %5, %6\n\t"
                   "v_cvt_pkrtz_f16_f32 %0, %2, %3\n\t"
                   "v_fma_mix_f32 %2, %0, -1.0, %2 op_sel_hi:[1,0,0]\n\t"
                   "v_fma_mix_f32 %3, %0, -1.0, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"
                   "v_cvt_pkrtz_f16_f32 %1, %2, %3"
                   : "=&v"(hb), "=&v"(lb), "=&v"(t0), "=&v"(t1) : "v"(acc[8 * c + j]), "v"(acc[8 * c + j + 1]), "v"(oscale));
    if (RELU) asm volatile("v_pk_max_u16 %0, %0, %1" : "+v"(rmax) : "v"(hb));   // range guard (range_track), pinned with the piece
    else range_track(rmax, hb, false);
    const half2v hv = __builtin_bit_cast(half2v, hb), lv = __builtin_bit_cast(half2v, lb);
    const int oc = 2 * mb + x3_chunk<P>(i), oj = x3_pos<P>(i);
    out[oc].hi[oj] = hv[0]; out[oc].hi[oj + 1] = hv[1];
    out[oc].lo[oj] = lv[0]; out[oc].lo[oj + 1] = lv[1];
  } else if constexpr (P::kSlotsPerChunk == 8) {
    typedef _Float16 half2v __attribute__((ext_vector_type(2)));
    const int c = i >> 2, j = i & 3;
    // volatile asm = fixed position in the instruction stream (between the MFMAs it hides behind), plain
    // register reads of the finished accumulators, no copies.  The accumulators read here were written by
    // MFMAs at least three MFMA issues earlier, which covers the XDL-write -> VALU-read wait states.
    uint32_t bits;
    if (RELU)
      asm volatile("v_cvt_pk_f16_f32 %0, %1, %2\n\tv_pk_max_f16 %0, %0, 0" : "=v"(bits) : "v"(acc[8 * c + 2 * j]), "v"(acc[8 * c + 2 * j + 1]));
    else
      asm volatile("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(bits) : "v"(acc[8 * c + 2 * j]), "v"(acc[8 * c + 2 * j + 1]));
    if (RELU) asm volatile("v_pk_max_u16 %0, %0, %1" : "+v"(rmax) : "v"(bits));   // range guard (range_track), pinned with the piece
    else range_track(rmax, bits, false);
    const half2v v = __builtin_bit_cast(half2v, bits);
    out[2 * mb + c][2 * j] = v[0];
    out[2 * mb + c][2 * j + 1] = v[1];
  } else {
    float x0 = acc[2 * i], x1 = acc[2 * i + 1];
    asm volatile("" : "+v"(x0), "+v"(x1));
    x0 = RELU ? fmaxf(x0, 0.f) : x0;
    x1 = RELU ? fmaxf(x1, 0.f) : x1;
    asm volatile("" : "+v"(x0), "+v"(x1));
    out[16 * mb + 2 * i] = x0;
    out[16 * mb + 2 * i + 1] = x1;
  }
}

// The split-f16 conversion piece in three parts, so that a K-chunk can place them BETWEEN its three dependent MFMAs (A after the
// first, B after the second, C after the third) instead of as one block behind them: the parts of store_hidden_piece<PrecX3>.
#ifdef DFN_MLP_LEAN_TU
#define DFN_X3_HOLD , rhold   // layer(): the even piece's hi pair, handed to the odd piece's part C
#else
#define DFN_X3_HOLD
#endif
struct X3Piece {
  uint32_t hb, hs, lb;
  float t0, t1;
  // A: ReLU on the UNSCALED accumulators (they carry in_scale x the value: the packer keeps in_scale x |activation| inside f16).
  template <bool RELU>
  DFN_DEV void A(const f32x16& acc, int i) {
    const int c = i >> 2, j = (i & 3) * 2;
    if (RELU) asm volatile("v_max_f32 %0, %2, 0\n\tv_max_f32 %1, %3, 0" : "=&v"(t0), "=&v"(t1) : "v"(acc[8 * c + j]), "v"(acc[8 * c + j + 1]));
    else asm volatile("v_mov_b32 %0, %2\n\tv_mov_b32 %1, %3" : "=&v"(t0), "=&v"(t1) : "v"(acc[8 * c + j]), "v"(acc[8 * c + j + 1]));
  }
  // B: truncated hi pair of the unscaled values, scaled as a PACKED f16 product (a power of two: exact), then the two remainders
  // t x s - hi' in one mixed-precision FMA each — the accumulator -> operand scale costs one instruction per PAIR instead of two.
  DFN_DEV void B(float s, uint32_t s2) {
    asm volatile("v_cvt_pkrtz_f16_f32 %0, %2, %3\n\t"
                 "v_pk_mul_f16 %1, %0, %5\n\t"
                 "v_fma_mix_f32 %2, %2, %4, -%1 op_sel_hi:[0,0,1]\n\t"
                 "v_fma_mix_f32 %3, %3, %4, -%1 op_sel:[0,0,1] op_sel_hi:[0,0,1]"
                 : "=&v"(hb), "=&v"(hs), "+v"(t0), "+v"(t1) : "v"(s), "v"(s2));
  }
  // B in two halves (the 16x16x32 chunk spreads the parts over more, shorter MFMA gaps): B1 = hi pair and its scaled copy, B2 = remainders
  DFN_DEV void B1(uint32_t s2) {
    asm volatile("v_cvt_pkrtz_f16_f32 %0, %2, %3\n\t"
                 "v_pk_mul_f16 %1, %0, %4"
                 : "=&v"(hb), "=&v"(hs) : "v"(t0), "v"(t1), "v"(s2));
  }
  DFN_DEV void B2(float s) {
    asm volatile("v_fma_mix_f32 %0, %0, %2, -%3 op_sel_hi:[0,0,1]\n\t"
                 "v_fma_mix_f32 %1, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]"
                 : "+v"(t0), "+v"(t1) : "v"(s), "v"(hs));
  }
#ifdef DFN_MLP_LEAN_TU
  // The lean unit: the guard of a ReLU conversion at one instruction per TWO pieces.  An even piece leaves its unscaled hi pair in
  // `hold` (a register kept until the odd piece's part C, no instruction); the odd piece takes rmax = maximum3(rmax, hold, hb) as packed
  // f16 (v_pk_maximum3_f16).  Why range_report() raises the flag in exactly the launches in which it does after two v_pk_max_u16:
  //   * Both halves of hb come from v_cvt_pkrtz_f16_f32 of t = v_max_f32(acc, 0).  For a finite or +inf t they are non-negative f16
  //     patterns 0x0000 .. 0x7c00, on which the float order IS the order of the 16-bit patterns, so the two instructions keep the same
  //     maximum; rmax itself starts as +0 and is such a pattern until something else enters it.
  //   * A NaN accumulator: v_max_f32(NaN, 0) in the kernels' IEEE mode is 0 for a quiet NaN (hb = 0 under both guards: neither raises,
  //     as today) and a quiet NaN for a signalling one.  That NaN converts to an f16 NaN, a pattern above 0x7c00 in the low 15 bits:
  //     v_pk_max_u16 keeps it as the largest unsigned pattern, v_pk_maximum3_f16 returns NaN whenever an operand is NaN, and a NaN in
  //     rmax stays one through every later maximum3 and is the largest pattern for every later v_pk_max_u16 (the guards of the layers
  //     without ReLU, which keep their masked form).  With or without its sign bit the 16-bit pattern is >= 0x7c00 > both thresholds:
  //     the flag is raised under both.
  //   * -0 (0x8000): as an unsigned pattern it is above the thresholds, as a float it is below +0, so the two guards would differ on it.
  //     It cannot occur: v_max_f32(x, 0) returns +0 for x = -0 and for every negative x, and the truncating conversion of a non-negative
  //     value is non-negative.  (Were it to occur, today's guard would raise on an in-range value.)
  //   * The f16 denormal mode: were v_pk_maximum3_f16 to flush a denormal operand, it would return +0 or the denormal, both below 2^-14;
  //     no value moves across 0x7bff / 0x7c00, the only patterns range_report() compares with.
  template <bool RELU, class P = PrecX3, int OC>
  DFN_DEV void C(half8x2 (&out)[OC], int mb, int i, uint32_t& rmax, uint32_t& hold) {
    typedef _Float16 half2v __attribute__((ext_vector_type(2)));
    const int c = x3_chunk<P>(i), j = x3_pos<P>(i);
    asm volatile("v_cvt_pkrtz_f16_f32 %0, %1, %2" : "=v"(lb) : "v"(t0), "v"(t1));
    // range guard on the UNSCALED hi pair: that conversion is the one that saturates
    if (RELU) {
      if ((i & 1) == 0) hold = hb;
      else asm volatile("v_pk_maximum3_f16 %0, %0, %1, %2" : "+v"(rmax) : "v"(hold), "v"(hb));
    } else range_track(rmax, hb, false);
#else
  template <bool RELU, class P = PrecX3, int OC>
  DFN_DEV void C(half8x2 (&out)[OC], int mb, int i, uint32_t& rmax) {
    typedef _Float16 half2v __attribute__((ext_vector_type(2)));
    const int c = x3_chunk<P>(i), j = x3_pos<P>(i);
    asm volatile("v_cvt_pkrtz_f16_f32 %0, %1, %2" : "=v"(lb) : "v"(t0), "v"(t1));
    // range guard on the UNSCALED hi pair: that conversion is the one that saturates
    if (RELU) asm volatile("v_pk_max_u16 %0, %0, %1" : "+v"(rmax) : "v"(hb));
    else range_track(rmax, hb, false);
#endif
    const half2v hv = __builtin_bit_cast(half2v, hs), lv = __builtin_bit_cast(half2v, lb);
    out[2 * mb + c].hi[j] = hv[0]; out[2 * mb + c].hi[j + 1] = hv[1];
    out[2 * mb + c].lo[j] = lv[0]; out[2 * mb + c].lo[j + 1] = lv[1];
  }
};

// A layer whose MB output M-blocks feed the next layer, plus (EXTRA) one trailing head M-block
// whose raw accumulators go back to the caller.  Weights arrive in staging units of UMB M-blocks;
// NEWUNIT = false continues inside the unit opened by the previous layer (small layers are packed
// several to a unit: no barrier, no DMA wait between them).
//
// Software pipeline: inside a staging unit the A fragments form one flat stream t = (m-block, chunk);
// fragment t+PF is fetched from LDS before the MFMAs of fragment t issue, so the ~100+-cycle LDS
// latency hides under PF*NB MFMAs instead of stalling every chunk.  The bias is the C operand of
// each accumulator's FIRST MFMA (no register copies) and is fetched one M-block ahead; RAYBIAS
// layers seed their accumulators from the per-ray table.
//
// PIPE: the f32 -> f16 (+ReLU) conversion of M-block m-1 is issued piecewise between the MFMAs of
// M-block m.  CIN >= 0: the previous layer left its LAST M-block unconverted in `carry`; it lands in
// chunks CIN, CIN+1 of Bin and is converted during this layer's chunks 0..CIN-1 (before they are read).
// COUT: leave this layer's last M-block in `carry` for the next layer instead of converting it here.
// NOBIAS: the unit's bias fragments are all zero (backward layers): no bias reads, the first MFMA starts from a zero C operand.
// SCALE_FIRST (split-f16, PIPE): the pipelined conversion in its scale-in-fp32-first form (store_hidden_piece, a block of pieces behind
// each chunk's MFMAs) instead of the three-part X3Piece form, which converts the UNSCALED accumulators and so needs the render
// kernels' unit weight scale — the gradient kernels keep the 2^10 scale and per-point renormalisation factors (Stager::lane_mul).
// TRACK = false: the range guard does not watch this layer's conversions (the caller checks the finished operand itself: the gradient
// kernel's renormalisation already takes the maximum |hi| of it, renorm_factor).
// HALF (PrecX3M16, a layer that is ONE head M-block: kernel variant 6): the block's head values c = 0..3 sit on its 16-row half
// ms = 0 (head_row_m16) and nothing of half 1 is read, so the unit holds and the loop runs the KC / 2 fragments with ms = 0 only (live
// chunk kl = the 32-K chunk k32 = kl); head[] values c >= 4 come back as zeros.  The carried-in M-block is then converted inside
// KC / 2 - 1 live chunks: see the hazard counts at the chunk body.
// RES >= 0 (kernel variant 7): the layer's units sit back to back at LDS byte offset RES for the whole kernel (stage_resident), in the
// unit format but without the rounding to pieces.  It is the NEWUNIT = false form with a compile-time base: no open_unit(), no
// mid_sync(), the Stager is not touched; the fragment prefetch, bias reads, carry-in and conversion pieces are the streamed form's.
template <class P, int UMB, bool PIPE, int NB, int KC, int MB, bool RELU, bool EXTRA, bool RAYBIAS, bool NEWUNIT,
          int CIN, bool CIN_RELU, bool COUT, bool NOBIAS = false, bool SCALE_FIRST = false, bool TRACK = true, bool HALF = false, int RES = -1>
DFN_DEV void layer(Stager& st, char* smem, typename FragOf<P>::type (&Bin)[NB][KC],
                   typename FragOf<P>::type (&Bout)[NB][(MB ? MB : 1) * chunks_of<P>(16)],
                   f32x16 (&head)[NB], const float* const (&raybias)[lane_pts<P>(NB)], f32x16 (&carry)[NB]) {
  using F = typename FragOf<P>::type;
  static_assert(!P::kM16 || (PIPE && NB == 1 && !SCALE_FIRST), "the 16x16x32 split-f16 layer is the pipelined one-point-block form");
  constexpr int TOT = MB + (EXTRA ? 1 : 0);
  constexpr int PF = P::kSplit ? 2 : (P::kSlotsPerChunk == 8 ? DFN_PF : 4);  // fragments in flight
  constexpr uint32_t FB = 64 * P::kLaneBytes;         // bytes of one A fragment
  constexpr int PPK = (8 * NB + KC - 1) / KC;         // conversion pieces (8 per point block) interleaved per chunk
  constexpr int PPKI = CIN > 0 ? (8 * NB + CIN - 1) / CIN : 0;  // same for the carried-in M-block
  static_assert(CIN < 0 || (PIPE && P::kSlotsPerChunk == 8 && CIN > 0 && CIN + 1 < KC + 1), "carry-in needs the pipelined f16 path");
  static_assert(!COUT || (PIPE && MB >= 1 && !EXTRA), "carry-out needs a regular last M-block");
  static_assert(NEWUNIT || UMB >= TOT || RES >= 0, "a layer that continues a unit must fit in it");
  static_assert(RES < 0 || (!NEWUNIT && P::kM16), "a resident layer opens no staging unit");
  static_assert(!HALF || (P::kM16 && EXTRA && MB == 0 && !RAYBIAS && KC % 2 == 0 && CIN >= 2 && CIN % 2 == 0 && CIN + 2 == KC),
                "a half-height block is a PrecX3M16 head layer whose last 32-K chunk is the carried-in M-block");
  constexpr int KCL = HALF ? KC / 2 : KC;      // fragments (chunks of the loop) per M-block
  constexpr int CINL = HALF ? CIN / 2 : CIN;   // chunks that precede the first reader of the carried-in M-block
  constexpr bool TAILBLK = HALF && CINL == 1;  // K = 64 half-height heads: one live chunk precedes the reader (see the chunk body)
  const int h = st.lane >> 5, g16 = st.lane >> 4;   // g16: lane group of the 16x16 fragments (PrecX3M16)
  uint32_t rmax_sink = 0;
  uint32_t& rmax_ = TRACK ? st.rmax : rmax_sink;
#ifdef DFN_MLP_LEAN_TU
  uint32_t rhold = 0;   // every M-block's eight pieces are converted in order inside one call: nothing is held across calls
#endif
  const float pscale = P::kSplit ? st.out_scale * st.lane_mul * kX3ActScale : 1.f;  // split-f16 pieces: accumulator -> operand scale
  uint32_t pscale2 = 0;   // ... the same factor as a packed f16 pair (X3Piece::B)
  if constexpr (P::kSplit) asm("v_cvt_pkrtz_f16_f32 %0, %1, %1" : "=v"(pscale2) : "v"(pscale));
  constexpr bool RB_ALL = RAYBIAS && NB <= 2;  // fetch all per-ray seeds at entry (latency behind the barrier)
  f32x16 rb[RB_ALL ? TOT : 1][NB];
  if (RB_ALL) {
#pragma unroll
    for (int mb = 0; mb < TOT; ++mb)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        if constexpr (P::kM16) rb[mb][nb] = load_raybias_m16(raybias, mb, g16);
        else rb[mb][nb] = load16(raybias[nb] + (mb * 2 + h) * 16);
#ifndef DFN_MLP_LEAN_TU   // the lean unit: the table holds in_scale x the seeds (ray_bias_kernel<true>)
        if constexpr (P::kSplit) rb[mb][nb] *= st.in_scale;   // accumulators carry in_scale x the true value
#endif
      }
  }
  f32x16 pend[PIPE ? NB : 1];  // accumulators of M-block mb-1 while M-block mb runs
#pragma unroll
  for (int u0 = 0; u0 < TOT; u0 += UMB) {
    const int nmb = (TOT - u0) < UMB ? (TOT - u0) : UMB;  // M-blocks in this unit (compile-time after unrolling)
    const int nt = nmb * KCL;
    uint32_t ub;
    if (NEWUNIT) { ub = open_unit(st); st.ubase = ub; st.uoff = 0; }
    else if constexpr (RES >= 0) ub = uint32_t(RES) + u0 * (KCL * FB + 128);   // full units of UMB M-blocks precede unit u0 / UMB
    else ub = st.ubase + st.uoff;
    if constexpr (RES < 0) st.uoff += nmb * KCL * FB + nmb * 128;
    // split-f16 fragment = a hi plane (64 lanes x 16 B) followed by a lo plane: both reads stay lane-linear 16-byte
    const char* wl = smem + ub + st.lane * (P::kSplit ? 16 : P::kLaneBytes);
    const char* bl = smem + ub + nmb * KCL * FB + (P::kM16 ? g16 * 32 : h * 64);
    F a[PF];
#define DFN_AFRAG(t) load_afrag<P>(wl + (t) * FB)
#pragma unroll
    for (int t = 0; t < PF; ++t)
      if (t < nt) a[t] = DFN_AFRAG(t);
    f32x16 bias = {};
    auto load_bias = [&](const char* p) {
      if constexpr (P::kM16) return load_bias_m16(reinterpret_cast<const float*>(p));
      else return load16(reinterpret_cast<const float*>(p));
    };
    if (!RAYBIAS && !NOBIAS) bias = load_bias(bl);
#pragma unroll
    for (int lm = 0; lm < UMB; ++lm) {
      if (lm < nmb) {
        const int mb = u0 + lm;
        f32x16 acc[NB];
        if constexpr (HALF) {   // registers 8..15 (half 1) are never written
#pragma unroll
          for (int nb = 0; nb < NB; ++nb) acc[nb] = f32x16{};
        }
        f32x16 bias_next = bias;
        if (RAYBIAS) {
#pragma unroll
          for (int nb = 0; nb < NB; ++nb) {
            if constexpr (P::kM16) acc[nb] = RB_ALL ? rb[RB_ALL ? mb : 0][nb] : load_raybias_m16(raybias, mb, g16);
            else acc[nb] = RB_ALL ? rb[RB_ALL ? mb : 0][nb] : load16(raybias[nb] + (mb * 2 + h) * 16);
#ifndef DFN_MLP_LEAN_TU
            if constexpr (P::kSplit && !RB_ALL) acc[nb] *= st.in_scale;
#endif
          }
        }
#pragma unroll
        for (int kc = 0; kc < KCL; ++kc) {
          const int t = lm * KCL + kc;
          if (NEWUNIT && lm == 0 && kc == (KCL > 1 ? KCL / 2 : 0)) mid_sync(st, smem);
          const F cur = a[t % PF];
          if (t + PF < nt) a[t % PF] = DFN_AFRAG(t + PF);
          if (kc == (PIPE ? KCL / 2 : 0) && !RAYBIAS && !NOBIAS && lm + 1 < nmb) bias_next = load_bias(bl + (lm + 1) * 128);
          __builtin_amdgcn_sched_barrier(0);  // keep the prefetch ABOVE this chunk's MFMAs (hipcc otherwise sinks it to its use)
          if constexpr (P::kSplit && PIPE && NB == 1 && !SCALE_FIRST) {
            // split-f16: the conversion pieces of this chunk go BETWEEN its three dependent MFMAs, a third each (the block form
            // behind them measured 46.5 against 42.7 cycles per MFMA in tools/ubench/x3loop.hip)
            constexpr int PPKI_ = TAILBLK ? 4 : ((CIN > 0) ? (8 * NB + CINL - 1) / CINL : 1), PPK_ = (8 * NB + KCL - 1) / KCL;
            constexpr int NPMAX = PPKI_ > PPK_ ? PPKI_ : PPK_;
            static_assert(!HALF || NPMAX <= 4, "half 1's pieces must not start in the first chunk");
            const bool from_carry = CIN > 0 && mb == 0 && kc < CINL, from_pend = mb >= 1;
            const int np = from_carry ? PPKI_ : (from_pend ? PPK_ : 0), base = kc * np;
            X3Piece pc[NPMAX];
            // kc == 0: the accumulators the pieces read (pend / carry) were written by the MFMA issued just before this chunk; an
            // XDL result is not interlocked against VALU reads from inline asm, so the first chunk keeps the block form -- all three
            // parts behind its third MFMA, >= 3 MFMA issues after the producer (read one issue later, the last correction product
            // of some results was missing: 1e-6 instead of 2.4e-7 against exact fp32).
            const bool late = kc == 0;
#define DFN_X3_PARTS_A \
            _Pragma("unroll") for (int q = 0; q < NPMAX; ++q) \
              if (q < np && base + q < 8) { \
                if (from_carry) pc[q].template A<CIN_RELU>(carry[0], base + q); \
                else pc[q].template A<RELU>(pend[0], base + q); \
              }
#define DFN_X3_PARTS_B \
            _Pragma("unroll") for (int q = 0; q < NPMAX; ++q) \
              if (q < np && base + q < 8) pc[q].B(pscale, pscale2);
            if constexpr (P::kM16) {
              // 16x16x32: chunk kc = the 32-K chunk kc >> 1 of the M-block's 16-row half ms = kc & 1.  Its A fragment feeds both N-blocks
              // (B chunks 2 (kc >> 1) + nb), three products each: two independent accumulation chains, fragments q = 2 ms + nb.  The
              // conversion parts go into the gaps after MFMAs 2..5 (A, B1, B2, C: 8 VALU cycles per 16-cycle MFMA are free).
              // Hazard (8-pass XDL result -> VALU read in inline asm: 12 wait states, no interlock): piece i reads fragment q = i >> 1 of
              // half ms = i >> 2, last written in chunk KC - 2 + ms of the previous M-block (layer), and half 1's pieces start at chunk
              // 8 / (2 np) >= 1 (np <= 4 pieces per chunk): >= 8 MFMA issues lie between producer and reader in every chunk, the first
              // one included (the 32x32 path's `late` rule holds by construction).
              // HALF: live chunk kl = (k32 = kl, ms = 0); the producer of the carried-in M-block is unchanged (half ms last written in
              // chunk KC - 2 + ms of the layer before), only the readers move.
              //   K = 128 (static_sigma: 4 live chunks, the carried-in chunk is read by the 4th): 8 pieces over live chunks 0..2 = 3 per
              //   chunk (np = 3 <= 4).  Pieces 0..2 (half 0) in live chunk 0: part A sits behind 6 (producer layer's last chunk) + 2
              //   = 8 MFMA issues after half 0's last write.  Half 1's first pieces 4, 5 are in live chunk 1 = 4 / 3: part A behind
              //   6 (live chunk 0) + 2 = 8 MFMA issues after the producer layer's last MFMA.  The count of the full-height form holds.
              //   K = 64 (static_rgb, transient head: 2 live chunks, the 2nd reads the carried-in chunk; TAILBLK): pieces 0..3 (half 0) go
              //   into live chunk 0's gaps exactly as in the full-height form (8 issues).  No gap with 8 MFMA issues behind half 1's
              //   producer exists before the reader, so pieces 4..7 are converted in the BLOCK form behind live chunk 0's last MFMA,
              //   with explicit wait states: 6 MFMA issues + s_nop 7 (8 states) = 14 >= the 12 wait states an 8-pass XDL result needs
              //   before a VALU read, counting each MFMA issue as ONE state (an issue behind an 8-pass MFMA takes >= 8 passes, and the
              //   36 VALU instructions of pieces 0..3 lie in between as well).  The same parts in the same arithmetic: same bits.
              //   These are counts in SOURCE order.  hipcc keeps the asm pieces in order among themselves but may place a chunk's
              //   first two MFMAs behind its part A (it does for bias-seeded chunks, in the full-height kernels too), which takes 2 off
              //   a count; in the generated code of the three half-height kernels the shortest distance from an accumulator's last
              //   write to the piece that reads it is 6 MFMA issues, the full-height folded kernel's own minimum (LABBOOK R12.1).
              const int ms = HALF ? 0 : (kc & 1), bc = HALF ? 2 * kc : 2 * (kc >> 1);
              f32x4 c0, c1;
              if (kc < (HALF ? 1 : 2) && !RAYBIAS) { c0 = sub4(bias, 4 * ms); c1 = c0; }
              else { c0 = sub4(acc[0], 8 * ms); c1 = sub4(acc[0], 8 * ms + 4); }
#define DFN_X3_PARTS(...) \
              _Pragma("unroll") for (int q = 0; q < NPMAX; ++q) \
                if (q < np && base + q < 8) { __VA_ARGS__; }
              c0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(cur.hi, Bin[0][bc].hi, c0, 0, 0, 0);
              c1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(cur.hi, Bin[0][bc + 1].hi, c1, 0, 0, 0);
              __builtin_amdgcn_sched_barrier(0);
              DFN_X3_PARTS_A
              __builtin_amdgcn_sched_barrier(0);
              c0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(cur.hi, Bin[0][bc].lo, c0, 0, 0, 0);
              __builtin_amdgcn_sched_barrier(0);
              DFN_X3_PARTS(pc[q].B1(pscale2))
              __builtin_amdgcn_sched_barrier(0);
              c1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(cur.hi, Bin[0][bc + 1].lo, c1, 0, 0, 0);
              __builtin_amdgcn_sched_barrier(0);
              DFN_X3_PARTS(pc[q].B2(pscale))
              __builtin_amdgcn_sched_barrier(0);
              c0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(cur.lo, Bin[0][bc].hi, c0, 0, 0, 0);
              __builtin_amdgcn_sched_barrier(0);
              DFN_X3_PARTS(if (from_carry) pc[q].template C<CIN_RELU, P>(Bin[0], CIN / 2, base + q, rmax_ DFN_X3_HOLD);
                           else pc[q].template C<RELU, P>(Bout[0], mb - 1, base + q, rmax_ DFN_X3_HOLD))
              __builtin_amdgcn_sched_barrier(0);
              c1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(cur.lo, Bin[0][bc + 1].hi, c1, 0, 0, 0);
#undef DFN_X3_PARTS
              put4(acc[0], 8 * ms, c0);
              put4(acc[0], 8 * ms + 4, c1);
              if constexpr (TAILBLK) {
                if (from_carry) {   // pieces 4..7 (half 1 of the carried-in M-block) in the block form: the counts above
                  __builtin_amdgcn_sched_barrier(0);
                  asm volatile("s_nop 7");
                  X3Piece tp[4];
#pragma unroll
                  for (int q = 0; q < 4; ++q) tp[q].template A<CIN_RELU>(carry[0], 4 + q);
#pragma unroll
                  for (int q = 0; q < 4; ++q) tp[q].B1(pscale2);
#pragma unroll
                  for (int q = 0; q < 4; ++q) tp[q].B2(pscale);
#pragma unroll
                  for (int q = 0; q < 4; ++q) tp[q].template C<CIN_RELU, P>(Bin[0], CIN / 2, 4 + q, rmax_ DFN_X3_HOLD);
                }
              }
              if (from_carry && kc == CINL - 1) asm volatile("s_nop 3");
              __builtin_amdgcn_sched_barrier(0);
              continue;
            }
            f32x16 c0 = (kc == 0) ? (RAYBIAS ? acc[0] : bias) : acc[0];
            c0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur.hi, Bin[0][kc].hi, c0, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if (!late) { DFN_X3_PARTS_A }
            __builtin_amdgcn_sched_barrier(0);
            c0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur.hi, Bin[0][kc].lo, c0, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if (!late) { DFN_X3_PARTS_B }
            __builtin_amdgcn_sched_barrier(0);
            c0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur.lo, Bin[0][kc].hi, c0, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if (late) { DFN_X3_PARTS_A DFN_X3_PARTS_B }
#undef DFN_X3_PARTS_A
#undef DFN_X3_PARTS_B
#pragma unroll
            for (int q = 0; q < NPMAX; ++q)
              if (q < np && base + q < 8) {
                if (from_carry) pc[q].template C<CIN_RELU>(Bin[0], CIN / 2, base + q, rmax_ DFN_X3_HOLD);
                else pc[q].template C<RELU>(Bout[0], mb - 1, base + q, rmax_ DFN_X3_HOLD);
              }
            acc[0] = c0;
            if (from_carry && kc == CIN - 1) asm volatile("s_nop 3");
            __builtin_amdgcn_sched_barrier(0);
            continue;
          }
          if constexpr (!P::kM16) {
#pragma unroll
          for (int nb = 0; nb < NB; ++nb) {
            if (kc == 0) acc[nb] = mfma<P>(cur, Bin[nb][0], RAYBIAS ? acc[nb] : bias);
            else acc[nb] = mfma<P>(cur, Bin[nb][kc], acc[nb]);
          }
          }
          if (CIN > 0 && mb == 0 && kc < CIN) {  // the previous layer's last M-block -> chunks CIN, CIN+1 of Bin
#pragma unroll
            for (int q = 0; q < PPKI; ++q) {
              const int piece = kc * PPKI + q;
              if (piece < 8 * NB) store_hidden_piece<P, CIN_RELU>(carry[piece >> 3], Bin[piece >> 3], CIN / 2, piece & 7, pscale, rmax_);
            }
            if (kc == CIN - 1) asm volatile("s_nop 3");  // VALU-written B operand is read by the very next MFMA
          }
          if (PIPE && mb >= 1) {  // previous M-block's conversion, block by block (frees pend[0] first)
#pragma unroll
            for (int q = 0; q < PPK; ++q) {
              const int piece = kc * PPK + q;
              if (piece < 8 * NB) store_hidden_piece<P, RELU>(pend[piece >> 3], Bout[piece >> 3], mb - 1, piece & 7, pscale, rmax_);
            }
          }
          __builtin_amdgcn_sched_barrier(0);
        }
        bias = bias_next;
        if (mb < MB) {
          if (PIPE) {
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) pend[nb] = acc[nb];
          } else {
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) store_hidden<P, RELU>(acc[nb], Bout[nb], mb, st.out_scale * st.lane_mul, rmax_);
          }
        } else {
#pragma unroll
          for (int nb = 0; nb < NB; ++nb) {  // (the M-block before a head is converted during the head's MFMAs)
            head[nb] = acc[nb];
            if constexpr (P::kSplit) head[nb] *= st.out_scale * st.lane_mul;
            if constexpr (P::kM16) {  // head value c of the sample of lane 16 g + (l & 15), g = 0, 1: fragment 2 (c >> 2) + g (head_row_m16)
              const f32x16 v = head[nb];
              const bool g1 = (g16 & 1) != 0;
#pragma unroll
              for (int c = 0; c < 8; ++c) {
                if (HALF && c >= 4) head[nb][c] = 0.f;   // half 1 was not computed (fragments q = nb only)
#ifdef DFN_MLP_LEAN_TU
                // the lean unit: the two candidates behind an opaque copy.  The select of two extractelements of one vector is
                // otherwise folded into one extract with a lane-dependent index, and an f32x16 in VGPRs has no indexed read: 15
                // v_cmp_eq_u32 + 16 v_cndmask_b32 per index register, the 15 masks held in SGPR pairs.  This is one v_cndmask_b32.
                else {
                  float a0 = v[8 * (c >> 2) + (c & 3)], a1 = v[8 * (c >> 2) + 4 + (c & 3)];
                  asm("" : "+v"(a0), "+v"(a1));
                  head[nb][c] = g1 ? a1 : a0;
                }
#else
                else head[nb][c] = g1 ? v[8 * (c >> 2) + 4 + (c & 3)] : v[8 * (c >> 2) + (c & 3)];
#endif
              }
            }
          }
        }
      }
    }
  }
  if (PIPE && MB >= 1 && !EXTRA) {  // the last M-block has no successor inside this layer
    if (COUT) {
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) carry[nb] = pend[nb];
    } else {
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) store_hidden<P, RELU>(pend[nb], Bout[nb], MB - 1, st.out_scale * st.lane_mul, rmax_);
    }
  }
}

// ------------------------------------------------------------------------------------------
// Positional encoding of a point into the layer-1 B operand (slot map: pe_xyz_feature()).
// FAST: x/(2pi) in two-term extended precision, exact fract, then v_sin_f32 / v_cos_f32 (which
// take revolutions), five octaves per coordinate-half from one evaluation by double-angle steps.  Otherwise: split-f16 takes
// every octave from the same exact-fract hardware path (4e-7), exact fp32 the full-range sinf/cosf of the exact product
// x * 2^k, bit-for-bit the reference's sin(x * freq) up to libm rounding.
template <class P, bool FAST, int NB, int PC>
DFN_DEV void posenc_xyz(const float (&x)[NB][3], int h, typename FragOf<P>::type (&pe)[NB][PC]) {
  const float base = h ? 32.f : 1.f;  // half h owns frequencies 2^(5h) .. 2^(5h+4)
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float xc = x[nb][c];
      if (FAST) {
        float uh, ul, sn[5], cs[5];
        rev_split(xc, uh, ul);
        rev_sincos_octaves5(uh, ul, base, sn, cs);
#pragma unroll
        for (int k = 0; k < 5; ++k) {
          set_slot<P>(pe[nb], 6 * k + c, sn[k]);
          set_slot<P>(pe[nb], 6 * k + 3 + c, cs[k]);
        }
      } else if constexpr (P::kSplit) {
        // split-f16: every octave from the exact-fract hardware path (x / 2pi in two-term extended precision, exact v_fract,
        // v_sin / v_cos in revolutions; max abs error 4.1e-7 vs fp64 = fp32 round-off of the encoding).  libm's full-range
        // sinf / cosf expand to ~60 instructions each (large-argument reduction): 60 of them per point were HALF of this
        // kernel's instruction stream (7 000 of 16 900 per tile, next to 1 080 MFMAs).
        float uh, ul;
        rev_split(xc, uh, ul);
#pragma unroll
        for (int k = 0; k < 5; ++k) {
          float sn, cs;
          rev_sincos(uh, ul, base * float(1 << k), sn, cs);
          set_slot<P>(pe[nb], 6 * k + c, sn);
          set_slot<P>(pe[nb], 6 * k + 3 + c, cs);
        }
      } else {
        const float xb = xc * base;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
          const float a = xb * float(1 << k);
          set_slot<P>(pe[nb], 6 * k + c, sinf(a));
          set_slot<P>(pe[nb], 6 * k + 3 + c, cosf(a));
        }
      }
    }
    set_slot<P>(pe[nb], 30, h ? x[nb][2] : x[nb][0]);
    set_slot<P>(pe[nb], 31, h ? 0.f : x[nb][1]);
  }
}

// PrecX3M16: the same exact-fract hardware path for the two points of a lane (16 nb + (lane & 15)), 16 slots each in lane group g
// (slot map: pe_xyz_feature_m16): octaves 2g, 2g+1 of all three coordinates, then two of the six (coordinate, octave 8 | 9) pairs —
// group 3 puts the raw coordinates there.  Eight sin/cos evaluations per point and lane, as the 32x32 kernels' fifteen per point and half.
template <class P, int PC>
DFN_DEV void posenc_xyz_m16(const float (&x)[2][3], int g, typename FragOf<P>::type (&pe)[1][PC]) {
  static_assert(P::kM16 && PC == 4, "16 slots of two points");
  auto put = [&](int n, int s, float v) {
    _Float16 hi, lo;
    x3_split(v, hi, lo);
    pe[0][2 * (s >> 3) + n].hi[s & 7] = hi;
    pe[0][2 * (s >> 3) + n].lo[s & 7] = lo;
  };
  const float base = float(1 << (2 * g));          // octaves 2g, 2g + 1
  const float f6 = g == 2 ? 512.f : 256.f, f7 = g == 0 ? 256.f : 512.f;   // octave of the pairs rho = 2g, 2g + 1
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    float uh[3], ul[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) rev_split(x[n][c], uh[c], ul[c]);
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float sn, cs;
        rev_sincos(uh[c], ul[c], base * float(1 << k), sn, cs);
        put(n, 6 * k + c, sn);
        put(n, 6 * k + 3 + c, cs);
      }
    // rho = 2g: coordinate 0, 2, 1 (g = 0, 1, 2); rho = 2g + 1: coordinate 1, 0, 2
    float s6, c6, s7, c7;
    rev_sincos(g == 0 ? uh[0] : (g == 1 ? uh[2] : uh[1]), g == 0 ? ul[0] : (g == 1 ? ul[2] : ul[1]), f6, s6, c6);
    rev_sincos(g == 0 ? uh[1] : (g == 1 ? uh[0] : uh[2]), g == 0 ? ul[1] : (g == 1 ? ul[0] : ul[2]), f7, s7, c7);
    if (g == 3) { s6 = x[n][0]; c6 = x[n][1]; s7 = x[n][2]; c7 = 0.f; }
    put(n, 12, s6); put(n, 13, c6); put(n, 14, s7); put(n, 15, c7);
  }
}

// ------------------------------------------------------------------------------------------
// The 8-layer trunk (xyz_encoding_1..8, skip concat [pe, h] before layer 5).
// `hook(l, h)` (optional) is called once per trunk layer l = 0..6 with that layer's COMPLETE output operand (point block 0) — one
// layer late, because a pipelined layer hands its last M-block to the next layer unconverted; layer 7's output (`out`) completes in
// the caller's next layer.  The saving forward of the gradient path records the ReLU signs there (nerfh_mlp.hip).
struct NoTrunkHook {
  template <class A> DFN_DEV void operator()(int, A&) const {}
};
// RES_L1 >= 0: layer 1 is LDS-resident at that offset (kernel variant 7's coarse kernel: layer<..., RES>).
// kEncodingKept: the lean unit (DFN_MLP_LEAN_TU), see the skip concat below.
#ifdef DFN_MLP_LEAN_TU
constexpr bool kEncodingKept = true;
#else
constexpr bool kEncodingKept = false;
#endif
template <class P, int UMB, bool PIPE, bool FAST, int NB, int W = kWidth, class Hook = NoTrunkHook, int RES_L1 = -1>
DFN_DEV void trunk(Stager& st, char* smem, const float (&x)[lane_pts<P>(NB)][3],
                   typename FragOf<P>::type (&out)[NB][chunks_of<P>(W / 2)], f32x16 (&carry)[NB], Hook hook = Hook()) {
  using F = typename FragOf<P>::type;
  constexpr int PC = chunks_of<P>(32), HC = chunks_of<P>(W / 2), MBW = W / 32;
  constexpr bool CY = PIPE && P::kSlotsPerChunk == 8;  // hand a layer's last M-block to the next layer unconverted
  constexpr int CI = CY ? HC - 2 : -1;                 // ... where it lands in the last two chunks of the W-wide input
  static_assert(!PIPE || W == kWidth, "the pipelined epilogue is tuned for netwidth 128");
  const int h = st.lane >> 5;
  f32x16 nohead[NB];
  const float* const norb[lane_pts<P>(NB)] = {};
  F pe[NB][PC];
  auto encode = [&](const float (&xx)[lane_pts<P>(NB)][3]) {
    if constexpr (P::kM16) { static_assert(!FAST, "split-f16 only"); posenc_xyz_m16<P, PC>(xx, st.lane >> 4, pe); }
    else posenc_xyz<P, FAST, NB, PC>(xx, h, pe);
  };
  encode(x);
  F a[NB][HC], b[NB][HC];
  layer<P, UMB, PIPE, NB, PC, MBW, true, false, false, RES_L1 < 0, -1, true, CY, false, false, true, false, RES_L1>(st, smem, pe, a, nohead, norb, carry);
  layer<P, UMB, PIPE, NB, HC, MBW, true, false, false, true, CI, true, CY>(st, smem, a, b, nohead, norb, carry);
  hook(0, a[0]);
  layer<P, UMB, PIPE, NB, HC, MBW, true, false, false, true, CI, true, CY>(st, smem, b, a, nohead, norb, carry);
  hook(1, b[0]);
  layer<P, UMB, PIPE, NB, HC, MBW, true, false, false, true, CI, true, CY>(st, smem, a, b, nohead, norb, carry);
  hook(2, a[0]);
  {
    F cat[NB][PC + HC];
    // The skip concat's encoding.  The f16 / split-f16 kernels form it a SECOND time here, from an opaque copy of the coordinates:
    // in the 32x32 kernels (and the f16 one without the pipelined epilogue) 32 more VGPRs live across layers 2 to 4 cost more than
    // the evaluation.  The lean unit (kEncodingKept, its 16x16x32 kernels) keeps layer 1's operand instead:
    // those kernels have the registers free across layers 2 to 4 and their peak is inside layer 5, where the encoding is an operand
    // in either form.  The pipelined f16 kernel and exact fp32 have always kept it.
    if constexpr (P::kSlotsPerChunk == 8 && (!PIPE || P::kSplit) && !(kEncodingKept && P::kM16)) {
      float x2[lane_pts<P>(NB)][3];
#pragma unroll
      for (int nb = 0; nb < lane_pts<P>(NB); ++nb)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          x2[nb][c] = x[nb][c];
          asm volatile("" : "+v"(x2[nb][c]));  // opaque copy: stops the compiler from CSE-ing the two encodings
        }
      encode(x2);
    }
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
#pragma unroll
      for (int i = 0; i < PC; ++i) cat[nb][i] = pe[nb][i];
#pragma unroll
      for (int i = 0; i < HC; ++i) cat[nb][PC + i] = b[nb][i];
    }
    layer<P, l5_unit_mb_p<P>(UMB), PIPE, NB, PC + HC, MBW, true, false, false, true, (CY ? PC + HC - 2 : -1), true, CY>(st, smem, cat, a, nohead, norb, carry);
    hook(3, reinterpret_cast<F(&)[HC]>(cat[0][PC]));   // layer 4's output: the h part of the skip concat, completed inside layer 5
  }
  layer<P, UMB, PIPE, NB, HC, MBW, true, false, false, true, CI, true, CY>(st, smem, a, b, nohead, norb, carry);
  hook(4, a[0]);
  layer<P, UMB, PIPE, NB, HC, MBW, true, false, false, true, CI, true, CY>(st, smem, b, a, nohead, norb, carry);
  hook(5, b[0]);
  layer<P, UMB, PIPE, NB, HC, MBW, true, false, false, true, CI, true, CY>(st, smem, a, out, nohead, norb, carry);  // out's last two chunks stay in `carry`
  hook(6, a[0]);
}

}  // namespace dfn
