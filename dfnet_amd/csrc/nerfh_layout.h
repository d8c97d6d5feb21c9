// nerfh_layout.h — the NeRF-H MLP as a sequence of MFMA "layers", shared by the host-side
// weight packer (nerfh_pack.cpp) and the device kernels (nerfh_mlp.hip).
//
// Formulation: every Linear is computed TRANSPOSED on the matrix cores,
//     H_out^T[feature, point] = W[feature, k] * H_in^T[k, point]
// with the weights as the MFMA A operand (M = 32 output features per M-block) and the
// activations of 32 points as the B operand (N = 32 points).  The 32x32 C/D fragment of lane
// (p = lane&31, h = lane>>5) holds, for point p, output features
//     row(h, r) = (r&3) + 8*(r>>2) + 4*h,  r = 0..15
// of the M-block.  Because the order of the contraction index is free, the C registers of
// one layer ARE the B operand of the next once the next layer's weight columns are
// permuted to match — activations never leave registers between layers.
//
// "Slot" s of half h: the s-th contraction element held by the lanes of half h.  A layer with
// K (padded) inputs has K/2 slots per half.  f16 path: 8 slots per MFMA K-chunk
// (v_mfma_f32_32x32x16_f16), f32 path: 1 slot per chunk (v_mfma_f32_32x32x2_f32).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define DFN_HD __host__ __device__
#else
#define DFN_HD
#endif

namespace dfn {

constexpr int kWidth = 128;      // netwidth the kernels are specialised for
constexpr int kLxyz = 10;        // multires
constexpr int kLdir = 4;         // multires_views
constexpr int kChXyz = 63, kChDir = 27;

enum LayerId {
  LY_L1 = 0, LY_L2, LY_L3, LY_L4, LY_L5, LY_L6, LY_L7, LY_L8,
  LY_FIN,    // xyz_encoding_final (4 M-blocks, no activation) + static_sigma (5th M-block, row 0)
  LY_DIR,    // dir_encoding.0 on the `final` columns; pe_dir/appearance columns fold into a per-ray bias
  LY_RGB,    // static_rgb.0 (rows 0..2)
  LY_TE0,    // transient_encoding.0 on the `final` columns; transient-embedding columns -> per-ray bias
  LY_TE1, LY_TE2, LY_TE3,  // transient_encoding.{2,4,6}
  LY_THEAD,  // rows 0..2 transient_rgb, row 3 transient_sigma, row 8 transient_beta (all on half 0)
  LY_SIG,    // static_sigma alone (row 0): the coarse net, and the fine net of kernel variant 5
  // kernel variant 5 (xyz_encoding_final folded at commit): h8 -> 64 directly, the shapes of LY_DIR / LY_TE0
  LY_DIRF,   // (dir_encoding.0[:, :W] . xyz_encoding_final) on h8; the per-ray bias also carries dir_encoding.0[:, :W] . b_final
  LY_TE0F,   // (transient_encoding.0[:, :W] . xyz_encoding_final) on h8, likewise
  LY_COUNT
};

struct LayerShape { int slots; int mb; };  // slots per half (= K/2), number of 32-row M-blocks

// W = netwidth: 128 (every kernel variant) or 256 (the plain one-M-block-unit variants, nerfh_mlp.hip).
DFN_HD constexpr LayerShape layer_shape(int id, int W = kWidth) {
  return id == LY_L1 ? LayerShape{32, W / 32}
       : id == LY_L5 ? LayerShape{32 + W / 2, W / 32}
       : id <= LY_L8 ? LayerShape{W / 2, W / 32}
       : id == LY_FIN ? LayerShape{W / 2, W / 32 + 1}
       : id == LY_DIR ? LayerShape{W / 2, W / 64}
       : id == LY_RGB ? LayerShape{W / 4, 1}
       : id == LY_TE0 ? LayerShape{W / 2, W / 64}
       : id <= LY_TE3 ? LayerShape{W / 4, W / 64}
       : id == LY_THEAD ? LayerShape{W / 4, 1}
       : id == LY_DIRF || id == LY_TE0F ? LayerShape{W / 2, W / 64}
       : LayerShape{W / 2, 1};  // LY_SIG
}

// The layer sequences the kernels execute, in order.
constexpr int kCoarseSeq[] = {LY_L1, LY_L2, LY_L3, LY_L4, LY_L5, LY_L6, LY_L7, LY_L8, LY_SIG};
constexpr int kFineSeq[] = {LY_L1, LY_L2, LY_L3, LY_L4, LY_L5, LY_L6, LY_L7, LY_L8, LY_FIN,
                            LY_DIR, LY_RGB, LY_TE0, LY_TE1, LY_TE2, LY_TE3, LY_THEAD};
// Kernel variant 5: xyz_encoding_final has no activation and feeds only dir_encoding.0 and transient_encoding.0, so the packer
// multiplies it into them (LY_DIRF, LY_TE0F) and the kernel never forms `final`; static_sigma reads h8 as its own head block.
constexpr int kFineFoldSeq[] = {LY_L1, LY_L2, LY_L3, LY_L4, LY_L5, LY_L6, LY_L7, LY_L8, LY_SIG,
                                LY_DIRF, LY_RGB, LY_TE0F, LY_TE1, LY_TE2, LY_TE3, LY_THEAD};
static_assert(sizeof(kFineFoldSeq) == sizeof(kFineSeq), "the folded sequence has the layer count of the plain one");
// Staging-unit group of each layer when a unit may hold whole layers (unit_mb >= 8): small layers share a unit.
constexpr int kCoarseGroup[] = {0, 1, 2, 3, 4, 5, 6, 7, 7};
constexpr int kFineGroup[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 10, 10, 10, 10, 10};
constexpr int kCoarseLayers = sizeof(kCoarseSeq) / sizeof(int);
constexpr int kFineLayers = sizeof(kFineSeq) / sizeof(int);
// The coarse network's TRAINING query (nerfw.py:47-60, 326-343: the output_transient=False branch, [static_rgb(3), static_sigma]): the
// fine sequence cut off behind static_rgb, on the coarse network's weights -- dir_encoding.0 there is [W/2, W + 27] (no appearance
// columns), which LY_DIR / LY_DIRF read through the matrix's own leading dimension (Packer::mat).  Plain (f16, exact fp32, netwidth 256)
// and folded (split-f16 at netwidth 128, as kFineFoldSeq); the group table is kFineGroup's head.  nerfh_mlp_static_pts*.hip.
constexpr int kCoarseStaticSeq[] = {LY_L1, LY_L2, LY_L3, LY_L4, LY_L5, LY_L6, LY_L7, LY_L8, LY_FIN, LY_DIR, LY_RGB};
constexpr int kCoarseStaticFoldSeq[] = {LY_L1, LY_L2, LY_L3, LY_L4, LY_L5, LY_L6, LY_L7, LY_L8, LY_SIG, LY_DIRF, LY_RGB};
constexpr int kCoarseStaticGroup[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9};
constexpr int kCoarseStaticLayers = sizeof(kCoarseStaticSeq) / sizeof(int);
static_assert(sizeof(kCoarseStaticFoldSeq) == sizeof(kCoarseStaticSeq) && sizeof(kCoarseStaticGroup) == sizeof(kCoarseStaticSeq),
              "one entry per layer of the static sequence");
// (M-block, 8-slot K-chunk) pairs of a sequence: x 1 (f16), x 3 (split-f16 32x32x16) or x 6 (split-f16 16x16x32) MFMAs per 32-point
// block -- the fine sequences give the 2 160 / 1 968 of "Kernel variants" below.  What the expected time ratio of two kernels on the
// same geometry is computed from: static 316 / fine 360 = 0.878 plain, 284 / 328 = 0.866 folded.
DFN_HD constexpr int seq_chunks(const int* seq, int n, int W = kWidth) {
  int c = 0;
  for (int i = 0; i < n; ++i) c += layer_shape(seq[i], W).slots / 8 * layer_shape(seq[i], W).mb;
  return c;
}
static_assert(seq_chunks(kFineSeq, kFineLayers) == 360 && seq_chunks(kFineFoldSeq, kFineLayers) == 328 &&
              seq_chunks(kCoarseStaticSeq, kCoarseStaticLayers) == 316 && seq_chunks(kCoarseStaticFoldSeq, kCoarseStaticLayers) == 284,
              "MFMA chunk counts of the sequences");

// Feature index (within a 128- or 64-wide hidden vector) held in slot s of half h when the
// vector was produced by M-blocks of a previous layer.
DFN_HD constexpr int hidden_feature(int h, int s) {
  return 32 * (s >> 4) + 4 * h + (s & 3) + 8 * ((s & 15) >> 2);
}
// Row of an M-block held in C register r of half h.
DFN_HD constexpr int mblock_row(int h, int r) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// Slot -> column of the 63-wide xyz positional encoding (-1 = zero padding).  Half h computes
// frequencies 5h..5h+4: slots 6k'+c (c<3: sin of coord c, c>=3: cos of coord c-3), then the
// raw coordinates in slots 30, 31 (half 0: x, y; half 1: z, pad).
DFN_HD constexpr int pe_xyz_feature(int h, int s) {
  return s < 30 ? 3 + 6 * (5 * h + s / 6) + (s % 6) : (s == 30 ? (h ? 2 : 0) : (h ? -1 : 1));
}

// PrecX3M16: feature held in slot s (0 .. K/4 - 1, s = 8 k32 + j) of lane group g when the vector was produced by M-blocks of a
// previous layer: rows 16 (j >> 2) + 4 g + (j & 3) of M-block k32.
DFN_HD constexpr int hidden_feature_m16(int g, int s) { return 32 * (s >> 3) + 16 * ((s & 7) >> 2) + 4 * g + (s & 3); }
// PrecX3M16 positional-encoding slot map: 16 slots per lane group and point.  Slots 0..11: octaves 2g, 2g+1 (6k'+c sin of coord c,
// 6k'+3+c cos); slots 12..15 = two (sin, cos) pairs rho = 2g, 2g+1 of the last two octaves (rho < 6: coord rho % 3, octave
// 8 + rho / 3), group 3 holds the raw coordinates there instead (x, y, z, pad).
DFN_HD constexpr int pe_xyz_feature_m16(int g, int s) {
  return s < 12 ? 3 + 6 * (2 * g + s / 6) + (s % 6)
       : (g == 3 ? (s < 15 ? s - 12 : -1)
                 : 3 + 6 * (8 + (2 * g + ((s - 12) >> 1)) / 3) + 3 * ((s - 12) & 1) + (2 * g + ((s - 12) >> 1)) % 3);
}
// PrecX3M16 head M-blocks: row i (0..31) of the packed block -> row of the 32x32 head block it copies (-1 = zero).  Head value c (the
// C register of half 0 that carries it in the 32x32 kernels: row mblock_row(0, c)) goes to rows 16 (c >> 2) + 4 g + (c & 3) of lane
// groups g = 0, 1: fragment q = 2 (c >> 2) + g holds it for the sample of lane 16 g + (l & 15).
DFN_HD constexpr int head_row_m16(int i) {
  return ((i >> 2) & 3) < 2 ? (i & 3) + 8 * (i >> 4) : -1;
}

// Per-precision fragment geometry.
struct PrecF16 { static constexpr int kSlotsPerChunk = 8, kLaneBytes = 16; static constexpr bool kSplit = false, kM16 = false; };
struct PrecF32 { static constexpr int kSlotsPerChunk = 1, kLaneBytes = 4; static constexpr bool kSplit = false, kM16 = false; };
// Split-f16: every operand is hi + lo in f16 (hi = f16(x), lo = f16(x - hi)) and a product is accumulated in fp32
// as hi*hi + hi*lo + lo*hi — three v_mfma_f32_32x32x16_f16 instead of eight v_mfma_f32_32x32x2_f32 per 16
// contraction elements, fp32-grade results (the dropped lo*lo term is 2^-22 relative).  A fragment = 8 hi + 8 lo
// halves per lane.  Operands are pre-scaled by powers of two (activations x kX3ActScale, weights x 2^s per
// network) so the lo parts stay normal f16 numbers; MlpArgs::{in,out}_scale carry the product and its inverse.
struct PrecX3 { static constexpr int kSlotsPerChunk = 8, kLaneBytes = 32; static constexpr bool kSplit = true, kM16 = false; };
constexpr float kX3ActScale = 16.f;
// Split-f16 on v_mfma_f32_16x16x32_f16 (kernel variant 4).  A 32-row M-block is two 16-row halves ms = 0, 1 and a wave's 32 points
// are two 16-point N-blocks nb = 0, 1.  The array geometry is PrecX3's, only what sits where differs:
//   - A fragment t = (k32 = kc >> 1, ms = kc & 1) of an M-block: 16 rows x 32 K, lane l holds row 16 ms + (l & 15),
//     k = 32 k32 + 8 (l >> 4) + j (j = 0..7), hi plane then lo plane (2 KB, lane-linear 16-byte reads, as PrecX3);
//   - B chunk c = 2 k32 + nb: the 32-K chunk k32 of N-block nb, lane l holds point 16 nb + (l & 15), k as above;
//   - the f32x16 accumulator of an M-block = four 16x16 C fragments q = 2 ms + nb (registers 4q..4q+3), lane l holding
//     rows 16 ms + 4 g + r (g = l >> 4, r = 0..3) of point 16 nb + (l & 15).
// Rows of hidden M-blocks are the layer's output features in order, so two converted C fragments (ms = 0, 1) of one N-block are the
// next layer's B chunk directly (hidden_feature_m16); head M-blocks duplicate their rows on lane groups 0 and 1 (head_row_m16) so that
// head value c of sample p lands on lane p of half 0 with one select.
struct PrecX3M16 { static constexpr int kSlotsPerChunk = 8, kLaneBytes = 32; static constexpr bool kSplit = true, kM16 = true; };

// Kernel variants (DFN_MLP_VARIANT, an A/B aid; nerfh_mlp.hip).  0 to 3 differ in workgroup width and staging granularity:
//   variant 0: 8 waves per workgroup, 1 workgroup per CU, a unit = a whole layer (f16) / one M-block (f32)
//   variant 1: 4 waves per workgroup, 2 workgroups per CU, a unit = 2 M-blocks (f16) / one M-block (f32)
//   variant 2: 4 waves per workgroup x 3 point blocks, 1 workgroup per CU (1 wave per SIMD, 512 VGPRs), unit as variant 0
//   variant 3: variant 0's geometry without the pipelined epilogue (A/B reference)
// 4 to 12 exist in split-f16 at netwidth 128 only and each is the one before it with more (kVariantFacts); every other
// arithmetic mode, width and gradient path under them runs the `base` variant's kernels on its networks, and which kernel, network and
// per-ray table a call runs is nerfh_route.h:
//   variant 4: variant 0 on 16x16x32 MFMAs (PrecX3M16)
//   variant 5: the FINE kernel's tail folded (kFineFoldSeq, nerfh_mlp_fold.hip: 1 968 MFMAs per 32-point tile instead of 2 160)
//   variant 6: HALF-HEIGHT head M-blocks (nerfh_mlp_half.hip): a PrecX3M16 head block keeps its values c = 0..3 on the 16-row half
//              ms = 0 (head_row_m16), so static_sigma, static_rgb and -- where transient_beta reaches no output: compositing fused, no
//              maps -- the transient head are packed and multiplied as their ms = 0 fragments only (1 920 / 1 932 MFMAs per fine tile
//              plain / maps, 1 560 per coarse tile instead of 1 584)
//   variant 7: a fixed set of small layers RESIDENT in LDS in the coarse and the plain fused fine kernel (nerfh_mlp_res.hip;
//              kCoarseResident / kFineResident below): copied in once per workgroup behind the input slots, they leave the streamed
//              unit table (coarse 17 -> 14 units, fine 26 -> 22 per 256-point tile) with their barriers and DMA round trips; the same
//              fragments, MFMAs and conversion pieces in the same order: variant 6's outputs bit for bit
//   variant 12: variant 7's two kernels with per-tile work that the result does not need taken out (the lean unit, nerfh_mlp_lean.hip),
//              on variant 7's packed networks (it packs none of its own, so it is no index of dfn_nerfh_s::net) and resident blob.
//              Every technique gives the same values on the same lanes and the same range flag: variant 7's outputs bit for bit, which
//              makes variant 7 the independently written anchor that the lean unit is tested against.  One paragraph per technique:
//              CLAIMED tiles: the tiles are claimed from a device counter instead of dealt blockIdx.x, + gridDim.x, ...: scheduling
//              only.  Both tile counters are zeroed in front of a pass in which either kernel is the lean unit's.
//              KEPT encoding: the positional encoding is formed ONCE per tile and kept for the skip concat in front of layer 5 instead
//              of formed a second time there (trunk() in nerfh_mlp_core.h): 32 registers live across layers 2 to 4, which the
//              16x16x32 kernels have free, against 231 vector instructions per tile and wave, 32 of them quarter-rate v_sin / v_cos.
//              The kept operand is the value the second evaluation gives.
//              SCALED seeds and uniform values at their use, in the fused fine kernel: ray_bias_kernel writes the table of that route
//              multiplied by the fine network's in_scale, once per pass, instead of layer() multiplying the loaded seeds of the two
//              RAYBIAS layers on every tile; and uniform values (the weight DMA's per-wave piece, prefetch slot addresses, argument
//              pointers) are formed where they are used instead of parked in VGPR lanes and read back by v_readlane_b32 (79 -> 39
//              parked SGPRs, 231 -> 62 lane reads per tile).  The coarse kernel has no RAYBIAS layer and parks nothing.
//              ONE SELECT per head value of a PrecX3M16 head block (layer() in nerfh_mlp_core.h: the two candidates go through an
//              opaque copy, so the select of two extracted elements is not rewritten as one extract with a lane-dependent index -- a
//              chain of 15 compares and 16 selects per index register, whose masks were the scalar pressure behind the parked SGPRs:
//              4 023 -> 3 754 vector instructions per fine tile, 39 -> 0 parked SGPRs; coarse 2 728 -> 2 707).
//              LEAN tile seam and range guard: in the fine kernel the eight head activations are evaluated as four (the static
//              pre-activations ride on lanes 32..63, which carry no sample there); in both kernels the point -> ray division is a
//              multiply-high and a shift (nerfh_raydiv.h) and the range guard of the ReLU conversions is one v_pk_maximum3_f16 per two
//              pieces instead of one v_pk_max_u16 per piece (336 -> 168 / 256 -> 128 per tile): 3 754 -> 3 414 / 2 707 -> 2 556
//              vector instructions.
//   variants 8 to 11 were the steps by which variant 12 was reached, one technique at a time in the order above, each with a unit of its
//              own that gave its predecessor's outputs bit for bit (LABBOOK.md).  They are retired: the numbers stay accepted and
//              mean variant 12 (kVariantFacts), whose outputs are the bits theirs were
constexpr int kVariants = 8;   // packed networks per (coarse | fine, arithmetic): dfn_nerfh_s::net
constexpr int kFoldVariant = 5;
constexpr int kHalfVariant = 6;
constexpr int kResidentVariant = 7;
constexpr int kLeanVariant = 12;
constexpr int kLastVariant = kLeanVariant;   // DFN_MLP_VARIANT = 0 .. kLastVariant
// lean: the coarse and the plain fused fine kernel are nerfh_mlp_lean.hip's: they claim their tiles and the fine one's per-ray table
// holds in_scale x the seeds
struct VariantFacts { int base; bool fold, half, resident, lean; };
constexpr VariantFacts kLeanFacts = {4, true, true, true, true};
constexpr VariantFacts kVariantFacts[kLastVariant + 1] = {
    {0, false, false, false, false}, {1, false, false, false, false}, {2, false, false, false, false}, {3, false, false, false, false},
    {4, false, false, false, false},
    {4, true, false, false, false},   // kFoldVariant
    {4, true, true, false, false},    // kHalfVariant
    {4, true, true, true, false},     // kResidentVariant
    kLeanFacts, kLeanFacts, kLeanFacts, kLeanFacts,   // 8 to 11, retired: kLeanVariant's row
    kLeanFacts,                       // kLeanVariant
};
// kSelectedByDefault: what a process runs without DFN_MLP_VARIANT.  kPointsVariant: the variant whose routes the point queries take
// whatever DFN_MLP_VARIANT says (they have no resident or lean flavour: variant 6's coarse and variant 5's fine kernel)
constexpr int kSelectedByDefault = kLeanVariant;
constexpr int kPointsVariant = kResidentVariant;
template <class P> DFN_HD constexpr int unit_mb(int variant) {
  return P::kSlotsPerChunk == 1 ? 1 : (P::kSplit ? 2 : (variant == 1 ? 2 : 8));
}
DFN_HD constexpr int variant_waves(int variant) { return variant == 0 ? 8 : 4; }
// netwidth 256: M-blocks per staging unit
template <class P> DFN_HD constexpr int unit_mb_w256() { return (P::kSlotsPerChunk == 1 || P::kSplit) ? 1 : 2; }

constexpr uint32_t kPiece = 1024;  // staging granule: one wave-wide 16-byte LDS-DMA

DFN_HD constexpr uint32_t align_piece(uint32_t b) { return (b + kPiece - 1) / kPiece * kPiece; }

// Bytes of one staging unit holding `nmb` M-blocks of a layer with `slots` slots per half.  half: a half-height PrecX3M16 head
// block (kernel variant 6): the fragments of its 16-row half ms = 0 only; the 128-byte bias block keeps its size.
template <class P>
DFN_HD constexpr uint32_t unit_bytes(int slots, int nmb, bool half = false) {
  return align_piece(uint32_t(nmb) * (slots / P::kSlotsPerChunk / (half ? 2 : 1)) * 64 * P::kLaneBytes + uint32_t(nmb) * 2 * 16 * 4);
}
// Largest unit of either network when at most `umb` M-blocks go into one unit (sizes the two LDS
// staging buffers): the widest layers are L5 (96 slots, 4 M-blocks) and FIN (64 slots, 5 M-blocks).
// In the merged layout (umb >= 8) layer 5 (48 fragments) is split into two units of 2 M-blocks so that THREE staging
// buffers fit the 160 KB of LDS; the largest unit is then the merged transient group (44 fragments + 9 bias blocks).
DFN_HD constexpr int l5_unit_mb(int umb) { return umb >= 8 ? 2 : umb; }
// ... per precision: split-f16 with two-M-block units keeps layer 5 (96 slots: 25 KB per M-block) in one-M-block units so that
// three staging buffers + the input-prefetch slots stay inside the LDS.
template <class P> DFN_HD constexpr int l5_unit_mb_p(int umb) { return (P::kSplit && umb == 2) ? 1 : l5_unit_mb(umb); }
template <class P>
DFN_HD constexpr uint32_t max_unit_bytes(int umb, int W = kWidth) {
  const int m5 = l5_unit_mb_p<P>(umb), mbw = W / 32;
  const uint32_t a = unit_bytes<P>(32 + W / 2, m5 < mbw ? m5 : mbw), b = unit_bytes<P>(W / 2, umb < mbw + 1 ? umb : mbw + 1);
  const uint32_t g = umb >= 8 ? align_piece(44u * 64 * P::kLaneBytes + 9u * 128) : 0;
  return a > b ? (a > g ? a : g) : (b > g ? b : g);
}

// ---- kernel variant 7: LDS-resident layers ------------------------------------------------------------------
// The layers a PrecX3M16 W = 128 render kernel keeps in LDS for its whole life instead of streaming them per tile, in EXECUTION order
// (the order of the resident blob).  Head blocks are in their variant-6 half-height form.  A second candidate is one line here.
//   fine (plain, compositing fused): static_sigma 8 320 + static_rgb 4 224 + transient_encoding.6 16 640 + transient head 4 224 = 33 408 B
//   coarse: layer 1 (its two units, 2 x 16 640) + static_sigma 8 320 = 41 600 B
constexpr int kCoarseResident[] = {LY_L1, LY_SIG};
constexpr int kFineResident[] = {LY_SIG, LY_RGB, LY_TE3, LY_THEAD};
DFN_HD constexpr int resident_count(bool fine) { return int(fine ? sizeof(kFineResident) : sizeof(kCoarseResident)) / int(sizeof(int)); }
DFN_HD constexpr int resident_at(bool fine, int i) { return fine ? kFineResident[i] : kCoarseResident[i]; }
DFN_HD constexpr bool layer_resident(bool fine, int id) {
  for (int i = 0; i < resident_count(fine); ++i)
    if (resident_at(fine, i) == id) return true;
  return false;
}
// half-height head blocks of the kernels that keep layers resident (Packer::half_block with half_thead set)
DFN_HD constexpr bool resident_half(int id) { return id == LY_SIG || id == LY_RGB || id == LY_THEAD; }
// Bytes of a resident layer: its M-blocks in staging-unit format ([fragments][128-byte bias blocks] per unit of <= unit_mb M-blocks,
// Packer::pack_blocks), units back to back WITHOUT the rounding to pieces: mb x (fragment bytes + 128) whatever the unit size.
template <class P>
DFN_HD constexpr uint32_t resident_layer_bytes(int id) {
  const LayerShape sh = layer_shape(id);
  return uint32_t(sh.mb) * (uint32_t(sh.slots / P::kSlotsPerChunk / (resident_half(id) ? 2 : 1)) * 64 * P::kLaneBytes + 128u);
}
// Offset of resident layer `id` inside the resident region; id = LY_COUNT: the bytes of the whole set.
template <class P>
DFN_HD constexpr uint32_t resident_offset(bool fine, int id) {
  uint32_t off = 0;
  for (int i = 0; i < resident_count(fine) && resident_at(fine, i) != id; ++i) off += resident_layer_bytes<P>(resident_at(fine, i));
  return off;
}
// The region is filled by whole wave-wide DMA pieces: the set's bytes rounded up ONCE (the blob is zero-padded to match).
template <class P> DFN_HD constexpr uint32_t resident_bytes(bool fine) { return align_piece(resident_offset<P>(fine, LY_COUNT)); }
constexpr uint32_t kLdsBytes = 163840;   // LDS of a CU (gfx950)

// ---- input-gradient kernel (nerfh_bwd.hip) ---------------------------------------------------------------
// The backward pass of a Linear is the same transposed product with W^T as the A operand: the rows of an
// M-block are INPUT features of the forward layer and the contraction slots are its OUTPUT features, in the
// C-fragment order the previous backward layer leaves them in (hidden_feature()).
enum BwdLayerId {
  BW_THEAD = 0,  // [d rgb_t(3), d sigma_t, d beta] -> d t3 (64)
  BW_TE3, BW_TE2, BW_TE1,   // transient_encoding.{6,4,2}^T
  BW_RGB,        // d rgb_s(3) -> d dir_h (64)
  BW_FINCAT,     // [d t0_pre (64) ; d dir_pre (64)] -> d final (128) + 5th M-block: d pe_dir (27, pe_dir_feature())
  BW_FIN,        // [d final (128) ; d sigma_s_pre] -> d h8 (128)
  BW_L8, BW_L7, BW_L6,
  BW_L5,         // d h5_pre -> d h4 (128) + M-blocks 4,5: d pe_xyz in positional-encoding slot order
  BW_L4, BW_L3, BW_L2,
  BW_L1,         // d h1_pre -> d pe_xyz (M-blocks 0,1)
  BW_COUNT,
  // the coarse network's gradient kernel only (kBwdCoarseSeq; no part of the fine blob, which packs BW_THEAD .. BW_L1):
  BW_SIG = BW_COUNT,  // d sigma_pre (slot 0 of half 0) -> d h8 (128): static_sigma's row as a column
  // the coarse network's training query (kBwdCoarseStaticSeq), behind BW_SIG so that no index of the blobs above moves:
  BW_DIRCAT           // d dir_pre (64) -> d final (128) + 5th M-block: d pe_dir (27, pe_dir_feature()): BW_FINCAT without its transient half
};
// The coarse network's input gradient (nerfh_bwd_coarse_pts.hip): sigma = softplus(static_sigma(h8)), so d h8 is seeded by BW_SIG
// and the chain is the trunk's.
constexpr int kBwdCoarseSeq[] = {BW_SIG, BW_L8, BW_L7, BW_L6, BW_L5, BW_L4, BW_L3, BW_L2, BW_L1};
constexpr int kBwdCoarseLayers = sizeof(kBwdCoarseSeq) / sizeof(int);
// The input gradient of the coarse network's training query (nerfh_bwd_coarse_static_pts.hip): raw4 = [sigmoid(static_rgb), softplus(static_sigma)],
// the fine chain without its transient branch, on the coarse network's weights.
constexpr int kBwdCoarseStaticSeq[] = {BW_RGB, BW_DIRCAT, BW_FIN, BW_L8, BW_L7, BW_L6, BW_L5, BW_L4, BW_L3, BW_L2, BW_L1};
constexpr int kBwdCoarseStaticLayers = sizeof(kBwdCoarseStaticSeq) / sizeof(int);
DFN_HD constexpr LayerShape bwd_layer_shape(int id) {
  return id == BW_SIG ? LayerShape{16, 4}
       : id == BW_DIRCAT ? LayerShape{32, 5}
       : id == BW_THEAD || id == BW_RGB ? LayerShape{16, 2}
       : id <= BW_TE1 ? LayerShape{32, 2}
       : id == BW_FINCAT ? LayerShape{64, 5}
       : id == BW_FIN ? LayerShape{80, 4}
       : id == BW_L5 ? LayerShape{64, 6}
       : id == BW_L1 ? LayerShape{64, 2}
       : LayerShape{64, 4};
}
// Lane (half h', register r) of a C fragment <-> row i of its M-block, inverted.
DFN_HD constexpr int mblock_half_of_row(int i) { return (i >> 2) & 1; }
DFN_HD constexpr int mblock_reg_of_row(int i) { return (i & 3) + 4 * (i >> 3); }
// Column of the 27-wide direction encoding whose gradient lands in C register r of half h of BW_FINCAT's 5th
// M-block: half h owns frequencies 2h, 2h+1 (r = 6k'+c: sin of coord c, 6k'+3+c: cos), half 0 also the raw
// direction in r = 12..14.  -1 = unused.
DFN_HD constexpr int pe_dir_feature(int h, int r) {
  return r < 12 ? 3 + 6 * (2 * h + r / 6) + (r % 6) : (h == 0 && r < 15 ? r - 12 : -1);
}
// Staging buffer of the backward kernel: its largest unit is BW_L5 (6 M-blocks x 64 slots) / L5 forward.
// M-blocks per staging unit of the gradient kernel: a whole layer (f16); exact fp32: one; split-f16: TWO — the per-M-block
// barrier was 15-21 % of these kernels (ablation without barriers); three 49 KB buffers still fit the 160 KB of LDS.  The
// backward units only pay off together with the bias-free backward layers (layer<..., NOBIAS>: 32 registers fewer).
template <class P> DFN_HD constexpr int bwd_fwd_unit_mb() { return (P::kSlotsPerChunk == 8 && !P::kSplit) ? 8 : (P::kSplit ? 2 : 1); }
template <class P> DFN_HD constexpr int bwd_unit_mb() { return (P::kSlotsPerChunk == 8 && !P::kSplit) ? 8 : (P::kSplit ? 2 : 1); }
template <class P>
DFN_HD constexpr uint32_t bwd_max_unit_bytes() {
  constexpr bool whole = P::kSlotsPerChunk == 8 && !P::kSplit;
  constexpr int uf = bwd_fwd_unit_mb<P>(), ub = bwd_unit_mb<P>();
  const uint32_t a = unit_bytes<P>(96, whole ? 4 : uf);  // forward layer 5 (no merged layout here)
  const uint32_t f5 = unit_bytes<P>(64, whole ? 5 : uf); // forward 128-wide layers / xyz_encoding_final
  const uint32_t b = unit_bytes<P>(64, whole ? 6 : ub), c = unit_bytes<P>(80, whole ? 4 : ub);
  const uint32_t m1 = a > f5 ? a : f5, m2 = b > c ? b : c;
  return m1 > m2 ? m1 : m2;
}

// Per-ray bias table written by the ray-bias kernel and read by the fine kernel:
// [ray][table(0 = dir_encoding, 1 = transient_encoding.0)][mb(2)][h(2)][r(16)] fp32.
constexpr int kRayBiasFloats = 2 * 2 * 2 * 16;   // netwidth 128
DFN_HD constexpr int ray_bias_floats(int W) { return W; }   // 2 tables x (W / 64) M-blocks x 2 halves x 16
constexpr int kMaxWidth = 256;   // widest netwidth of the register-resident kernels

}  // namespace dfn
