// nerfh_route.h — which kernel, which packed network and which per-ray-bias table a call of the register-resident NeRF-H MLP runs, as
// constexpr functions of (kernel variant, netwidth, arithmetic, fused compositing, maps wanted) over kVariantFacts (nerfh_layout.h).
// Host-side and free of HIP: nerfh_api.hip resolves a route, fills MlpArgs and hands both to its launch_route().  The static_asserts
// at the end are the specification; a new variant is one row of kVariantFacts, one enumerator here and its group of asserts.
#pragma once
#include "nerfh_layout.h"

namespace dfn {

constexpr int kPrecF16 = 0, kPrecF32 = 1, kPrecF16X3 = 2;   // DFN_PREC_* (include/dfnet_hip.h; nerfh_api.hip checks them)

enum Launcher {       // nerfh_kernels.h:
  kLaunchPlain,       // launch_mlp
  kLaunchMaps,        // launch_mlp_maps
  kLaunchFold,        // launch_mlp_fold(maps)
  kLaunchHalf,        // launch_mlp_half(fine, maps)
  kLaunchResident,    // launch_mlp_res
  kLaunchLean,        // launch_mlp_lean: claimed tiles (claims_tiles below); the fine kernel reads the per-ray table written at the
                      // accumulators' scale (Route::seed_scaled)
  kLaunchPoints,      // launch_mlp_pts
  kLaunchPointsFold,  // launch_mlp_pts_fold
  kLaunchPointsHalf,  // launch_mlp_pts_half
};
constexpr int kNetHalfMaps = -1;   // Route::net: dfn_nerfh_s::half_maps instead of an index of dfn_nerfh_s::net[fine][prec]
struct Route {
  Launcher launcher;
  int net;           // index of net[fine][prec][*], or kNetHalfMaps
  int variant;       // what launch_mlp / launch_mlp_maps take as `variant` (the other launchers have one geometry)
  bool fold_table;   // fine: the per-ray table is written from rb_fold (the seeds carry W[:, :128] . b_final) instead of rb
  bool maps;         // fine: the render-maps flavour of the kernel (kMapsRecFloats floats per segment record)
  bool seed_scaled;  // fine: the per-ray table of this launch holds in_scale x the seeds (launch_ray_bias's scale); no other kernel reads it
};

// the launchers whose kernels claim their tiles: both tile counters are zeroed in front of a pass in which either kernel is one of them
constexpr bool claims_tiles(Launcher l) { return l == kLaunchLean; }

// Netwidth 256 has one kernel per arithmetic: variant 0.  Variants 5 to 12 differ from their base in split-f16 only.
constexpr VariantFacts route_facts(int variant, int width) { return kVariantFacts[width == kWidth ? variant : 0]; }

// points: the point queries (dfn_mlp_*_points, called with kPointsVariant); they have no resident / lean flavour and run variant 6's
constexpr Route coarse_route(int variant, int width, int prec, bool points = false) {
  const VariantFacts f = route_facts(variant, width);
  const bool x3 = prec == kPrecF16X3;
  if (x3 && f.lean && !points) return {kLaunchLean, kResidentVariant, f.base, false, false};
  if (x3 && f.resident && !points) return {kLaunchResident, kResidentVariant, f.base, false, false};
  if (x3 && f.half) return {points ? kLaunchPointsHalf : kLaunchHalf, kHalfVariant, f.base, false, false};
  return {points ? kLaunchPoints : kLaunchPlain, f.base, f.base, false, false};
}
// fused: the compositing runs inside the fine kernel (fused_compositing below); otherwise raw goes to memory (the raw route)
constexpr Route fine_route(int variant, int width, int prec, bool fused, bool want_maps, bool points = false) {
  const VariantFacts f = route_facts(variant, width);
  const bool x3 = prec == kPrecF16X3, maps = fused && want_maps;
  if (x3 && f.lean && fused && !want_maps) return {kLaunchLean, kResidentVariant, f.base, true, false, true};
  if (x3 && f.resident && fused && !want_maps) return {kLaunchResident, kResidentVariant, f.base, true, false};
  if (x3 && f.half && fused) return {kLaunchHalf, want_maps ? kNetHalfMaps : kHalfVariant, f.base, true, want_maps};
  if (x3 && f.fold) return {points ? kLaunchPointsFold : kLaunchFold, kFoldVariant, f.base, true, maps};
  return {points ? kLaunchPoints : (maps ? kLaunchMaps : kLaunchPlain), f.base, f.base, false, maps};
}

// Compositing is fused into the fine kernel when a wave's points are one ray segment and raw is not wanted: 64 samples per wave in the
// f16 variants 0/1/3, 32 in the split-f16 and fp32 kernels (one point block per wave); the 3-block f16 variant and netwidth 256 keep
// the separate compositor.
constexpr int fused_segment(int prec) { return prec == kPrecF16 ? 64 : 32; }
constexpr bool fused_compositing(int variant, int width, int prec, int Nf, bool want_raw) {
  return !want_raw && Nf % fused_segment(prec) == 0 && !(prec == kPrecF16 && kVariantFacts[variant].base == 2) && width == kWidth;
}

// ---- the routes, written out -------------------------------------------------------------------------------------------------
namespace route_spec {
constexpr int W = kWidth, W2 = kMaxWidth, H = kPrecF16, F = kPrecF32, X = kPrecF16X3, HM = kNetHalfMaps;
constexpr bool is(const Route& r, Launcher l, int net, int variant, bool fold_table = false, bool maps = false, bool seed_scaled = false) {
  return r.launcher == l && r.net == net && r.variant == variant && r.fold_table == fold_table && r.maps == maps &&
         r.seed_scaled == seed_scaled;
}
// (v, w, p) runs variant b's plain kernels on net[*][p][b] and the plain table everywhere: coarse; fine raw (maps then come from the
// separate compositor) and fused, where the maps flavour is launch_mlp_maps
constexpr bool plain_as(int v, int w, int p, int b) {
  return is(coarse_route(v, w, p), kLaunchPlain, b, b) && is(fine_route(v, w, p, false, false), kLaunchPlain, b, b) &&
         is(fine_route(v, w, p, false, true), kLaunchPlain, b, b) && is(fine_route(v, w, p, true, false), kLaunchPlain, b, b) &&
         is(fine_route(v, w, p, true, true), kLaunchMaps, b, b, false, true);
}
constexpr bool plain_all(int v, int w, int b) { return plain_as(v, w, H, b) && plain_as(v, w, F, b) && plain_as(v, w, X, b); }
// the raw route of variants 5 to 12 in split-f16: variant 5's fine kernel on net[1][F16X3][5], with or without maps wanted
constexpr bool raw_is_fold(int v) {
  return is(fine_route(v, W, X, false, false), kLaunchFold, 5, 4, true) && is(fine_route(v, W, X, false, true), kLaunchFold, 5, 4, true);
}
// variants 0 to 4: their own kernels and networks in every arithmetic (launch_mlp runs variant 4 as variant 0 outside split-f16, on
// net[*][*][4]); netwidth 256 is variant 0 under every variant
static_assert(plain_all(0, W, 0) && plain_all(0, W2, 0), "variant 0");
static_assert(plain_all(1, W, 1) && plain_all(1, W2, 0), "variant 1");
static_assert(plain_all(2, W, 2) && plain_all(2, W2, 0), "variant 2");
static_assert(plain_all(3, W, 3) && plain_all(3, W2, 0), "variant 3");
static_assert(plain_all(4, W, 4) && plain_all(4, W2, 0), "variant 4");
// variant 5: variant 4 but for the split-f16 fine kernel, fused or raw: launch_mlp_fold on its own network and the folded table
static_assert(plain_as(5, W, H, 4) && plain_as(5, W, F, 4) && plain_all(5, W2, 0), "variant 5 outside split-f16");
static_assert(is(coarse_route(5, W, X), kLaunchPlain, 4, 4), "variant 5 coarse");
static_assert(raw_is_fold(5) && is(fine_route(5, W, X, true, false), kLaunchFold, 5, 4, true) &&
              is(fine_route(5, W, X, true, true), kLaunchFold, 5, 4, true, true), "variant 5 fine");
// variant 6: launch_mlp_half in the coarse kernel and in the fused fine kernel (plain: net[1][F16X3][6], maps: half_maps)
static_assert(plain_as(6, W, H, 4) && plain_as(6, W, F, 4) && plain_all(6, W2, 0), "variant 6 outside split-f16");
static_assert(is(coarse_route(6, W, X), kLaunchHalf, 6, 4), "variant 6 coarse");
static_assert(raw_is_fold(6) && is(fine_route(6, W, X, true, false), kLaunchHalf, 6, 4, true) &&
              is(fine_route(6, W, X, true, true), kLaunchHalf, HM, 4, true, true), "variant 6 fine");
// variant 7: launch_mlp_res in the coarse and the plain fused fine kernel; the maps flavour runs variant 6's kernel on half_maps
static_assert(plain_as(7, W, H, 4) && plain_as(7, W, F, 4) && plain_all(7, W2, 0), "variant 7 outside split-f16");
static_assert(is(coarse_route(7, W, X), kLaunchResident, 7, 4), "variant 7 coarse");
static_assert(raw_is_fold(7) && is(fine_route(7, W, X, true, false), kLaunchResident, 7, 4, true) &&
              is(fine_route(7, W, X, true, true), kLaunchHalf, HM, 4, true, true), "variant 7 fine");
// variants 8 to 11 are retired and mean variant 12: every route of theirs is the corresponding route of 12 -- coarse, fine raw and
// fused, each with and without maps, and the point queries, in all three arithmetics and at both widths
// (same_routes walks every combination of its arguments, a superset of the routes a caller forms: fused with points, or maps without
// fused, reach no entry point)
constexpr bool same(const Route& a, const Route& b) { return is(a, b.launcher, b.net, b.variant, b.fold_table, b.maps, b.seed_scaled); }
constexpr bool same_routes(int v, int u) {
  const int widths[] = {W, W2}, precs[] = {H, F, X};
  for (int w : widths)
    for (int p : precs)
      for (int points = 0; points < 2; ++points) {
        if (!same(coarse_route(v, w, p, points), coarse_route(u, w, p, points))) return false;
        for (int fused = 0; fused < 2; ++fused)
          for (int maps = 0; maps < 2; ++maps)
            if (!same(fine_route(v, w, p, fused, maps, points), fine_route(u, w, p, fused, maps, points))) return false;
      }
  return true;
}
static_assert(same_routes(8, 12), "variant 8");
static_assert(same_routes(9, 12), "variant 9");
static_assert(same_routes(10, 12), "variant 10");
static_assert(same_routes(11, 12), "variant 11");
// variant 12: variant 7 with launch_mlp_lean where variant 7 has launch_mlp_res (and the scaled table in the fine kernel); the maps
// flavour, the raw route and the point queries as under variant 7
static_assert(plain_as(12, W, H, 4) && plain_as(12, W, F, 4) && plain_all(12, W2, 0), "variant 12 outside split-f16");
static_assert(is(coarse_route(12, W, X), kLaunchLean, 7, 4), "variant 12 coarse");
static_assert(raw_is_fold(12) && is(fine_route(12, W, X, true, false), kLaunchLean, 7, 4, true, false, true) &&
              is(fine_route(12, W, X, true, true), kLaunchHalf, HM, 4, true, true), "variant 12 fine");
static_assert(is(coarse_route(12, W, X, true), kLaunchPointsHalf, 6, 4) && is(fine_route(12, W, X, false, false, true), kLaunchPointsFold, 5, 4, true),
              "variant 12 points");
static_assert(claims_tiles(kLaunchLean) && !claims_tiles(kLaunchResident), "who claims tiles");
// the coarse pass of a split-f16 render under DFN_RENDER_COARSE_F16 is the f16 route: variant 0's kernel on net[0][F16][4]
static_assert(is(coarse_route(kSelectedByDefault, W, H), kLaunchPlain, 4, 4), "f16 coarse pass");
// point queries: kPointsVariant's routes (variant 7's, whatever DFN_MLP_VARIANT says) -- split-f16 at netwidth 128 variant 6's coarse and variant 5's fine (raw) kernel
static_assert(kPointsVariant == 7 && is(coarse_route(7, W, X, true), kLaunchPointsHalf, 6, 4) &&
              is(fine_route(7, W, X, false, false, true), kLaunchPointsFold, 5, 4, true), "split-f16 points");
static_assert(is(coarse_route(7, W, H, true), kLaunchPoints, 4, 4) && is(fine_route(7, W, F, false, false, true), kLaunchPoints, 4, 4) &&
              is(coarse_route(7, W2, X, true), kLaunchPoints, 0, 0) && is(fine_route(7, W2, X, false, false, true), kLaunchPoints, 0, 0),
              "points outside split-f16 at netwidth 128");
// fused compositing: whole segments, no raw, netwidth 128, and not the 3-block f16 kernel (base variant 2)
static_assert(fused_compositing(12, W, X, 128, false) && fused_compositing(11, W, X, 128, false) && fused_compositing(10, W, X, 128, false) &&fused_compositing(9, W, X, 128, false) && fused_compositing(8, W, X, 128, false) && fused_compositing(0, W, H, 128, false) &&
              fused_compositing(2, W, X, 96, false), "fused");
static_assert(!fused_compositing(8, W, X, 128, true) && !fused_compositing(8, W, X, 40, false) && !fused_compositing(0, W, H, 96, false) &&
              !fused_compositing(2, W, H, 128, false) && !fused_compositing(0, W2, X, 128, false), "not fused");
}  // namespace route_spec

}  // namespace dfn
