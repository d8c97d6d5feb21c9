"""Kernel variant 12 (the lean unit, nerfh_mlp_lean.hip) against kernel variant 7 (nerfh_mlp_res.hip), bit for bit.

Variant 12 is variant 7's split-f16 16x16x32 coarse kernel and plain fused fine kernel with per-tile work that the result does not need
taken out: tiles claimed from a device counter, the positional encoding kept for the skip concat, the fine kernel's per-ray seeds stored
at the accumulators' scale, uniform values formed at their use, one select per head value, the eight head activations evaluated as four,
point -> ray by a multiply-high and a shift, and the range guard of the ReLU conversions with one v_pk_maximum3_f16 per two pieces
(nerfh_layout.h: "Kernel variants").  Each gives the same values on the same lanes by the same arithmetic, so every output AND the range
flag must be variant 7's, the independently written kernels without any of it.  The variant is latched per process (DFN_MLP_VARIANT),
so each variant runs in a child with a time limit, and no child is started after one fails (tests/nerfh_lean_cases.py holds the
cases, the helpers and the child):

  * variant 12 against variant 7, elements that differ (each count must be 0; finite, not all zero) on coarse sigma and the fused
    route's rgb / disp / acc, split-f16 at netwidth 128, dfn_nerfh_range_status 0 after each case:
      a  64 rays at 64 + 64: fewer tiles than workgroups, nothing is ever claimed;
      b  8 calls of 257 rays at 16 + 16: ragged last tiles whose points are clamped (257 x 16 and 257 x 32 are no multiples of the
         256 points of a tile), several calls in one process;
      c  1 040 rays at 64 + 64: 260 coarse / 1 040 fine tiles on 256 workgroups, so workgroups claim second and third tiles, the
         streamed ring wraps past the resident layers and the kept operand must be the new tile's;
      d  case c a second time in the same process: the counters are zeroed again in front of every pass;
      cu  8 (CUs + 1) rays at 16 + 16, the CU count taken from the device: CUs + 1 fine tiles -- exactly one claim wins a tile, every
         other workgroup sees more == false;
      n1 n2 n3  320 rays at 3 + 29, 24 + 40 and 100 + 92: sample counts that are no powers of two (the magic number's general case);
      l0 l1  64 rays at 64 + 64 with near = 0.5, far = 2.5, lindisp off and on: both depth forms of the coarse kernel (l1's sigma must
         differ from l0's: the option reaches the kernel);
      h  case a with one histogram row per ray: ray_bias_kernel's other summation path (per-ray embeddings, two waves per ray), the
         only input on which the scaled table is formed by other code than in the shared-histogram cases;
      e  e2  the rays of a 12 x 16 and of a 24 x 32 image from raygen at 64 + 128: origins and directions differ per ray, Nf = 192 as
         in the workload;
      m1  kMaxFusedChunkRays + 64 = 65 600 rays at 16 + 16 in one call: two passes, the counters zeroed and the scaled table rewritten
         in front of each;
      m2  2 x 65 600 rays at 16 + 16 in one call: three passes;
      m3  kMaxFusedChunkRays + 64 rays at 8 + 24 in one call: two passes whatever that bound is;
      g  case a at precision f16: the route falls back to variant 4's plain kernels under either variant (nerfh_route.h);
      t  the threshold case: weights at gain 2 whose eight fine head biases are moved so that the pre-activations of the samples lie on
         both sides of 20 (softplus_hw's pass-through) and of -80 (sigmoid_hw's clamp): the shifts are found on the CPU oracle
         (threshold minus the median pre-activation per head value), and the test asserts that both sides occur for each of the eight
         head values -- these are the values that variant 12 selects and moves across lanes.  At gain 1 the transient head values of
         all samples lie within 6e-5 of each other, which is the kernels' own error at 80 and separates nothing;
    and one render_image frame at 640 x 480, 64 + 128.
  * under variant 12 the routes that it leaves with variant 7's kernels and that must still read the UNSCALED per-ray table give
    variant 7's bits on 64 rows: a maps render (rgb / disp / acc and the five maps), a `raw` render (rgb / disp / acc / raw) and a fine
    point query (raw), each with the shared and with the per-ray histogram.
  * the guard.  A hidden unit's bias is no part of the commit's weight scan (nerfh_recommit.h), so a bias of 1e9 on ONE unit of the
    last ReLU layer in front of a head saturates the hi half of that unit alone and nothing downstream is converted again: the flag
    must read 2 (DFN_RANGE_F16X3) under variants 7 and 12 alike, and 0 without the trip.  Row 16 ms + 4 g + r of an M-block is
    accumulator register 8 ms + 4 nb + r of lane group g (nerfh_layout.h), i.e. conversion piece i = 4 ms + 2 nb + (r >> 1) and half
    r & 1 of its packed word (nerfh_mlp_core.h: X3Piece, x3_chunk / x3_pos), so units r = 0, 1, 2, 3 cover
        r = 0: even piece, low half     r = 1: even piece, high half     r = 2: odd piece, low half     r = 3: odd piece, high half
    -- an even piece's hi word is the one variant 12 holds for the odd piece's v_pk_maximum3_f16.  Tripped in the coarse kernel
    (xyz_encoding_8, unit r of M-block 0: converted inside layer 8; unit 96 + r of M-block 3: carried into static_sigma, where pieces
    2 and 3 lie in different chunks) and in the fine kernel (transient_encoding.6, unit r: converted inside the layer; unit 48 + r:
    pieces 4..7 of the carried-in M-block, the block form behind the transient head's first chunk).
  * DFN_MLP_VARIANT=9, a retired number, on case a gives variant 12's bits: 8 to 11 mean 12 (nerfh_layout.h: kVariantFacts).

This file is also the child of its own tests: python tests/test_gpu_nerfh_lean.py <out.pt> [tag ...] (no tag: everything).
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import nerfh_lean_cases as lc  # noqa: E402

if __name__ == "__main__":
    lc.child(sys.argv[1], sys.argv[2:])
    sys.exit(0)

pytestmark = pytest.mark.gpu
WHAT = "variants 7 and 12"


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    """The child's outputs under variants 7 and 12."""
    return {v: lc.outputs(v, tmp_path_factory) for v in (7, 12)}


@pytest.mark.parametrize("tag", lc.TAGS)
def test_variant12_is_variant7_bit_for_bit(pair, tag):
    lc.same_case(pair[7], pair[12], tag, WHAT)


def test_frame_variant12_is_variant7(pair):
    a, b = pair[7]["frame"], pair[12]["frame"]
    lc.same_bits(a, b, ("rgb", "disp", "acc"), WHAT)
    assert tuple(a["rgb"].shape) == (480, 640, 3) and float(a["acc"].max()) > 0


def test_moved_heads_lie_on_both_sides_of_each_threshold(pair):
    lc.heads_on_both_sides(pair[7], pair[12])


def test_lindisp_reaches_the_coarse_kernel(pair):
    """cases l0 / l1 differ in the depth form alone"""
    assert not lc.torch.equal(pair[12]["l0"]["sigma"], pair[12]["l1"]["sigma"])


def test_per_ray_histograms_reach_the_output(pair):
    """case h is case a's rays with other embeddings: were the histogram rows ignored, h would test nothing a does not"""
    assert not lc.torch.equal(pair[12]["a"]["rgb"], pair[12]["h"]["rgb"])


def test_second_run_repeats_the_first(pair):
    lc.second_run_repeats(pair[12])


@pytest.mark.parametrize("kind,per_ray", lc.OTHER)
def test_other_routes_run_variant7s_kernels_on_the_unscaled_table(pair, kind, per_ray):
    lc.same_route(pair[7], pair[12], kind, per_ray, WHAT)


def test_trip_positions_cover_both_pieces_and_both_halves():
    """no GPU work: the four positions per (network, path), from the lane map"""
    for base, mb in ((0, 0), (96, 3), (48, 1)):
        seen = set()
        for r in range(4):
            m, pieces, half = lc.piece_and_half(base + r)
            assert m == mb and pieces[0] % 2 == pieces[1] % 2
            seen.add((pieces[0] % 2, half))
        assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert lc.piece_and_half(98)[1] == (1, 3) and lc.piece_and_half(50)[1] == (5, 7) and lc.piece_and_half(2)[1] == (1, 3) and lc.piece_and_half(0)[1] == (0, 2)


def test_guard_reads_0_without_a_trip(pair):
    assert pair[7]["guard"]["none"] == [0, 0] and pair[12]["guard"]["none"] == [0, 0]


@pytest.mark.parametrize("trip", lc.TRIPS, ids=lc.TRIP_IDS)
def test_guard_raises_the_same_flag(pair, trip):
    lc.same_trip_flag(pair[7], pair[12], trip, WHAT)


@pytest.mark.parametrize("retired", (9,))
def test_retired_number_means_variant12(pair, tmp_path, retired):
    """one more child, started only behind the pair's two: case a under a retired DFN_MLP_VARIANT"""
    path = str(tmp_path / f"v{retired}.pt")
    lc.run_child(retired, path, "a")
    lc.same_bits(lc.torch.load(path)["a"], pair[12]["a"], lc.KEYS, f"variants {retired} and 12")
