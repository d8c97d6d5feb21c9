"""DFN_MLP_VARIANT=10 and 11: the retired variants 10 and 11 are one set of kernels, variant 12's.

Kernel variants 8 to 11 were the steps by which variant 12 was reached and are retired (nerfh_layout.h: "Kernel variants"): the numbers
stay accepted and mean 12.  This file compared variant 11 with variant 10 when the two had kernels of their own; its tests keep their
names and assertions and now check that alias end to end: every output of a process under 11 has the bits of a process under 10, zero
differing elements, range flag 0.  The cases, and the comparison of the kernels themselves with variant 7's, are
tests/test_gpu_nerfh_lean.py's; the children are shared with it through tests/nerfh_lean_cases.py (one per variant and session).
"""
import pytest

from tests import nerfh_lean_cases as lc

pytestmark = pytest.mark.gpu
A, B = 10, 11
WHAT = f"variants {A} and {B}"


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    return {v: lc.outputs(v, tmp_path_factory) for v in (A, B)}


@pytest.mark.parametrize("tag", ("a", "b", "c", "d", "e", "g", "h", "t"))
def test_variant11_is_variant10_bit_for_bit(pair, tag):
    lc.same_case(pair[A], pair[B], tag, WHAT)


def test_moved_heads_lie_on_both_sides_of_each_threshold(pair):
    lc.heads_on_both_sides(pair[A], pair[B])


def test_per_ray_histograms_reach_the_output(pair):
    """case h is case a's rays with other embeddings"""
    assert not lc.torch.equal(pair[B]["a"]["rgb"], pair[B]["h"]["rgb"])


def test_second_run_repeats_the_first(pair):
    lc.second_run_repeats(pair[B])


@pytest.mark.parametrize("kind", ("maps", "raw", "points"))
def test_other_routes_run_variant10s_kernels(pair, kind):
    lc.same_route(pair[A], pair[B], kind, False, WHAT)
