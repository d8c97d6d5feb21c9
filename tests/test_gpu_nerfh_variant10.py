"""DFN_MLP_VARIANT=9 and 10: the retired variants 9 and 10 are one set of kernels, variant 12's.

Kernel variants 8 to 11 were the steps by which variant 12 was reached and are retired (nerfh_layout.h: "Kernel variants"): the numbers
stay accepted and mean 12.  This file compared variant 10 with variant 9 when the two had kernels of their own; its tests keep their
names and assertions and now check that alias end to end: every output of a process under 10 has the bits of a process under 9, zero
differing elements, range flag 0.  The cases, and the comparison of the kernels themselves with variant 7's, are
tests/test_gpu_nerfh_lean.py's; the children are shared with it through tests/nerfh_lean_cases.py (one per variant and session).
"""
import pytest

from tests import nerfh_lean_cases as lc

pytestmark = pytest.mark.gpu
A, B = 9, 10
WHAT = f"variants {A} and {B}"
# this file's tags -> the cases of tests/nerfh_lean_cases.py: its 24 x 32 image is e2 there, its two-pass call m1
CASE = {"e": "e2", "f": "m1"}


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    return {v: lc.outputs(v, tmp_path_factory) for v in (A, B)}


@pytest.mark.parametrize("tag", ("a", "b", "c", "d", "e", "f", "g", "h"))
def test_variant10_is_variant9_bit_for_bit(pair, tag):
    lc.same_case(pair[A], pair[B], CASE.get(tag, tag), WHAT)


def test_per_ray_histograms_reach_the_output(pair):
    """case h is case a's rays with other embeddings: were the histogram rows ignored, h would test nothing a does not"""
    assert not lc.torch.equal(pair[B]["a"]["rgb"], pair[B]["h"]["rgb"])


def test_second_run_repeats_the_first(pair):
    lc.second_run_repeats(pair[B])


@pytest.mark.parametrize("kind,per_ray", lc.OTHER)
def test_other_routes_keep_the_unscaled_table(pair, kind, per_ray):
    lc.same_route(pair[A], pair[B], kind, per_ray, WHAT)
