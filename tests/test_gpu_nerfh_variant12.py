"""DFN_MLP_VARIANT=11 and 12: the retired variant 11 is variant 12.

Kernel variants 8 to 11 were the steps by which variant 12 was reached and are retired (nerfh_layout.h: "Kernel variants"): the numbers
stay accepted and mean 12.  This file compared variant 12 with variant 11 when the two had kernels of their own; its tests keep their
names and assertions and now check that alias end to end: every output and range flag of a process under 11 is that of a process
under 12, zero differing elements, the guard's trips included.  The cases, and the comparison of the kernels themselves with variant
7's, are tests/test_gpu_nerfh_lean.py's; the children are shared with it through tests/nerfh_lean_cases.py (one per variant and
session).
"""
import pytest

from tests import nerfh_lean_cases as lc

pytestmark = pytest.mark.gpu
A, B = 11, 12
WHAT = f"variants {A} and {B}"


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    return {v: lc.outputs(v, tmp_path_factory) for v in (A, B)}


@pytest.mark.parametrize("tag", ("a", "b", "c", "d", "n1", "n2", "n3", "l0", "l1", "h", "e", "g", "t"))
def test_variant12_is_variant11_bit_for_bit(pair, tag):
    lc.same_case(pair[A], pair[B], tag, WHAT)


def test_moved_heads_lie_on_both_sides_of_each_threshold(pair):
    lc.heads_on_both_sides(pair[A], pair[B])


def test_lindisp_reaches_the_coarse_kernel(pair):
    """cases l0 / l1 differ in the depth form alone"""
    assert not lc.torch.equal(pair[B]["l0"]["sigma"], pair[B]["l1"]["sigma"])


def test_second_run_repeats_the_first(pair):
    lc.second_run_repeats(pair[B])


@pytest.mark.parametrize("kind", ("maps", "raw", "points"))
def test_other_routes_run_variant11s_kernels(pair, kind):
    lc.same_route(pair[A], pair[B], kind, False, WHAT)


def test_guard_reads_0_without_a_trip(pair):
    assert pair[A]["guard"]["none"] == [0, 0] and pair[B]["guard"]["none"] == [0, 0]


@pytest.mark.parametrize("trip", lc.TRIPS, ids=lc.TRIP_IDS)
def test_guard_raises_the_same_flag(pair, trip):
    lc.same_trip_flag(pair[A], pair[B], trip, WHAT)
