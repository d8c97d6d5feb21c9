"""GPU tests of the density grid (dfnet_amd.mesh.density_grid, dfn_grid_points): the grid is the existing point query on the grid's
nodes, slab by slab, so it must have the query's BITS, whatever the slab size; against the CPU oracle it sits inside the bounds of
tests/test_gpu_points.py.  Engines: that file's `scenes` fixture (netwidth 128 and 256), every precision; a 7 x 5 x 6 grid."""
import pytest
import torch

from dfnet_amd import engine as eng, mesh, nerfw
from oracle import nerfh_oracle as orc
from tests.test_gpu_points import DEV, PRECS, TOL_COARSE, TOL_FINE, relmax, scenes, wrapped  # noqa: F401  (scenes: a fixture)

pytestmark = pytest.mark.gpu
SHAPE = (7, 5, 6)
BOUNDS = (-1.2, -1.0, -0.9, 1.1, 1.3, 1.0)
_grids = {}


def axes():
    return mesh.grid_axes(BOUNDS, SHAPE, device=torch.device(DEV))


def node_points(ax):
    """[nx ny, nz, 3] from torch.meshgrid: the nodes in id order, rows of nz points."""
    X, Y, Z = torch.meshgrid(*ax, indexing="ij")
    return torch.stack([X, Y, Z], -1).reshape(SHAPE[0] * SHAPE[1], SHAPE[2], 3).contiguous()


def grid(scenes, width, prec, net):
    """density_grid of one engine, precision and network with all planes in one slab: made once, shared by the tests below."""
    key = (width, prec, net)
    if key not in _grids:
        E = scenes[width][0]
        old, E.precision = E.precision, prec
        try:
            _grids[key] = mesh.density_grid(nerfw.HipQuery(E), axes(), net=net)
        finally:
            E.precision = old
    return _grids[key]


def test_grid_axes():
    ax = axes()
    assert [a.numel() for a in ax] == list(SHAPE) and all(a.dtype == torch.float32 and a.is_cuda for a in ax)
    for a, lo, hi in zip(ax, BOUNDS[:3], BOUNDS[3:]):
        assert float(a[0]) == pytest.approx(lo) and float(a[-1]) == pytest.approx(hi) and bool((a[1:] > a[:-1]).all())
    assert [a.numel() for a in mesh.grid_axes(BOUNDS, 4, device=torch.device(DEV))] == [4, 4, 4]


@pytest.mark.parametrize("i0,i1", [(0, 7), (2, 5), (6, 7), (3, 3)])
def test_grid_points_are_the_meshgrid(i0, i1):
    ax = axes()
    got = eng.grid_points(ax, i0, i1)
    want = node_points(ax).reshape(SHAPE + (3,))[i0:i1].reshape((i1 - i0) * SHAPE[1], SHAPE[2], 3)
    assert got.shape == want.shape and torch.equal(got, want)


@pytest.mark.parametrize("width", [128, 256])
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("net", ["fine", "coarse"])
def test_grid_has_the_bits_of_the_point_query(scenes, width, prec, net, monkeypatch):
    E = scenes[width][0]
    sigma = grid(scenes, width, prec, net)
    assert tuple(sigma.shape) == SHAPE
    monkeypatch.setattr(E, "precision", prec)
    q = nerfw.HipQuery(E)
    pts = node_points(axes())
    if net == "fine":
        v = torch.tensor([[0., 0., -1.]], device=DEV).expand(pts.shape[0], 3).contiguous()
        want = q(pts, v, torch.zeros(1, 10, device=DEV), None, 'fine')[..., 3]
    else:
        want = q(pts, None, None, None, 'coarse')[..., 0]
    assert torch.equal(sigma.reshape(want.shape), want), f"{int((sigma.reshape(want.shape) != want).sum())} of {want.numel()} values differ"
    # 1 plane, 2 planes and all planes per slab
    for slab_points in (SHAPE[1] * SHAPE[2], 2 * SHAPE[1] * SHAPE[2], 1 << 20):
        assert torch.equal(mesh.density_grid(q, axes(), net=net, slab_points=slab_points), sigma), slab_points
    assert E.range_flags() == 0


@pytest.mark.parametrize("width", [128, 256])
@pytest.mark.parametrize("prec", PRECS)
def test_grid_vs_oracle(scenes, width, prec):
    E, c, f, ea, et = scenes[width]
    pts = node_points(axes()).cpu()
    rows = pts.shape[0]
    with torch.no_grad():
        ref_fine = orc.query_fine(f, ea, et, pts, torch.tensor([[0., 0., -1.]]).expand(rows, 3), torch.zeros(rows, 10))[..., 3]
        ref_coarse = orc.query_coarse_sigma(c, pts)[..., 0]
    e_fine = relmax(grid(scenes, width, prec, "fine").reshape(rows, -1), ref_fine)
    e_coarse = relmax(grid(scenes, width, prec, "coarse").reshape(rows, -1), ref_coarse)
    print(f"width {width} {prec}: fine sigma {e_fine:.2e} (bound {TOL_FINE[prec]:.0e}), coarse sigma {e_coarse:.2e} (bound {TOL_COARSE[prec]:.0e})")
    assert e_fine < TOL_FINE[prec] and e_coarse < TOL_COARSE[prec]


def test_other_widths_raise_the_point_querys_error():
    q64, _, _ = wrapped(width=64, seed=3)
    for net in ("fine", "coarse"):
        with pytest.raises(NotImplementedError, match="netwidth 64"):
            mesh.density_grid(q64, axes(), net=net)
    with pytest.raises(ValueError, match="net must be"):
        mesh.density_grid(q64, axes(), net="both")
