"""GPU tests of the iso-surface extraction (dfn_isosurface_count / dfn_isosurface_emit through dfnet_amd.mesh.isosurface) on GIVEN
density volumes: no network is involved.  The checker is tests/isosurface_cases.py, a NumPy restatement of the specification in
include/dfnet_hip.h; the closed fields are also checked by invariants that do not use it.  Every shape is non-cubic, so a transposed
stride cannot pass.

Scan structure the two large cases rely on (isosurface.hip): count_kernel scans blocks of kScan = 256 nodes, scan_sums_kernel scans
the block sums in trips of kTop = 1024.
  trig_67x45x35   105 525 nodes = 412 scan blocks + a remainder of 53 nodes (more than two scan blocks plus a remainder)
  trig_67x65x63   274 365 nodes = 1071 scan blocks + a remainder: more block sums than one trip of 1024, so the carry is used"""
import ctypes

import numpy as np
import pytest
import torch

from dfnet_amd import _lib, mesh
from tests import isosurface_cases as ic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24

FIELDS = {
    "sphere": ic.sphere, "torus": ic.torus, "two_spheres": ic.two_spheres, "tilted_plane": ic.tilted_plane,
    "plane_through_nodes": ic.plane_through_nodes, "all_inside": lambda: ic.constant(1.0), "all_outside": lambda: ic.constant(0.0),
    "one_corner": ic.one_corner, "nan_nodes": ic.with_nans, "non_uniform": ic.non_uniform,
    "trig_67x45x35": lambda: ic.trig((67, 45, 35)), "trig_67x65x63": lambda: ic.trig((67, 65, 63), seed=2),
}
CLOSED = {"sphere": 2, "torus": 0, "two_spheres": 4}     # the Euler characteristic of the three closed fields
_cache = {}


def case(name):
    """(sigma, axes, iso, the restatement's result, the device result), made once per case and never modified."""
    if name not in _cache:
        sigma, axes, iso = FIELDS[name]()
        ref = ic.marching_tets(sigma, axes, iso)
        dev_axes = tuple(torch.from_numpy(a).to(DEV) for a in axes)
        got = mesh.isosurface(torch.from_numpy(sigma).to(DEV), dev_axes, iso)
        torch.cuda.synchronize()
        _cache[name] = (sigma, axes, iso, ref, got, dev_axes)
    return _cache[name]


def test_scan_sizes_are_what_the_cases_assume():
    assert 67 * 45 * 35 == 412 * 256 + 53 and 67 * 65 * 63 > 1024 * 256 + 256


@pytest.mark.parametrize("name", list(FIELDS))
def test_surface_equals_the_restatement(name):
    sigma, axes, iso, (rv, rf, _, _), (verts, faces), dev_axes = case(name)
    assert verts.dtype == torch.float32 and faces.dtype == torch.int32 and verts.is_cuda and faces.is_cuda
    assert tuple(verts.shape) == (rv.shape[0], 3) and tuple(faces.shape) == (rf.shape[0], 3), (verts.shape, faces.shape, rv.shape, rf.shape)
    v, f = verts.cpu().numpy(), faces.cpu().numpy()
    assert np.array_equal(ic.canonical_faces(f), ic.canonical_faces(rf))
    assert np.array_equal(f, rf), "faces are ordered by cell, tet, triangle, and start at the rule's first corner"
    M = max(float(np.abs(a).max()) for a in axes)
    # each of the two subtractions and the division in t, the rounding of p_b - p_a, the product and the final sum is <= 2^-24
    # relative and an edge spans at most 2 M: below 11 units of 2^-24 M, rounded up to 16
    err = float(np.abs(v.astype(np.float64) - rv).max()) if v.size else 0.0
    print(f"{name}: V {v.shape[0]} F {f.shape[0]}, worst vertex component {err:.3e} from the restatement (bound {16 * EPS * M:.3e})")
    assert err <= 16 * EPS * M
    if v.shape[0]:
        assert ic.surface_invariants(v, f)["all_used"]      # every vertex id is referenced


@pytest.mark.parametrize("name", list(FIELDS))
def test_two_runs_give_the_same_bits(name):
    sigma, axes, iso, _, (verts, faces), dev_axes = case(name)
    v2, f2 = mesh.isosurface(torch.from_numpy(sigma).to(DEV), dev_axes, iso)
    assert torch.equal(v2, verts) and torch.equal(f2, faces)


def test_quoted_counts():
    """The counts the specification was checked with on the CPU: sphere V 594 F 1184, torus V 1272 F 2544; the empty and the
    single-corner cases."""
    assert tuple(case("sphere")[4][0].shape) == (594, 3) and tuple(case("sphere")[4][1].shape) == (1184, 3)
    assert tuple(case("torus")[4][0].shape) == (1272, 3) and tuple(case("torus")[4][1].shape) == (2544, 3)
    for name in ("all_inside", "all_outside"):
        assert case(name)[4][0].shape == (0, 3) and case(name)[4][1].shape == (0, 3)
    assert case("one_corner")[4][1].shape == (6, 3) and case("one_corner")[4][0].shape == (7, 3)


@pytest.mark.parametrize("name", list(CLOSED))
def test_closed_surfaces_are_watertight_and_oriented(name):
    """Without the restatement: every directed edge once and its reverse once, V - E + F, and a positive signed volume (normals
    point toward lower density, which is outside these bodies)."""
    verts, faces = case(name)[4]
    inv = ic.surface_invariants(verts.cpu().numpy(), faces.cpu().numpy())
    print(name, inv)
    assert inv["closed"] and inv["all_used"]
    assert inv["euler"] == CLOSED[name]
    assert inv["volume"] > 0


def test_sphere_vertices_lie_near_the_sphere():
    """Linear interpolation of a quadratic with second derivative 2 along an edge no longer than the cell diagonal:
    | |p|^2 - R^2 | <= (hx^2 + hy^2 + hz^2) / 4 + 16 * 2^-24."""
    _, axes, _, _, (verts, _), _ = case("sphere")
    h2 = sum(float(a[1] - a[0]) ** 2 for a in axes)
    p = verts.cpu().numpy().astype(np.float64)
    resid = float(np.abs((p * p).sum(1) - ic.SPHERE_R ** 2).max())
    print(f"sphere: worst | |p|^2 - R^2 | {resid:.5f}, bound {h2 / 4 + 16 * EPS:.5f}")
    assert resid <= h2 / 4 + 16 * EPS


def test_tilted_plane_vertices_lie_on_the_plane():
    _, axes, _, _, (verts, _), _ = case("tilted_plane")
    M = max(float(np.abs(a).max()) for a in axes)
    p = verts.cpu().numpy().astype(np.float64)
    resid = float(np.abs(2.5 - p[:, 0] + 0.25 * p[:, 1]).max())
    print(f"tilted plane: worst residual {resid:.3e}, bound {16 * EPS * M:.3e}")
    assert p.shape[0] > 0 and resid <= 16 * EPS * M


def test_emit_bounds_its_stores_by_the_counts_it_is_given():
    """dfn_isosurface_emit with a V and F below the workspace's totals writes the leading rows and nothing behind them."""
    sigma, axes, iso, _, (verts, faces), dev_axes = case("torus")
    lib = _lib.load()
    s = torch.from_numpy(sigma).to(DEV)
    nx, ny, nz = sigma.shape
    nbytes = lib.dfn_isosurface_workspace_bytes(nx, ny, nz)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    totals = torch.zeros(2, dtype=torch.int64, device=DEV)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    _lib.check(lib.dfn_isosurface_count(P(s), nx, ny, nz, float(iso), P(ws), nbytes, P(totals), _lib.current_stream()))
    V, F = totals.tolist()
    assert (V, F) == (verts.shape[0], faces.shape[0])
    v = torch.full((V, 3), -7.0, device=DEV)
    f = torch.full((F, 3), -7, dtype=torch.int32, device=DEV)
    Vs, Fs = V // 2, F // 3
    _lib.check(lib.dfn_isosurface_emit(P(s), *(P(a) for a in dev_axes), nx, ny, nz, float(iso), P(ws), nbytes, P(v), Vs, P(f), Fs,
                                       _lib.current_stream()))
    assert torch.equal(v[:Vs], verts[:Vs]) and bool((v[Vs:] == -7.0).all())
    assert torch.equal(f[:Fs], faces[:Fs]) and bool((f[Fs:] == -7).all())
