"""Host-side checks of the mesh export (no GPU): the PLY writer and loader, default_bounds, the new option rows, and the argument
rules of the four entries of isosurface.hip, which are checked before any device work."""
import ctypes

import numpy as np
import pytest

from dfnet_amd import _lib, mesh, options
from dfnet_amd.nerfw import to8b


def tetrahedron():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32) + np.float32(0.1)
    f = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)
    c = np.array([[0., .5, 1.], [1.2, -.1, .25], [.999, .004, .5], [.3, .3, .3]], np.float32)
    return v, f, c


@pytest.mark.parametrize("colored", [False, True])
def test_ply_round_trip(tmp_path, colored):
    v, f, c = tetrahedron()
    path = str(tmp_path / "t.ply")
    mesh.save_ply(path, v, f, c if colored else None)
    head = open(path, "rb").read().split(b"end_header\n")[0].decode().split("\n")
    assert head[:2] == ["ply", "format binary_little_endian 1.0"] and "element vertex 4" in head and "element face 4" in head
    assert ("property uchar red" in head) == colored and "property list uchar int vertex_indices" in head
    v2, f2, c2 = mesh.load_ply(path)
    assert v2.dtype == np.float32 and f2.dtype == np.int32
    assert np.array_equal(v2, v) and np.array_equal(f2, f)
    if colored:
        assert np.array_equal(c2, to8b(c)) and c2.dtype == np.uint8      # the project's truncating conversion, clipped
    else:
        assert c2 is None


def test_ply_round_trip_of_an_empty_mesh(tmp_path):
    path = str(tmp_path / "e.ply")
    mesh.save_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), np.zeros((0, 3), np.float32))
    v, f, c = mesh.load_ply(path)
    assert v.shape == (0, 3) and f.shape == (0, 3) and c.shape == (0, 3)
    with pytest.raises(ValueError, match="colours"):
        mesh.save_ply(path, np.zeros((2, 3), np.float32), np.zeros((0, 3), np.int32), np.zeros((1, 3), np.float32))


def test_default_bounds():
    poses = np.zeros((3, 3, 4))
    poses[:, :3, :3] = np.eye(3)
    poses[:, :, 3] = [[0.5, -1, 2], [-0.25, 3, 1], [0.1, 0, -4]]
    want = (-0.25 - 2.5, -1 - 2.5, -4 - 2.5, 0.5 + 2.5, 3 + 2.5, 2 + 2.5)
    assert mesh.default_bounds(poses, 2.5) == want
    assert mesh.default_bounds(poses.reshape(3, 12), 2.5) == want                 # the dataloader's flat [n, 12] poses
    full = np.concatenate([poses, np.tile([[[0, 0, 0, 1.]]], (3, 1, 1))], 1)      # [n, 4, 4]
    assert mesh.default_bounds(full, 2.5) == want
    import torch
    assert mesh.default_bounds(torch.from_numpy(poses), 2.5) == want


def test_mesh_option_rows():
    ns = options.nerf_parser().parse_args([])
    assert ns.mesh_only is False and ns.mesh_grid_size == 80                      # the reference's two flags, as they were
    assert ns.mesh_bounds is None and ns.mesh_threshold == 20.0 and ns.mesh_colors is False
    ns = options.nerf_parser().parse_args(["--mesh_only", "--mesh_bounds", "-1", "-2", "-3", "1", "2.5", "3", "--mesh_threshold", "7.5",
                                           "--mesh_colors", "--mesh_grid_size", "12"])
    assert ns.mesh_only and ns.mesh_colors and ns.mesh_bounds == [-1., -2., -3., 1., 2.5, 3.] and ns.mesh_threshold == 7.5
    assert ns.mesh_grid_size == 12
    text = options.nerf_parser().format_help()
    assert "not a tuned or measured number" in " ".join(text.split())
    for parser in (options.feature_parser(), options.dm_parser()):                # the new rows are run_nerf.py's alone
        ns = parser.parse_args([])
        assert hasattr(ns, "mesh_only") and not hasattr(ns, "mesh_bounds") and not hasattr(ns, "mesh_threshold")
        assert not hasattr(ns, "mesh_colors")


def test_isosurface_entries_refuse_bad_arguments_without_a_gpu():
    """Null pointers, n < 2, the node bound and a short workspace are refused before any device work: DFN_ERR_ARG (-1) or, for the
    node bound, DFN_ERR_UNSUPPORTED (-4), with a message, on a box without a GPU too."""
    lib = _lib.load()
    one = ctypes.c_void_p(16)      # a non-null token: never dereferenced when another argument is refused first
    size = lib.dfn_isosurface_workspace_bytes
    assert size(2, 2, 2) > 0 and size(512, 512, 512) >= 512 ** 3 * 9
    assert size(2, 5, 17895697) > 0 and size(2, 5, 17895698) == 0                 # 178 956 970 nodes is the bound
    assert size(1, 4, 4) == 0 and size(4, 4, 0) == 0 and size(1024, 1024, 1024) == 0
    need = size(4, 5, 6)
    arg = [
        lib.dfn_grid_points(None, one, one, 4, 5, 6, 0, 4, one, None),
        lib.dfn_grid_points(one, one, one, 4, 5, 6, 0, 4, None, None),
        lib.dfn_grid_points(one, one, one, 4, 1, 6, 0, 4, one, None),
        lib.dfn_grid_points(one, one, one, 4, 5, 6, 3, 2, one, None),
        lib.dfn_grid_points(one, one, one, 4, 5, 6, 0, 5, one, None),
        lib.dfn_isosurface_count(None, 4, 5, 6, 0.5, one, need, one, None),
        lib.dfn_isosurface_count(one, 4, 5, 6, 0.5, None, need, one, None),
        lib.dfn_isosurface_count(one, 4, 5, 6, 0.5, one, need, None, None),
        lib.dfn_isosurface_count(one, 4, 5, 1, 0.5, one, need, one, None),
        lib.dfn_isosurface_count(one, 4, 5, 6, 0.5, one, need - 1, one, None),
        lib.dfn_isosurface_emit(None, one, one, one, 4, 5, 6, 0.5, one, need, one, 3, one, 1, None),
        lib.dfn_isosurface_emit(one, one, None, one, 4, 5, 6, 0.5, one, need, one, 3, one, 1, None),
        lib.dfn_isosurface_emit(one, one, one, one, 4, 5, 6, 0.5, None, need, one, 3, one, 1, None),
        lib.dfn_isosurface_emit(one, one, one, one, 4, 5, 6, 0.5, one, need, None, 3, one, 1, None),
        lib.dfn_isosurface_emit(one, one, one, one, 4, 5, 6, 0.5, one, need, one, 3, None, 1, None),
        lib.dfn_isosurface_emit(one, one, one, one, 0, 5, 6, 0.5, one, need, one, 3, one, 1, None),
        lib.dfn_isosurface_emit(one, one, one, one, 4, 5, 6, 0.5, one, need - 1, one, 3, one, 1, None),
        lib.dfn_isosurface_emit(one, one, one, one, 4, 5, 6, 0.5, one, need, one, -1, one, 1, None),
        lib.dfn_isosurface_emit(one, one, one, one, 4, 5, 6, 0.5, one, need, one, 3, one, 12 * 120 + 1, None),
    ]
    assert all(rc == -1 for rc in arg), arg
    assert b"dfn_isosurface_emit" in lib.dfn_last_error()
    big = 1 << 40
    unsupported = [
        lib.dfn_grid_points(one, one, one, 600, 600, 600, 0, 1, one, None),
        lib.dfn_isosurface_count(one, 600, 600, 600, 0.5, one, big, one, None),
        lib.dfn_isosurface_emit(one, one, one, one, 600, 600, 600, 0.5, one, big, one, 3, one, 1, None),
    ]
    assert all(rc == -4 for rc in unsupported), unsupported
    assert b"178956970" in lib.dfn_last_error()
    # nothing to do is not an error and launches nothing: an empty slab, an empty surface
    assert lib.dfn_grid_points(one, one, one, 4, 5, 6, 2, 2, None, None) == 0
    assert lib.dfn_isosurface_emit(one, one, one, one, 4, 5, 6, 0.5, one, need, None, 0, None, 0, None) == 0
