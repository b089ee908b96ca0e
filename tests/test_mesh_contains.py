"""Point-in-mesh for large meshes, on the host: the specification meshing.mesh_contains (the reference's check_mesh_contains with
its TriangleHash restated as a predicate) against fixture F10, the brute-force oracle and a scalar restatement of the hash; the
strictness of the rule, degenerate inputs, argument checks, the byte queries, and geometry.voxelize / geometry.mesh_iou on CPU
tensors.  The kernels are held to the specification in test_mesh_contains_gpu.py."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import golden
from oracle.mesh_oracle import check_mesh_contains_np
from test_geometry_metrics import icosphere

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("arah_contains_index_bytes", "arah_contains_index_count", "arah_contains_index_fill", "arah_mesh_contains",
               "arah_mesh_contains_grid")


def f10():
    d = golden("f10_mesh_contains.npz")
    return (torch.from_numpy(np.asarray(d["verts"])), torch.from_numpy(np.asarray(d["faces"])), torch.from_numpy(np.asarray(d["points"])),
            np.asarray(d["contains"]))


def indexed(tris):
    """An (F,3,3) soup as (verts float32, faces int32) tensors, three vertices a face."""
    verts = torch.from_numpy(np.ascontiguousarray(tris, np.float32).reshape(-1, 3))
    return verts, torch.arange(verts.shape[0], dtype=torch.int32).reshape(-1, 3)


def cube(side=1.0):
    """The 12-triangle cube [0, side]^3; both caps (z = 0, z = side) are split along the diagonal x = y."""
    v = np.array([(x, y, z) for z in (0, 1) for y in (0, 1) for x in (0, 1)], np.float32) * np.float32(side)
    f = np.array([(0, 3, 1), (0, 2, 3), (4, 5, 7), (4, 7, 6), (0, 1, 5), (0, 5, 4), (2, 7, 3), (2, 6, 7), (0, 4, 6), (0, 6, 2),
                  (1, 3, 7), (1, 7, 5)], np.int32)
    return torch.from_numpy(v), torch.from_numpy(f)


def hash_restated(verts, faces, points, resolution):
    """triangle_hash.pyx as a dict of lists, scalar Python: -> the number of candidates per point."""
    V, F, P = np.asarray(verts, np.float64), np.asarray(faces), np.asarray(points, np.float64)
    tri = V[F]
    lo, hi = tri.reshape(-1, 3).min(0), tri.reshape(-1, 3).max(0)
    scale = (resolution - 1) / (hi - lo)
    translate = 0.5 - scale * lo
    T, Q = scale * tri + translate, scale * P + translate
    cells = {}
    for t in range(len(T)):
        mn = [min(max(int(min(T[t, 0, j], T[t, 1, j], T[t, 2, j])), 0), resolution - 1) for j in range(2)]
        mx = [min(max(int(max(T[t, 0, j], T[t, 1, j], T[t, 2, j])), 0), resolution - 1) for j in range(2)]
        for x in range(mn[0], mx[0] + 1):
            for y in range(mn[1], mx[1] + 1):
                cells.setdefault(resolution * x + y, []).append(t)
    tested = np.zeros(len(Q), np.int64)
    for i in range(len(Q)):
        if not (np.isfinite(Q[i, 0]) and np.isfinite(Q[i, 1])) or max(abs(Q[i, 0]), abs(Q[i, 1])) > 1e9:
            continue
        x, y = int(Q[i, 0]), int(Q[i, 1])
        if 0 <= x < resolution and 0 <= y < resolution:
            tested[i] = len(cells.get(resolution * x + y, []))
    return tested


# ------------------------------------------------------------------------------------------ 1. fixture F10
@pytest.mark.parametrize("resolution,n_ambiguous,max_tested", [(512, 2, 21), (64, 1, 37), (8, 0, 396), (2, 0, 1554)])
def test_specification_equals_the_fixture_and_the_oracle(resolution, n_ambiguous, max_tested):
    """Measured on the host: 1 075 inside at every resolution; ambiguous 2 / 1 / 0 / 0 (the one at 64 is a query point that IS a
    vertex of the mesh: u + v misses |detA| by one unit in the last place); mean and maximum candidates a point 2.19 / 21 at 512,
    1 372 / 1 554 at 2."""
    from arah_release_amd import meshing
    verts, faces, points, contains = f10()
    assert faces.shape[0] == 5172 and points.shape[0] == 8256 and points.dtype == torch.float64
    inside, ambiguous, tested = meshing.mesh_contains(verts, faces, points, resolution)
    print("resolution %d: inside %d ambiguous %d tested mean %.2f max %d" % (resolution, int(inside.sum()), int(ambiguous.sum()),
                                                                              float(tested.double().mean()), int(tested.max())))
    assert inside.dtype == torch.bool and ambiguous.dtype == torch.bool and tested.dtype == torch.int32
    oracle = check_mesh_contains_np(verts.numpy(), faces.numpy(), points.numpy(), resolution)
    assert np.array_equal(inside.numpy(), oracle)
    assert int(inside.sum()) == 1075
    if resolution == 512:
        assert np.array_equal(inside.numpy(), contains)
    assert int(ambiguous.sum()) == n_ambiguous and int(tested.max()) == max_tested
    assert not bool((ambiguous & inside).any())
    # the result does not depend on the chunking
    again = meshing.mesh_contains(verts[:, :], faces, points[:700], resolution, chunk_pairs=1 << 16)
    assert all(torch.equal(a, b[:700]) for a, b in zip(again, (inside, ambiguous, tested)))


# ------------------------------------------------------------------------------------------ 2. tested
def test_tested_equals_the_restated_hash():
    from arah_release_amd import meshing
    verts, faces = indexed(icosphere(1))
    rng = np.random.default_rng(5)
    points = rng.uniform(-1.3, 1.3, (600, 3))
    points[:5] = [(np.nan, 0, 0), (0, np.inf, 0), (0, 0, np.nan), (-1e30, 0, 0), (0.2, 0.1, 7.0)]
    points = torch.from_numpy(points)
    for resolution in (2, 8, 33):
        _, _, tested = meshing.mesh_contains(verts, faces, points, resolution)
        want = hash_restated(verts.numpy(), faces.numpy(), points.numpy(), resolution)
        assert np.array_equal(tested.numpy(), want), resolution
        assert want[:4].tolist() == [0, 0, want[2], 0] and want[4] > 0   # a cell is a matter of x and y alone


# ------------------------------------------------------------------------------------------ 3. an exact bracket
def test_icosphere_bracket_without_tolerance():
    from arah_release_amd import meshing
    tris = icosphere(2)
    assert tris.shape[0] == 320
    t64 = tris.astype(np.float64)
    n = np.cross(t64[:, 1] - t64[:, 0], t64[:, 2] - t64[:, 0])
    inscribed = float(np.abs((n * t64[:, 0]).sum(1) / np.linalg.norm(n, axis=1)).min())
    assert 0.98 < inscribed < 0.9823          # 0.9822: every point nearer the centre is inside the polyhedron
    verts, faces = indexed(tris)
    gen = torch.Generator().manual_seed(0)
    points = (torch.rand(20000, 3, generator=gen, dtype=torch.float64) * 2.2 - 1.1)
    inside, ambiguous, _ = meshing.mesh_contains(verts, faces, points, 512)
    r = points.norm(dim=1)
    assert bool(inside[r < 0.98].all()) and int((r < 0.98).sum()) > 5000
    assert not bool(inside[r > 1.0].any()) and int((r > 1.0).sum()) > 5000
    assert not bool(ambiguous.any())


# ------------------------------------------------------------------------------------------ 4. the strictness, pinned
def test_strictness_on_the_cube():
    """The centre's column passes through the diagonals of both caps, where u + v == |detA| or a coordinate is 0: no crossing is
    counted and the centre of the cube is answered OUTSIDE, as the reference answers it.  A point off the diagonal is inside."""
    from arah_release_amd import meshing
    verts, faces = cube()
    points = torch.tensor([[0.5, 0.5, 0.5], [0.5, 0.25, 0.5], [0.5 + 2.0 ** -20, 0.5, 0.5], [0.25, 0.25, 0.75]], dtype=torch.float64)
    for resolution in (512, 8):
        inside, ambiguous, tested = meshing.mesh_contains(verts, faces, points, resolution)
        oracle = check_mesh_contains_np(verts.numpy(), faces.numpy(), points.numpy(), resolution)
        print("cube at %d:" % resolution, inside.tolist(), ambiguous.tolist(), tested.tolist(), oracle.tolist())
        assert inside.tolist() == oracle.tolist()
        assert inside.tolist() == [False, True, True, False]
        assert not bool(ambiguous.any()) and int(tested.min()) >= 2


# ------------------------------------------------------------------------------------------ 5. degenerate inputs
def test_degenerate_points_and_meshes():
    from arah_release_amd import meshing
    verts, faces = cube(511.0)                      # at resolution 512: scale 1, translate 0.5, q = x + 0.5 exactly
    nan = float("nan")
    points = torch.tensor([[255.0, 100.0, 30.0],     # inside
                           [nan, 100.0, 30.0], [255.0, nan, 30.0], [255.0, 100.0, nan],
                           [-0.75, 100.0, 30.0], [255.0, 600.0, 30.0], [255.0, 100.0, -0.75],        # outside the box
                           [-0.25, 100.0, 30.0],     # q.x = 0.25: in the box, cell 0, outside the mesh
                           [511.25, 100.0, 30.0],    # q.x = 511.75 in (resolution - 0.5, resolution): cell 511
                           [511.5, 100.0, 30.0],     # q.x = resolution itself: in the box, no cell
                           [255.0, 511.5, 30.0], [255.0, 100.0, 511.5]], dtype=torch.float64)
    inside, ambiguous, tested = meshing.mesh_contains(verts, faces, points, 512)
    assert inside.tolist() == [True] + [False] * 11
    assert not bool(ambiguous.any())
    # the four cap triangles' rectangles cover every cell; a cell is a matter of x and y alone, so a NaN z still has its own
    assert tested[0] == 4 and tested[1] == 0 and tested[2] == 0 and tested[3] == 4 and tested[6] == 4 and tested[11] == 4
    assert tested[4] > 4 and tested[5] == 0                 # (int)(-0.25) is cell 0, beside the wall x = 0; q.y = 600.5 has no cell
    assert tested[7] > 4 and tested[8] > 4 and tested[9] == 0 and tested[10] == 0
    assert np.array_equal(tested.numpy(), hash_restated(verts.numpy(), faces.numpy(), points.numpy(), 512))
    assert np.array_equal(inside.numpy(), check_mesh_contains_np(verts.numpy(), faces.numpy(), points.numpy(), 512))
    # float32 points are their float64 values
    p32 = torch.tensor([[255.1, 100.3, 30.7], [0.1, 0.2, 510.9], [600.0, 1.0, 1.0], [nan, 1.0, 1.0]], dtype=torch.float32)
    assert all(torch.equal(a, b) for a, b in zip(meshing.mesh_contains(verts, faces, p32, 64),
                                                 meshing.mesh_contains(verts, faces, p32.double(), 64)))
    # degenerate meshes: every point outside, nothing ambiguous, nothing tested
    flat = verts.clone()
    flat[:, 2] = 3.0
    poisoned = torch.cat([verts, torch.tensor([[nan, 0.0, 0.0]])])
    used_nan, unused_nan = faces.clone(), faces
    used_nan[0, 0] = 8
    out_of_range = faces.clone()
    out_of_range[3, 1] = 8
    for v, f in ((verts, faces[:0]), (flat, faces), (poisoned, used_nan), (verts, out_of_range), (verts[:0], faces[:0])):
        i, a, t = meshing.mesh_contains(v, f, points, 512)
        assert not bool(i.any()) and not bool(a.any()) and int(t.abs().sum()) == 0 and i.shape == (12,)
    # a NaN vertex no face uses does not matter; no points is legal
    assert torch.equal(meshing.mesh_contains(poisoned, unused_nan, points, 512)[0], inside)
    assert [x.shape for x in meshing.mesh_contains(verts, faces, points[:0], 512)] == [(0,)] * 3


# ------------------------------------------------------------------------------------------ 6. host-side logic
def test_argument_errors():
    from arah_release_amd import geometry, meshing
    verts, faces = cube()
    pts = torch.zeros(4, 3)
    for bad in (1, 4097, 0, -3, 512.0, True, "512"):
        with pytest.raises(ValueError):
            meshing.mesh_contains(verts, faces, pts, bad)
    for res in (2, 4096):
        meshing.check_contains_args(verts, faces, pts, res)
    with pytest.raises(ValueError):
        meshing.mesh_contains(verts, faces.float(), pts)
    with pytest.raises(ValueError):
        meshing.mesh_contains(verts.long(), faces, pts)
    with pytest.raises(ValueError):
        meshing.mesh_contains(verts, faces, pts.half())
    with pytest.raises(ValueError):
        meshing.mesh_contains(verts, faces, pts[:, :2])
    with pytest.raises(ValueError):
        meshing.mesh_contains(verts[:, :2], faces, pts)
    with pytest.raises(ValueError):
        geometry.mesh_contains((verts, faces, faces), pts)
    with pytest.raises(ValueError):
        geometry.mesh_contains(torch.zeros(3, 3), pts)
    with pytest.raises(ValueError):
        geometry.voxelize((verts, faces))                                  # neither dims nor resolution
    with pytest.raises(ValueError):
        geometry.voxelize((verts, faces), dims=4, resolution=4)
    with pytest.raises(ValueError):
        geometry.voxelize((verts, faces), dims=(4, 0, 4))
    with pytest.raises(ValueError):
        geometry.voxelize((verts, faces), dims=4, padding=-1.0)
    with pytest.raises(ValueError):
        geometry.voxelize((verts, faces), dims=4, bounds=((0, 0, 0), (1, -1, 1)))
    with pytest.raises(ValueError):
        geometry.mesh_iou((verts, faces), (verts, faces), n_points=0)
    with pytest.raises(ValueError):
        geometry.mesh_iou((verts, faces), (verts, faces), resolution=1)
    with pytest.raises(ValueError):
        geometry.mesh_contains((verts, faces), pts, index=object())


def test_symbols_and_byte_queries():
    import __graft_entry__ as g
    g.build()
    from arah_release_amd import hip
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "arah_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(arah_[a-z0-9_]+)\s*\(", header))
    lib = hip.load_library()
    for name in NEW_EXPORTS:
        assert name in declared and name in hip.EXPORTS and hasattr(lib, name), name
    size = lib.arah_contains_index_bytes
    for n_faces, resolution in ((-1, 512), (1, 1), (1, 4097), (1, 0), ((1 << 28) + 1, 512), (1, -512)):
        assert size(n_faces, resolution) == 0, (n_faces, resolution)
    cells = 512 * 512
    assert size(0, 2) > 0 and size(0, 2) % 256 == 0
    # a header, 16 doubles + a rectangle + two list slots per face, a count and a start per cell
    assert size(98000, 512) >= 256 + 98000 * (16 * 8 + 16 + 8) + 8 * cells
    assert size(98000, 512) < 256 + 98000 * (16 * 8 + 16 + 8) + 8 * cells + 8 * cells // 2048 + 16 * 256
    assert size(1 << 28, 4096) > size(98000, 4096) > size(98000, 512) > size(1, 512) > size(1, 2)


def test_voxelize_and_iou_on_the_host():
    from arah_release_amd import geometry, meshing
    tris = icosphere(2)
    verts, faces = indexed(tris)
    # bounds that are not symmetric: a lattice column in a coordinate plane of the icosphere runs along its edges (the strictness)
    default = geometry.voxelize((verts, faces), dims=2)["bounds"]
    assert default == (tuple(verts.numpy().min(0).astype(np.float64)), tuple(verts.numpy().max(0).astype(np.float64)))
    vox = geometry.voxelize((verts, faces), dims=(9, 8, 7), bounds=((-1.0, -1.125, -1.25), (1.125, 1.0, 1.0)), padding=0.125)
    occ = vox["occupancy"]
    assert occ.shape == (9, 8, 7) and occ.dtype == torch.bool and int(vox["ambiguous"]) == 0
    lo, hi = vox["bounds"]
    assert lo == (-1.125, -1.25, -1.375) and hi == (1.25, 1.125, 1.125)
    assert vox["xs"].dtype == torch.float32 and vox["xs"].shape == (9,)
    assert float(vox["xs"][0]) == np.float32(lo[0] + 0.5 * (hi[0] - lo[0]) / 9)
    grid = torch.stack(torch.meshgrid(vox["xs"], vox["ys"], vox["zs"], indexing="ij"), -1).reshape(-1, 3)
    assert torch.equal(occ.reshape(-1), meshing.mesh_contains(verts, faces, grid, 512)[0])
    r = grid.double().norm(dim=1)
    assert bool(occ.reshape(-1)[r < 0.98].all()) and not bool(occ.reshape(-1)[r > 1.0].any()) and int(occ.sum()) > 0
    # the soup form, cubic cells, bounds given
    cubic = geometry.voxelize(tris_t := torch.from_numpy(tris), resolution=6, bounds=((-1.5, -1, -1), (1.5, 1, 1)))
    assert cubic["occupancy"].shape == (6, 4, 4) and cubic["bounds"] == ((-1.5, -1.0, -1.0), (1.5, 1.0, 1.0))

    same = geometry.mesh_iou((verts, faces), tris_t, n_points=5000, seed=3)
    assert float(same["iou"]) == 1.0 and int(same["n_a"]) == int(same["n_b"]) == int(same["n_both"]) == int(same["n_either"]) > 0
    assert same["n_points"] == 5000 and int(same["ambiguous_a"]) == 0
    box = float(np.prod(verts.numpy().max(0).astype(np.float64) - verts.numpy().min(0).astype(np.float64)))
    assert float(same["volume_a"]) == int(same["n_a"]) / 5000 * box
    assert abs(float(same["volume_a"]) - 4.19 * 0.97) < 0.25                 # a little less than the ball's 4 pi / 3
    away = torch.from_numpy(icosphere(2, centre=(2.5, 0.0, 0.0)))
    apart = geometry.mesh_iou((verts, faces), away, n_points=5000, seed=3)
    assert float(apart["iou"]) == 0.0 and int(apart["n_both"]) == 0 and int(apart["n_a"]) > 0 and int(apart["n_b"]) > 0
    assert int(apart["n_either"]) == int(apart["n_a"]) + int(apart["n_b"])
    half = geometry.mesh_iou((verts, faces), torch.from_numpy(icosphere(2, centre=(0.5, 0.0, 0.0))), n_points=5000, seed=3,
                             return_points=True)
    assert int(half["n_either"]) == int(half["n_a"]) + int(half["n_b"]) - int(half["n_both"]) and 0.0 < float(half["iou"]) < 1.0
    assert float(half["iou"]) == int(half["n_both"]) / int(half["n_either"])
    assert torch.equal(half["inside_a"], meshing.mesh_contains(verts, faces, half["points"], 512)[0])
    again = geometry.mesh_iou((verts, faces), torch.from_numpy(icosphere(2, centre=(0.5, 0.0, 0.0))), n_points=5000, seed=3)
    assert all(torch.equal(torch.as_tensor(again[k]), torch.as_tensor(half[k])) for k in geometry.IOU_KEYS)
    # no point in either: NaN
    nowhere = geometry.mesh_iou((verts, faces), tris_t, n_points=100, bounds=((3, 3, 3), (4, 4, 4)))
    assert int(nowhere["n_either"]) == 0 and float(nowhere["iou"]) != float(nowhere["iou"])
