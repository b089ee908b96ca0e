"""Generalized winding numbers, the specification on the host (DESIGN.md "Winding numbers on the device"): meshing.winding_tree /
meshing.mesh_winding against an independent restatement of the brute-force sum, the classification of fixture F10 (libmesh's
check_mesh_contains answers for 8 256 points), the error of the dipole approximation, meshes that are not watertight, the smallest
shapes, and the argument errors of geometry.* with rule="winding"."""
import math
import os
import re

import numpy as np
import pytest
import torch

from test_geometry_metrics import icosphere
from test_mesh_contains import cube, f10, indexed

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
NEW_EXPORTS = ("arah_winding_index_bytes", "arah_winding_index_count", "arah_winding_index_fill", "arah_mesh_winding",
               "arah_mesh_winding_grid")
# per exactly summed triangle: a term moves w = sum / (4 pi) by at most 1/2, and 2^-48 allows 16 ulp of that to two atan2s
TERM_BOUND = 2.0 ** -48

_CACHE = {}


def _f10():
    """F10 with float32 vertices and points, its trees and winding numbers by (depth, accuracy), each computed once."""
    if "mesh" not in _CACHE:
        verts, faces, points, contains = f10()
        _CACHE["mesh"] = (verts.to(torch.float32), faces, points.to(torch.float32), torch.from_numpy(np.asarray(contains)).bool())
    return _CACHE["mesh"]


def _f10_tree(depth):
    from arah_release_amd import meshing
    if ("tree", depth) not in _CACHE:
        verts, faces, _, _ = _f10()
        _CACHE["tree", depth] = meshing.winding_tree(verts, faces, depth)
    return _CACHE["tree", depth]


def _f10_winding(depth, accuracy):
    from arah_release_amd import meshing
    if ("w", depth, accuracy) not in _CACHE:
        _CACHE["w", depth, accuracy] = meshing.mesh_winding(_f10_tree(depth), _f10()[2], accuracy)
    return _CACHE["w", depth, accuracy]


def brute_force(verts, faces, points, chunk=64):
    """The generalized winding number restated in numpy: Van Oosterom & Strackee per (point, face), summed in face order."""
    V, P = np.asarray(verts, np.float64), np.asarray(points, np.float64)
    tri = V[np.asarray(faces, np.int64)]
    px, py, pz = (np.ascontiguousarray(P[:, k])[:, None] for k in range(3))
    total = np.zeros(len(P))
    for f0 in range(0, len(tri), chunk):
        t = tri[f0:f0 + chunk]
        (ax, ay, az), (bx, by, bz), (cx, cy, cz) = (((t[None, :, k, 0] - px), (t[None, :, k, 1] - py), (t[None, :, k, 2] - pz))
                                                    for k in range(3))
        num = ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz) + az * (bx * cy - by * cx)
        la, lb, lc = np.sqrt(ax * ax + ay * ay + az * az), np.sqrt(bx * bx + by * by + bz * bz), np.sqrt(cx * cx + cy * cy + cz * cz)
        den = la * lb * lc + (ax * bx + ay * by + az * bz) * lc + (bx * cx + by * cy + bz * cz) * la + (cx * ax + cy * ay + cz * az) * lb
        terms = np.where(num == 0, 0.0, 2.0 * np.arctan2(num, den))
        for j in range(terms.shape[1]):
            total = total + terms[:, j]
    return total / (4.0 * math.pi)


def signed_volume(verts, faces):
    t = np.asarray(verts, np.float64)[np.asarray(faces, np.int64)]
    return float(np.einsum("fk,fk->f", t[:, 0], np.cross(t[:, 1], t[:, 2])).sum() / 6.0)


def test_exact_rule_against_an_independent_restatement():
    verts, faces, points, _ = _f10()
    F = int(faces.shape[0])
    want = brute_force(verts.numpy(), faces.numpy(), points.numpy())
    w0, n_exact, n_far = _f10_winding(0, INF)
    assert w0.dtype == torch.float64 and n_exact.dtype == torch.int32 and n_far.dtype == torch.int32
    tree = _f10_tree(0)
    assert tree.n_nodes == 1 and torch.equal(tree.order, torch.arange(F, dtype=torch.int32))     # the root is the leaf: face order
    d0 = float(np.abs(w0.numpy() - want).max())
    d3 = float(np.abs(_f10_winding(3, INF)[0].numpy() - want).max())
    print("F10, accuracy inf against the numpy restatement: max |dw| %.3g at depth 0, %.3g at depth 3; bound %.3g" % (d0, d3, F * TERM_BOUND))
    assert d0 <= F * TERM_BOUND
    assert d3 <= 2 * F * TERM_BOUND           # another order of the same terms


def test_orientation_and_classification_on_f10():
    from arah_release_amd import meshing
    verts, faces, points, contains = _f10()
    tree = _f10_tree(3)
    assert tree.orient == -1 and signed_volume(verts.numpy(), faces.numpy()) < 0
    for v, f in (cube(), indexed(icosphere(2))):
        want = -1 if signed_volume(v.numpy(), f.numpy()) < 0 else 1
        assert meshing.winding_tree(v, f).orient == want == meshing.winding_orient(v, f)[0]
    flipped = meshing.winding_tree(*((lambda v, f: (v, f[:, [0, 2, 1]]))(*cube())))
    assert flipped.orient == -meshing.winding_tree(*cube()).orient
    w = _f10_winding(3, INF)[0]
    inside = meshing.winding_inside(w, tree.orient)
    decided = (tree.orient * w - 0.5).abs() > 0.1
    excluded = int((~decided).sum())
    print("F10: %d of %d points within 0.1 of the threshold" % (excluded, len(w)))
    assert excluded <= 0.01 * len(w)
    assert torch.equal(inside[decided], contains[decided])


def test_approximation_error_on_f10():
    from arah_release_amd import meshing
    verts, faces, points, _ = _f10()
    F = int(faces.shape[0])
    for depth in (2, 4):
        tree = _f10_tree(depth)
        exact, n_exact, n_far = _f10_winding(depth, INF)
        assert bool((n_exact == F).all()) and bool((n_far == 0).all())
        errs = {}
        for accuracy in (2.0, 3.0):
            w, n_exact, n_far = _f10_winding(depth, accuracy)
            errs[accuracy] = float((w - exact).abs().max())
            print("F10 depth %d accuracy %g: max |w - w(inf)| = %.4f, mean n_exact %.1f, n_far %.1f"
                  % (depth, accuracy, errs[accuracy], float(n_exact.double().mean()), float(n_far.double().mean())))
            assert bool(((n_exact + n_far) >= 1).all()) and bool((n_exact <= F).all())
            sure = (tree.orient * exact - 0.5).abs() > 2.0 * errs[accuracy]
            assert int((~sure).sum()) <= 0.01 * len(w)
            assert torch.equal(meshing.winding_inside(w, tree.orient)[sure], meshing.winding_inside(exact, tree.orient)[sure])
        assert errs[3.0] <= errs[2.0]
        # 100 diagonals away the root itself is far
        diag = float((verts.double().amax(0) - verts.double().amin(0)).norm())
        away = (verts.double().mean(0) + torch.tensor([60.0, 60.0, 52.0], dtype=torch.float64) * diag).to(torch.float32)[None]
        w, n_exact, n_far = meshing.mesh_winding(tree, away, 3.0)
        assert int(n_exact) == 0 and int(n_far) == 1 and abs(float(w)) < 1e-4


def _holed(verts, faces, n_hole=316):
    """F10 without the n_hole faces whose centroids lie closest to the centroid of face 0: one hole."""
    cen = verts.double()[faces.long()].mean(1)
    d = (cen - cen[0]).norm(dim=1)
    keep = torch.ones(faces.shape[0], dtype=torch.bool)
    keep[torch.argsort(d, stable=True)[:n_hole]] = False
    return faces[keep]


def test_open_meshes_classify_like_the_closed_mesh():
    from arah_release_amd import geometry
    verts, faces, points, contains = _f10()
    thirds = faces[torch.arange(faces.shape[0]) % 3 != 0]                 # f10_open of test_mesh_sdf_gpu: every third face removed
    holed = _holed(verts, faces)
    assert holed.shape[0] == faces.shape[0] - 316
    for name, open_faces in (("every third face removed", thirds), ("a 316-face hole", holed)):
        inside, ambiguous = geometry.mesh_contains((verts, open_faces), points, rule="winding", return_ambiguous=True)
        assert inside.dtype == torch.bool and inside.shape == ambiguous.shape and not bool(ambiguous.any())
        agree = float((inside == contains).double().mean())
        print("F10 with %s, rule='winding': agrees with the closed mesh's contains on %.4f of the points" % (name, agree))
        assert agree >= 0.99
        w = geometry.winding_number((verts, open_faces), points)
        assert torch.equal(inside, (-1.0 * w) >= 0.5)                      # F10's faces are clockwise seen from outside


def test_smallest_shapes():
    from arah_release_amd import geometry, meshing
    f32 = torch.float32
    # F = 0: w = 0, nothing inside
    tree = meshing.winding_tree(torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32))
    w, n_exact, n_far = meshing.mesh_winding(tree, torch.rand(5, 3), 3.0)
    assert tree.n_nodes == 0 and bool((w == 0).all()) and not bool(n_exact.any()) and not bool(n_far.any())
    assert not bool(geometry.mesh_contains((torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32)), torch.rand(5, 3), rule="winding").any())
    # F = 1: the triangle on the three axes is seen from the origin, a point of its axis, under an octant: w = 1/8; from the origin's
    # mirror image under the same angle from the other side; from a corner, an edge and its plane under none
    tri = (torch.eye(3, dtype=f32), torch.tensor([[0, 1, 2]], dtype=torch.int32))
    pts = torch.tensor([[0, 0, 0], [2 / 3, 2 / 3, 2 / 3], [1, 0, 0], [0.5, 0.5, 0], [2, -1, 0]], dtype=torch.float64)
    w = geometry.winding_number(tri, pts, accuracy=INF)
    assert abs(float(w[0]) - 0.125) <= TERM_BOUND and abs(float(w[1]) + 0.125) <= 1e-7     # the mirror image is rounded to float32
    assert bool((w[2:] == 0).all())
    # the cube: a corner sees an octant of it, the middle of an edge a quarter, a point in a face's plane beside it nothing
    cv, cf = cube()
    P = torch.tensor([[0, 0, 0], [0.5, 0, 0], [2, 0.5, 0], [0.5, 0.5, 0.5], [0.25, 0.5, 0.125]], dtype=f32)
    orient = meshing.winding_tree(cv, cf).orient
    for depth in (0, 1, meshing.WINDING_MAX_DEPTH):
        w = orient * geometry.winding_number((cv, cf), P, accuracy=INF, depth=depth)
        assert bool((w - torch.tensor([0.125, 0.25, 0.0, 1.0, 1.0], dtype=torch.float64)).abs().max() <= 12 * TERM_BOUND), (depth, w)
    # a duplicated face counts twice, a face without area not at all
    twice = orient * geometry.winding_number((cv, torch.cat([cf, cf])), P, accuracy=INF)
    assert bool((twice - torch.tensor([0.25, 0.5, 0.0, 2.0, 2.0], dtype=torch.float64)).abs().max() <= 24 * TERM_BOUND)
    flat = torch.tensor([[0, 0, 7], [1, 7, 1], [3, 3, 3]], dtype=torch.int32)
    same = geometry.winding_number((cv, torch.cat([cf[:5], flat, cf[5:]])), P, accuracy=INF)
    assert bool((orient * same - torch.tensor([0.125, 0.25, 0.0, 1.0, 1.0], dtype=torch.float64)).abs().max() <= 15 * TERM_BOUND)
    # P = 0, 1, 65
    many = torch.rand(65, 3, dtype=f32, generator=torch.Generator().manual_seed(3)) * 2 - 0.5
    full = geometry.winding_number((cv, cf), many)
    for n in (0, 1, 65):
        w, n_exact, n_far = geometry.winding_number((cv, cf), many[:n], return_counts=True)
        assert tuple(w.shape) == (n,) and torch.equal(w, full[:n]) and tuple(n_exact.shape) == (n,) and tuple(n_far.shape) == (n,)
    # all faces but one in one leaf: a small sphere and one triangle far away
    sv, sf = indexed(icosphere(1, radius=0.01))
    far = torch.tensor([[10, 10, 10], [10, 11, 10], [11, 10, 10]], dtype=f32)
    lump = (torch.cat([sv, far]), torch.cat([sf, torch.tensor([[len(sv), len(sv) + 1, len(sv) + 2]], dtype=torch.int32)]))
    tree = meshing.winding_tree(*lump, depth=2)
    leaves = tree.count[tree.level == 2]
    assert sorted(leaves.tolist()) == [1, sf.shape[0]] and tree.n_nodes == 5
    q = torch.tensor([[0, 0, 0], [0.02, 0, 0], [5, 5, 5]], dtype=f32)
    w2, flat0 = meshing.mesh_winding(tree, q, INF)[0], meshing.mesh_winding(meshing.winding_tree(*lump, depth=0), q, INF)[0]
    assert bool(((w2 - flat0).abs() <= 2 * (sf.shape[0] + 1) * TERM_BOUND).all()) and abs(abs(float(w2[0])) - 1.0) < 1e-3
    # a NaN in a vertex: every winding number is NaN and nothing is inside; a NaN in a point: that point
    bad = cv.clone()
    bad[3, 1] = float("nan")
    assert bool(torch.isnan(geometry.winding_number((bad, cf), P)).all())
    assert not bool(geometry.mesh_contains((bad, cf), P, rule="winding").any())
    nanp = P.clone()
    nanp[1, 2] = float("nan")
    w = geometry.winding_number((cv, cf), nanp)
    assert bool(torch.isnan(w[1])) and bool(torch.isfinite(w[[0, 2, 3, 4]]).all())
    assert not bool(geometry.mesh_contains((cv, cf), nanp, rule="winding")[1])


def test_argument_errors():
    from arah_release_amd import geometry, meshing
    cv, cf = cube()
    P = torch.rand(4, 3)
    for accuracy in (0.5, float("nan"), "3", True, None):
        with pytest.raises(ValueError):
            geometry.winding_number((cv, cf), P, accuracy=accuracy)
        with pytest.raises(ValueError):
            geometry.mesh_contains((cv, cf), P, rule="winding", accuracy=accuracy)
    for rule in ("crossing", None, 1):
        for call in (lambda: geometry.mesh_contains((cv, cf), P, rule=rule), lambda: geometry.voxelize((cv, cf), dims=4, rule=rule),
                     lambda: geometry.mesh_iou((cv, cf), (cv, cf), n_points=10, rule=rule), lambda: geometry.mesh_sdf((cv, cf), P, rule=rule),
                     lambda: geometry.mesh_sdf_grid((cv, cf), dims=4, rule=rule), lambda: geometry.remesh((cv, cf), rule=rule)):
            with pytest.raises(ValueError):
                call()
    for depth in (-1, 8, 2.0, True):
        with pytest.raises(ValueError):
            meshing.winding_tree(cv, cf, depth)
    with pytest.raises(ValueError):
        meshing.winding_tree(cv, torch.tensor([[0, 1, 8]], dtype=torch.int32))          # a face id outside [0, V)
    with pytest.raises(ValueError):
        geometry.winding_number((cv, torch.tensor([[0, 1, -1]], dtype=torch.int32)), P)
    with pytest.raises(ValueError):
        geometry.winding_number((cv, cf), P, index=object())                             # an index belongs to a mesh on the GPU
    with pytest.raises(ValueError):
        meshing.mesh_winding(object(), P)
    assert meshing.check_accuracy(1) == 1.0 and meshing.check_accuracy(INF) == INF
    assert [meshing.winding_depth(n) for n in (0, 8, 9, 32, 33, 5172, 98304, 10 ** 8)] == [0, 0, 1, 1, 2, 5, 7, 7]


def test_rule_winding_through_geometry_on_the_host():
    """The dicts gain "winding", nothing is ambiguous, and the default calls keep their keys and bits."""
    from arah_release_amd import geometry
    cv, cf = cube()
    P = torch.tensor([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.1, 0.9, 0.2]], dtype=torch.float32)
    sdf = geometry.mesh_sdf((cv, cf), P, rule="winding")
    assert set(sdf) == set(geometry.SDF_KEYS) | {"winding"} and sdf["inside"].tolist() == [True, False, True]
    assert not bool(sdf["ambiguous"].any()) and sdf["sdf"].tolist() == [-0.5, 0.5, pytest.approx(-0.1)]
    assert set(geometry.mesh_sdf((cv, cf), P)) == set(geometry.SDF_KEYS)
    vox = geometry.voxelize((cv, cf), dims=(4, 5, 3), padding=0.5, rule="winding")
    plain = geometry.voxelize((cv, cf), dims=(4, 5, 3), padding=0.5)
    assert set(vox) == set(plain) | {"winding"} and torch.equal(vox["occupancy"], plain["occupancy"]) and int(vox["ambiguous"]) == 0
    field = geometry.mesh_sdf_grid((cv, cf), dims=(4, 5, 3), padding=0.5, rule="winding")
    assert torch.equal(field["inside"], vox["occupancy"]) and tuple(field["winding"].shape) == (4, 5, 3)
    iou = geometry.mesh_iou((cv, cf), (cv * 0.5, cf), n_points=4000, rule="winding")
    assert set(iou) == set(geometry.IOU_KEYS) | {"n_points", "winding"}
    assert abs(float(iou["iou"]) - 0.125) < 0.03 and int(iou["ambiguous_a"]) == 0
    assert set(geometry.mesh_iou((cv, cf), (cv * 0.5, cf), n_points=100)) == set(geometry.IOU_KEYS) | {"n_points"}


def test_declared_symbols_equal_the_exported_symbols():
    from arah_release_amd import hip
    header = open(os.path.join(REPO, "include", "arah_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(arah_[a-z0-9_]+)\s*\(", header))
    assert declared == set(hip.EXPORTS) and set(NEW_EXPORTS) <= declared
    assert len(hip.EXPORTS) == len(set(hip.EXPORTS))
