"""Quadric-error vertex placement and face-count targets for geometry.simplify_mesh: the tensor specification
meshing.mesh_quadric_place against a numpy float64 restatement written with python loops (bit for bit), the properties the
placement must have (a plane stays, a ridge is found, a sphere keeps its surface and its volume, the fall-backs fall back), the
face-count search against a restatement of its rule, and the C ABI's declarations and argument checks.  Everything here runs on
the host; tests/test_mesh_quadric_gpu.py holds the kernels of csrc/meshquadric.hpp to the specification."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("arah_mesh_quadric_place_scratch_bytes", "arah_mesh_quadric_place")
OLD_KEYS = {"verts", "faces", "n_verts", "n_tris", "vert_src", "removed", "cell", "dims"}
LIMIT = 1 << 15
_MESH, _CLUSTERED, _SPEC, _RESTATED = {}, {}, {}, {}


# ---- meshes -------------------------------------------------------------------------------------------------------------------------
def sphere_field(n, radius=0.8):
    ax = torch.linspace(-1, 1, n)
    X, Y, Z = torch.meshgrid(ax, ax, ax, indexing="ij")
    return torch.sqrt(X ** 2 + Y ** 2 + Z ** 2) - radius


def dirty(verts, faces):
    """The mesh with a non-finite vertex, an id out of range (above and below), a repeated-id face and a zero-area face (three
    different ids, two of them at one position)."""
    V = verts.shape[0]
    verts = torch.cat([verts, verts[5:6]])                                        # vertex V sits on vertex 5
    verts[11, 1] = float("nan")
    a, b = int(faces[40, 0]), int(faces[40, 1])
    more = torch.tensor([[3, 4, V + 7], [-1, 8, 9], [a, a, b], [5, V, int(faces[0, 2])]], dtype=faces.dtype)
    return verts, torch.cat([faces[:100], more, faces[100:]])


def fan(n, wave=0.15):
    """n triangles around vertex 0, the rim a circle of radius 1 whose height waves: a one-cell cluster of n faces that is not
    flat, so the quadric has full rank."""
    k = torch.arange(n + 1, dtype=torch.float64)
    ang = k * (2.0 * math.pi / n)
    rim = torch.stack([torch.cos(ang), torch.sin(ang), wave * torch.sin(3.0 * ang) + 0.05 * torch.cos(7.0 * ang)], 1)
    verts = torch.cat([torch.tensor([[0.0, 0.0, 0.3]], dtype=torch.float64), rim]).float()
    i = torch.arange(1, n + 1)
    return verts, torch.stack([torch.zeros_like(i), i, i + 1], 1)


def flat_grid(n):
    """n x n quads in the plane z = 0.25 over [0, 1]^2, two triangles each."""
    ax = torch.arange(n + 1, dtype=torch.float32) / n
    X, Y = torch.meshgrid(ax, ax, indexing="ij")
    verts = torch.stack([X.reshape(-1), Y.reshape(-1), torch.full(((n + 1) ** 2,), 0.25)], 1)
    i, j = torch.meshgrid(torch.arange(n), torch.arange(n), indexing="ij")
    p = (i * (n + 1) + j).reshape(-1)
    faces = torch.cat([torch.stack([p, p + n + 1, p + 1], 1), torch.stack([p + 1, p + n + 1, p + n + 2], 1)])
    return verts, faces


def mesh(name):
    """(verts (V,3) float32, faces (F,3) int64) of a named mesh on the host, computed once and shared; never modified."""
    from arah_release_amd import meshing
    if name not in _MESH:
        if name.startswith("sphere"):
            verts, faces, _ = meshing.marching_cubes_indexed(sphere_field(int(name[6:8])))
            if name.endswith("_dirty"):
                verts, faces = dirty(verts, faces)
        elif name.startswith("fan"):
            verts, faces = fan(int(name[3:]))
        elif name == "plane150":
            verts, faces = flat_grid(150)
        _MESH[name] = (verts, faces)
    return _MESH[name]


def grid_of(verts, cell):
    """simplify_mesh's grid rule, in float32, over the box of the finite vertices."""
    v = verts.numpy()[np.isfinite(verts.numpy()).all(1)]
    lo, hi, c = v.min(0).astype(np.float32), v.max(0).astype(np.float32), np.float32(cell)
    origin = (np.floor(lo / c) * c).astype(np.float32)
    return [float(x) for x in origin], float(c), [int(x) + 1 for x in np.floor((hi - origin) / c)]


def grid(name, mult):
    """The grid of a case: `mult` lattice steps for a sphere; 0, and every other mesh: one cell that holds everything."""
    verts = mesh(name)[0]
    if mult == 0 or not name.startswith("sphere"):
        return [-2.0, -2.0, -2.0], 4.0, [1, 1, 1]
    return grid_of(verts, mult * 2.0 / (int(name[6:8]) - 1))


def clustered(name, mult):
    """(verts, faces, vert_map, means, counts, cell) of a case: the inputs of the placement, computed once; never modified."""
    from arah_release_amd import meshing
    if (name, mult) not in _CLUSTERED:
        verts, faces = mesh(name)
        g = grid(name, mult)
        means, _, vert_map, _, _, counts = meshing.mesh_simplify(verts, faces, *g, position="mean")
        _CLUSTERED[(name, mult)] = (verts, faces, vert_map, means, counts, g[1])
    return _CLUSTERED[(name, mult)]


def spec(name, mult, reg=1e-3):
    """meshing.mesh_quadric_place of a case on the host, computed once and shared; never modified."""
    from arah_release_amd import meshing
    if (name, mult, reg) not in _SPEC:
        _SPEC[(name, mult, reg)] = meshing.mesh_quadric_place(*clustered(name, mult), reg=reg)
    return _SPEC[(name, mult, reg)]


# ---- an independent restatement ---------------------------------------------------------------------------------------------------
def numpy_quadric(verts, faces, vert_map, means, K, cell, reg):
    """The rule once more in numpy float64 scalars: python loops over faces and clusters, the tree as written, the cofactors
    written out.  -> (pos (V,3) float32, vert_src (V,) int32, qcounts (4,) int32)."""
    verts32, means32 = np.asarray(verts, np.float32), np.asarray(means, np.float32)
    v64, faces, vert_map = verts32.astype(np.float64), np.asarray(faces, np.int64), np.asarray(vert_map, np.int64)
    V, F = v64.shape[0], faces.shape[0]
    cell, reg = np.float64(np.float32(cell)), np.float64(reg)
    segments = [[] for _ in range(K)]
    for f in range(F):
        ids = [int(i) for i in faces[f]]
        if not all(0 <= i < V for i in ids):
            continue
        cs = [int(vert_map[i]) for i in ids]
        if not all(0 <= c < K for c in cs):
            continue
        for j, c in enumerate(cs):
            if c not in cs[:j]:
                segments[c].append(f)                                             # ascending face id by construction
    pos = np.zeros((V, 3), np.float32)
    fallbacks, longest, status = 0, max([len(s) for s in segments] + [0]), 0
    with np.errstate(all="ignore"):
        for k in range(K):
            pos[k] = means32[k]
            n = len(segments[k])
            if n > LIMIT:
                status = 2
                continue
            m = means32[k].astype(np.float64)
            x = []
            for f in segments[k]:
                pa, pb, pc = (v64[faces[f, j]] - m for j in range(3))
                e1, e2 = pb - pa, pc - pa
                nx = e1[1] * e2[2] - e1[2] * e2[1]
                ny = e1[2] * e2[0] - e1[0] * e2[2]
                nz = e1[0] * e2[1] - e1[1] * e2[0]
                d = -((nx * pa[0] + ny * pa[1]) + nz * pa[2])
                x.append(np.array([nx * nx, nx * ny, nx * nz, ny * ny, ny * nz, nz * nz, nx * d, ny * d, nz * d]))
            stride = 1
            while stride < n:
                for i in range(0, n, 2 * stride):
                    if i + stride < n:
                        x[i] = x[i] + x[i + stride]
                stride *= 2
            A00, A01, A02, A11, A12, A22, b0, b1, b2 = x[0] if n else np.zeros(9)
            t = (A00 + A11) + A22
            if not (np.isfinite(t) and t > 0):
                fallbacks += 1
                continue
            lam = reg * t
            M00, M11, M22, M01, M02, M12 = A00 + lam, A11 + lam, A22 + lam, A01, A02, A12
            C00 = M11 * M22 - M12 * M12
            C01 = M02 * M12 - M01 * M22
            C02 = M01 * M12 - M02 * M11
            C11 = M00 * M22 - M02 * M02
            C12 = M01 * M02 - M00 * M12
            C22 = M00 * M11 - M01 * M01
            det = (M00 * C00 + M01 * C01) + M02 * C02
            if not (np.isfinite(det) and det > 0):
                fallbacks += 1
                continue
            y = [-((C00 * b0 + C01 * b1) + C02 * b2) / det, -((C01 * b0 + C11 * b1) + C12 * b2) / det,
                 -((C02 * b0 + C12 * b1) + C22 * b2) / det]
            if not all(np.isfinite(ya) and abs(ya) <= cell for ya in y):
                fallbacks += 1
                continue
            pos[k] = [np.float32(m[a] + y[a]) for a in range(3)]
        best = {}
        for v in range(V):
            k = int(vert_map[v])
            if not 0 <= k < K:
                continue
            dx, dy, dz = v64[v] - pos[k].astype(np.float64)
            d2 = np.float32((dx * dx + dy * dy) + dz * dz)
            if k not in best or d2 < best[k][0]:                                  # ascending v: a tie keeps the lowest id
                best[k] = (d2, v)
    vert_src = np.zeros(V, np.int32)
    for k, (_, v) in best.items():
        vert_src[k] = v
    return pos, vert_src, np.array([fallbacks, sum(len(s) for s in segments), longest, status], np.int32)


def restated(name, mult, reg=1e-3):
    if (name, mult, reg) not in _RESTATED:
        verts, faces, vert_map, means, counts, cell = clustered(name, mult)
        _RESTATED[(name, mult, reg)] = numpy_quadric(verts.numpy(), faces.numpy(), vert_map.numpy(), means.numpy(), int(counts[0]),
                                                     cell, reg)
    return _RESTATED[(name, mult, reg)]


def same_bits(got, want, what):
    pos, src, qc = got
    assert pos.dtype == torch.float32 and src.dtype == torch.int32 and qc.dtype == torch.int32, what
    assert np.array_equal(pos.cpu().numpy().view(np.int32), np.asarray(want[0]).view(np.int32)), (what, "pos")
    assert np.array_equal(src.cpu().numpy(), np.asarray(want[1])), (what, "vert_src")
    assert qc.cpu().tolist() == [int(x) for x in want[2]], (what, "qcounts", qc.tolist(), list(want[2]))


SPEC_CASES = [("sphere17", 2), ("sphere17", 4), ("sphere33", 2), ("sphere33", 4), ("sphere17_dirty", 2), ("sphere17_dirty", 4)]


# ---- 1: the specification is the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mult", SPEC_CASES)
def test_specification_is_the_restatement(name, mult):
    got, want = spec(name, mult), restated(name, mult)
    same_bits(got, want, (name, mult))
    K = int(clustered(name, mult)[4][0])
    assert K > 8 and int(got[2][1]) > K and not got[0][K:].any() and not got[1][K:].any()
    if name.endswith("_dirty"):                                                   # the garbage is there and is skipped
        verts, faces, vert_map = clustered(name, mult)[:3]
        assert int(vert_map[11]) == -1 and int(got[2][3]) == 0
        assert int(got[2][1]) < int(spec(name[:-6], mult)[2][1])                 # the faces around vertex 11 went, two came


def test_tree_sum_is_the_loop():
    from arah_release_amd import meshing
    g = torch.Generator().manual_seed(5)
    n = torch.tensor([0, 1, 2, 3, 7, 8, 9, 33, 0, 257])
    x = torch.randn(int(n.sum()), 2, generator=g, dtype=torch.float64) * torch.logspace(-6, 6, int(n.sum()), dtype=torch.float64)[:, None]
    start = torch.cumsum(n, 0) - n
    got = meshing.quadric_tree_sum(x, start, n)
    for k in range(n.shape[0]):
        seg = [x[int(start[k]) + i].clone() for i in range(int(n[k]))]
        stride = 1
        while stride < len(seg):
            for i in range(0, len(seg), 2 * stride):
                if i + stride < len(seg):
                    seg[i] = seg[i] + seg[i + stride]
            stride *= 2
        assert torch.equal(got[k], seg[0] if seg else torch.zeros(2, dtype=torch.float64)), k


# ---- 2: a plane stays where it is -------------------------------------------------------------------------------------------------
def test_plane_at_a_dyadic_height_keeps_its_means():
    from arah_release_amd import meshing
    verts, faces = flat_grid(16)
    means, _, vert_map, _, _, counts = meshing.mesh_simplify(verts, faces, [0.0, 0.0, 0.0], 0.25, [5, 5, 2], position="mean")
    pos, src, qc = meshing.mesh_quadric_place(verts, faces, vert_map, means, counts, 0.25)
    assert int(counts[0]) == 25 and qc.tolist()[0] == 0 and qc.tolist()[3] == 0
    assert torch.equal(pos.view(torch.int32), means.view(torch.int32))


# ---- 3: a ridge is found -----------------------------------------------------------------------------------------------------------
def test_roof_ridge_inside_the_cells():
    from arah_release_amd import meshing
    n, h, cell = 20, 0.1, 0.5
    i, j = torch.meshgrid(torch.arange(n + 1), torch.arange(n + 1), indexing="ij")
    x, y = (i.reshape(-1) - n // 2).double() * h, (j.reshape(-1) - n // 2).double() * h
    verts = torch.stack([x, y, -x.abs()], 1).float()
    p = (i[:-1, :-1] * (n + 1) + j[:-1, :-1]).reshape(-1)
    faces = torch.cat([torch.stack([p, p + n + 1, p + 1], 1), torch.stack([p + 1, p + n + 1, p + n + 2], 1)])
    means, _, vert_map, _, _, counts = meshing.mesh_simplify(verts, faces, [-1.25] * 3, cell, [5, 5, 5], position="mean")
    pos, _, qc = meshing.mesh_quadric_place(verts, faces, vert_map, means, counts, cell)
    K = int(counts[0])
    left = torch.zeros(K).index_add_(0, vert_map.long(), (verts[:, 0] < -0.05).float()) > 0
    right = torch.zeros(K).index_add_(0, vert_map.long(), (verts[:, 0] > 0.05).float()) > 0
    ridge = left & right
    assert int(ridge.sum()) == 5 and qc.tolist()[0] == 0
    assert float(pos[:K][ridge][:, [0, 2]].abs().max()) <= 0.01 * cell           # on the ridge line x = z = 0
    assert float((means[:K][ridge][:, 2] + cell / 4).abs().max()) <= 0.05 * cell  # where the means sat: inside the roof
    flat = ~ridge                                                                 # one slope only: the minimiser stays on its plane
    assert float((pos[:K][flat][:, 2] + pos[:K][flat][:, 0].abs()).abs().max()) <= 1e-6


# ---- 4: a sphere keeps its surface and its volume ---------------------------------------------------------------------------------
def surface_error_and_volume(verts, faces, radius=0.8, n_samples=16):
    """Area-weighted mean of | |p| - r | over fixed seeded barycentric samples of every face, and the signed volume / the
    sphere's, in float64."""
    g = torch.Generator().manual_seed(1234)
    u = torch.rand(n_samples, 2, generator=g, dtype=torch.float64)
    flip = u.sum(1) > 1
    u[flip] = 1 - u[flip]
    w = torch.cat([1 - u.sum(1, keepdim=True), u], 1)                             # (S,3) barycentric
    tri = verts.double()[faces.long()]                                            # (F,3,3)
    area = torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]).norm(dim=1) / 2
    pts = torch.einsum("sc,fcx->fsx", w, tri)
    err = (pts.norm(dim=2) - radius).abs().mean(1)
    vol = (tri[:, 0] * torch.linalg.cross(tri[:, 1], tri[:, 2])).sum() / 6
    return float((err * area).sum() / area.sum()), abs(float(vol)) / (4 / 3 * math.pi * radius ** 3)


@pytest.mark.parametrize("mult", [2, 4])
def test_sphere_keeps_its_surface_and_volume(mult):
    from arah_release_amd import geometry
    verts, faces = mesh("sphere33")
    cell = mult * 2.0 / 32
    mean = geometry.simplify_mesh(verts, faces, cell=cell, position="mean")
    quad = geometry.simplify_mesh(verts, faces, cell=cell, position="quadric")
    assert quad["quadric"]["fallbacks"] == 0 and torch.equal(mean["faces"], quad["faces"])
    (e_mean, v_mean), (e_quad, v_quad) = (surface_error_and_volume(r["verts"], r["faces"]) for r in (mean, quad))
    print("sphere33 cell %d steps: faces %d, surface error mean %.3e quadric %.3e (ratio %.3f), volume mean %.4f quadric %.4f "
          "(ratio of |1 - v| %.3f)" % (mult, quad["n_tris"], e_mean, e_quad, e_quad / e_mean, v_mean, v_quad,
                                        abs(1 - v_quad) / abs(1 - v_mean)))
    assert e_quad <= 0.5 * e_mean
    assert abs(1 - v_quad) <= 0.5 * abs(1 - v_mean)


# ---- 5: the fall-backs -------------------------------------------------------------------------------------------------------------
ONE_CELL = ([0.0, 0.0, 0.0], 1.0, [1, 1, 1])


def _one_cluster(verts, faces, reg):
    from arah_release_amd import meshing
    verts, faces = torch.tensor(verts, dtype=torch.float32), torch.tensor(faces)
    means, _, vert_map, _, _, counts = meshing.mesh_simplify(verts, faces, *ONE_CELL, position="mean")
    assert int(counts[0]) == 1
    got = meshing.mesh_quadric_place(verts, faces, vert_map, means, counts, 1.0, reg=reg)
    same_bits(got, numpy_quadric(verts.numpy(), faces.numpy(), vert_map.numpy(), means.numpy(), 1, 1.0, reg), "one cluster")
    return got, means


WEDGE = ([[0.1, 0.1, 0.0], [0.3, 0.1, 0.0], [0.1, 0.3, 0.0],                      # z = 0
          [0.1, 0.1, 0.051], [0.3, 0.1, 0.053], [0.1, 0.3, 0.051],                # z = 0.05 + 0.01 x: meets it at x = -5
          [0.1, 0.2, 0.1], [0.3, 0.2, 0.1], [0.2, 0.2, 0.3]],                     # y = 0.2
         [[0, 1, 2], [3, 4, 5], [6, 7, 8]])


def test_fall_backs_keep_the_mean_and_are_counted():
    planar = ([[0.125, 0.125, 0.5], [0.5, 0.125, 0.5], [0.125, 0.5, 0.5], [0.5, 0.5, 0.5]], [[0, 1, 2], [1, 3, 2]])
    (pos, _, qc), means = _one_cluster(*planar, reg=0.0)                           # rank 1 and no regulariser: det = 0
    assert qc.tolist() == [1, 2, 2, 0] and torch.equal(pos.view(torch.int32), means.view(torch.int32))
    (pos, _, qc), means = _one_cluster(*planar, reg=1e-3)                          # the regulariser makes it solvable: it stays
    assert qc.tolist() == [0, 2, 2, 0] and torch.equal(pos.view(torch.int32), means.view(torch.int32))
    needles = ([[0.1, 0.1, 0.1], [0.2, 0.2, 0.2], [0.4, 0.4, 0.4], [0.8, 0.8, 0.8]], [[0, 1, 2], [1, 2, 3], [0, 0, 3]])
    (pos, _, qc), means = _one_cluster(*needles, reg=1e-3)                         # zero-area faces only: t = 0
    assert qc.tolist() == [1, 3, 3, 0] and torch.equal(pos.view(torch.int32), means.view(torch.int32))
    (pos, _, qc), means = _one_cluster(*WEDGE, reg=1e-9)                           # the minimiser lies five cells away
    assert qc.tolist() == [1, 3, 3, 0] and torch.equal(pos.view(torch.int32), means.view(torch.int32))
    (pos, _, qc), means = _one_cluster(*WEDGE, reg=1e-3)                           # regularised it stays inside the cell, and moves
    assert qc.tolist() == [0, 3, 3, 0] and not torch.equal(pos, means) and float((pos[0] - means[0]).abs().max()) <= 1.0


# ---- 6: a segment too long to sort ------------------------------------------------------------------------------------------------
def test_long_segment_is_not_placed():
    from arah_release_amd import geometry
    verts, faces = mesh("plane150")
    means, counts = clustered("plane150", 0)[3:5]
    pos, src, qc = spec("plane150", 0)
    assert int(counts[0]) == 1 and qc.tolist() == [0, 45000, 45000, 2]
    assert torch.equal(pos.view(torch.int32), means.view(torch.int32)) and not pos[1:].any()
    with pytest.raises(ValueError, match="smaller cell or position='mean'"):
        geometry.simplify_mesh(verts, faces, cell=4.0, bounds=([-2.0] * 3, [2.0] * 3), position="quadric")
    assert geometry.simplify_mesh(verts, faces, cell=4.0, bounds=([-2.0] * 3, [2.0] * 3), position="mean")["n_verts"] == 0


# ---- 7: the numbering of the vertices does not matter ------------------------------------------------------------------------------
def test_renumbered_vertices_give_the_same_positions():
    from arah_release_amd import meshing
    verts, faces, _, _, counts, cell = clustered("sphere17", 2)
    perm = torch.randperm(verts.shape[0], generator=torch.Generator().manual_seed(3))     # new id -> old id
    new_id = torch.empty_like(perm)
    new_id[perm] = torch.arange(perm.shape[0])
    v2, f2 = verts[perm], new_id[faces]
    means, _, vert_map, _, _, counts2 = meshing.mesh_simplify(v2, f2, *grid("sphere17", 2), position="mean")
    pos2, _, qc2 = meshing.mesh_quadric_place(v2, f2, vert_map, means, counts2, cell)
    pos, _, qc = spec("sphere17", 2)
    assert torch.equal(counts, counts2) and torch.equal(qc, qc2)
    assert torch.equal(pos.view(torch.int32), pos2.view(torch.int32))             # clusters are numbered by their cells


# ---- 8: face-count targets --------------------------------------------------------------------------------------------------------
def restated_search(count, target, r_max=400):
    """The search rule once more.  count(r) -> kept faces."""
    probes = []

    def ask(r):
        probes.append((r, count(r)))
        return probes[-1][1]
    if ask(1) > target:
        return 1, probes, False
    if ask(r_max) <= target:
        return r_max, probes, True
    lo, hi = 1, r_max
    while hi - lo != 1:
        mid = (lo + hi) // 2
        if ask(mid) <= target:
            lo = mid
        else:
            hi = mid
    return lo, probes, True


@pytest.mark.parametrize("target,position", [(300, "mean"), (1000, "quadric"), (10 ** 6, "member"), (3, "mean")])
def test_target_faces_is_the_search(target, position):
    from arah_release_amd import geometry
    verts, faces = mesh("sphere17")

    def count(r):
        return geometry.simplify_mesh(verts, faces, resolution=r)["n_tris"]
    got = geometry.simplify_mesh(verts, faces, target_faces=target, position=position)
    r, probes, reached = restated_search(count, target)
    assert (got["resolution"], got["probes"], got["reached"]) == (r, probes, reached) and len(probes) <= 11
    want = geometry.simplify_mesh(verts, faces, resolution=r, position=position)
    assert set(got) == set(want) | {"resolution", "probes", "reached"}
    for key in want:
        same = torch.equal(got[key], want[key]) if isinstance(want[key], torch.Tensor) else got[key] == want[key]
        assert same, key
    if target == 3:
        assert not reached and r == 1 and got["n_tris"] > target
    else:
        assert reached and got["n_tris"] <= target and (r == 400 or count(r + 1) > target)
    assert (r == 400) == (target == 10 ** 6)


def test_exactly_one_of_cell_resolution_target():
    from arah_release_amd import geometry
    verts, faces = mesh("sphere17")
    for how in ({"cell": 0.2, "resolution": 8}, {"cell": 0.2, "target_faces": 100}, {"resolution": 8, "target_faces": 100},
                {"cell": 0.2, "resolution": 8, "target_faces": 100}, {}):
        with pytest.raises(ValueError):
            geometry.simplify_mesh(verts, faces, **how)
        with pytest.raises(ValueError):
            geometry.check_simplify(dict(how))


# ---- 9: the old modes return what they returned ------------------------------------------------------------------------------------
def test_key_sets():
    from arah_release_amd import geometry
    verts, faces = mesh("sphere17")
    normal = torch.nn.functional.normalize(verts, dim=1)
    for position in ("mean", "member"):
        assert set(geometry.simplify_mesh(verts, faces, cell=0.25, position=position)) == OLD_KEYS
    res = geometry.simplify_mesh(verts, faces, cell=0.25, position="quadric", attributes={"normal": normal})
    assert set(res) == OLD_KEYS | {"quadric", "normal"} and set(res["quadric"]) == {"fallbacks", "longest"}
    assert res["normal"].shape[0] == res["n_verts"] and torch.equal(res["normal"], normal[res["vert_src"]])
    d = (verts[res["vert_src"]] - res["verts"]).norm(dim=1)                       # the representative is a member of the cell
    assert float(d.max()) <= 0.25 * math.sqrt(3) * 2
    with pytest.raises(ValueError):
        geometry.simplify_mesh(verts, faces, cell=0.25, position="quadric", attributes={"quadric": normal})
    geometry.simplify_mesh(verts, faces, cell=0.25, attributes={"quadric": normal})        # free in the other modes, as before


# ---- 10: arguments and the ABI -----------------------------------------------------------------------------------------------------
def test_check_simplify_and_arguments():
    from arah_release_amd import geometry, meshing
    kw = {"target_faces": 500, "position": "quadric", "quadric_reg": 1e-2}
    assert geometry.check_simplify(kw) == kw
    for bad in ({"cell": 0.1, "quadric_reg": -1}, {"target_faces": 0}, {"target_faces": 2.5}, {"target_faces": True},
                {"cell": 0.1, "quadric_reg": float("nan")}, {"cell": 0.1, "position": "median"}, {"cell": 0.1, "quadric_reg": "x"}):
        with pytest.raises(ValueError):
            geometry.check_simplify(bad)
    verts, faces, vert_map, means, counts, cell = clustered("sphere17", 2)
    for bad in (lambda: meshing.mesh_quadric_place(verts.double(), faces, vert_map, means, counts, cell),
                lambda: meshing.mesh_quadric_place(verts, faces.float(), vert_map, means, counts, cell),
                lambda: meshing.mesh_quadric_place(verts, faces, vert_map[:-1], means, counts, cell),
                lambda: meshing.mesh_quadric_place(verts, faces, vert_map.float(), means, counts, cell),
                lambda: meshing.mesh_quadric_place(verts, faces, vert_map, means[:-1], counts, cell),
                lambda: meshing.mesh_quadric_place(verts, faces, vert_map, means, 2.5, cell),
                lambda: meshing.mesh_quadric_place(verts, faces, vert_map, means, counts, 0.0),
                lambda: meshing.mesh_quadric_place(verts, faces, vert_map, means, counts, float("inf")),
                lambda: meshing.mesh_quadric_place(verts, faces, vert_map, means, counts, cell, reg=-1e-3),
                lambda: meshing.mesh_quadric_place(verts, faces, vert_map, means, counts, cell, reg=float("nan"))):
        with pytest.raises(ValueError):
            bad()
    same = meshing.mesh_quadric_place(verts, faces.to(torch.int32), vert_map.long(), means, int(counts[0]), cell)
    for a, b in zip(same, spec("sphere17", 2)):
        assert torch.equal(a, b)
    empty = meshing.mesh_quadric_place(torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int64), torch.zeros(0, dtype=torch.int32),
                                       torch.zeros(0, 3), 0, 1.0)
    assert empty[0].shape == (0, 3) and empty[1].shape == (0,) and empty[2].tolist() == [0, 0, 0, 0]
    no_faces = meshing.mesh_quadric_place(verts, faces[:0], vert_map, means, counts, cell)            # every cluster falls back
    assert no_faces[2].tolist() == [int(counts[0]), 0, 0, 0] and torch.equal(no_faces[0], means)


def test_new_entries_are_declared_exported_and_check_their_arguments():
    import __graft_entry__ as g
    g.build()
    from arah_release_amd import hip
    lib = hip.load_library()
    header = open(os.path.join(REPO, "include", "arah_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(arah_[a-z0-9_]+)\s*\(", header))
    for name in NEW_EXPORTS:
        assert name in declared and name in hip.EXPORTS and hasattr(lib, name), name
    assert len(hip.EXPORTS) == len(set(hip.EXPORTS))
    source = open(os.path.join(REPO, "arah_release_amd", "csrc", "meshquadric.hpp")).read()
    kernels = set(re.findall(r"__global__[^\n]*?void (k_[a-z0-9_]+)\(", source))
    assert kernels and all(k.startswith("k_mq_") for k in kernels)
    assert "atomicAdd(float" not in source and "unsafeAtomicAdd" not in source
    # the argument checks answer before anything touches a device
    size = lib.arah_mesh_quadric_place_scratch_bytes
    assert size(10, 10) > 0 and size(0, 0) > 0 and size(10, 10) % 256 == 0
    for sizes in ((-1, 0), (0, -1), (2 ** 26 + 1, 0), (0, 2 ** 28 + 1)):
        assert size(*sizes) == 0
    BADARG, p = -1, C.c_void_p(256)                                               # a pointer that is never followed

    def call(V=4, F=2, verts=p, faces=p, vert_map=p, means=p, counts=p, cell=0.5, reg=1e-3, pos=p, src=p, qc=p, scratch=p):
        return lib.arah_mesh_quadric_place(verts, C.c_int64(V), faces, C.c_int64(F), vert_map, means, counts, C.c_float(cell),
                                           C.c_double(reg), pos, src, qc, scratch, C.c_size_t(1 << 20), None)
    for bad in ({"V": -1}, {"F": -1}, {"V": 2 ** 26 + 1}, {"F": 2 ** 28 + 1}, {"pos": None}, {"src": None}, {"verts": None},
                {"faces": None}, {"vert_map": None}, {"means": None}, {"counts": None}, {"qc": None}, {"scratch": None},
                {"cell": float("nan")}, {"cell": float("inf")}, {"cell": 0.0}, {"reg": float("nan")}, {"reg": float("inf")},
                {"reg": -1.0}):
        assert call(**bad) == BADARG, bad
