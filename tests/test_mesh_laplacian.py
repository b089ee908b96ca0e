"""The cotangent Laplacian, curvatures and cotangent smoothing on the host: the tensor specifications meshing.mesh_cotangent /
laplacian_apply / mesh_curvature / mesh_smooth(weights="cotangent") against a numpy float64 restatement written with python loops
(bit for bit), symmetry, linear precision on planar meshes, the partition of the area, Gauss-Bonnet, convergence on refined
spheres, the cases with a known answer, and the argument checks.  Everything here runs on the host;
tests/test_mesh_laplacian_gpu.py holds the kernels of csrc/meshlaplace.hpp to the specification."""
import math
import os
import re

import numpy as np
import pytest
import torch

from test_mesh_flip import adjacency_np, mesh as flip_mesh

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("arah_mesh_cotangent", "arah_mesh_laplacian_apply", "arah_mesh_curvature", "arah_mesh_smooth_cotangent_scratch_bytes",
               "arah_mesh_smooth_cotangent")
NAMES = ("faces", "degenerate", "nonfinite", "obtuse", "negative_edges", "bad_area")
MASSES = ("barycentric", "mixed")
HOST = ("tetrahedron", "octahedron", "kite", "sheet", "three_faces", "misoriented", "nan_vertex", "bad_ids", "open_sphere", "bicone40",
        "jgrid9_0", "sphere9", "zero_area", "repeated_id")
ATAN2_TERM = 2.0 ** -47                 # 16 ulp of an angle below 4: the allowance of tests/test_mesh_winding_gpu.py, per corner angle
_MESH, _SPEC, _REST = {}, {}, {}


# ---- meshes -------------------------------------------------------------------------------------------------------------------------
def icosahedron():
    t = (1.0 + math.sqrt(5.0)) / 2.0
    v = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1], [-t, 0, -1],
         [-t, 0, 1]]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8], [3, 9, 4],
         [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    return torch.tensor(v, dtype=torch.float32), torch.tensor(f)


def icosphere(levels, radius):
    """An icosahedron refined `levels` times by midpoint subdivision, every vertex pushed to the sphere; counter-clockwise faces."""
    from arah_release_amd import meshing
    verts, faces = icosahedron()
    for _ in range(levels):
        out = meshing.mesh_subdivide_round(verts, faces, method="midpoint")
        verts, faces = out[0][:int(out[4][0])], out[1][:int(out[4][1])].long()      # rows past the counts are padding
    verts = (verts.double() / verts.double().norm(dim=1, keepdim=True) * radius).float()
    return verts, faces


def mesh(name):
    """(verts (V,3) float32, faces (F,3) int64) of a named mesh on the host, computed once and shared; never modified."""
    if name not in _MESH:
        if name == "zero_area":                                                   # a face with three collinear corners in the sheet
            verts, faces = flip_mesh("sheet")
            verts = torch.cat([verts, torch.tensor([[2.0, 0.0, 0.0], [3.0, 0.0, 0.0], [4.0, 0.0, 0.0]])])
            V = verts.shape[0]
            faces = torch.cat([faces[:7], torch.tensor([[V - 3, V - 2, V - 1]]), faces[7:]])
        elif name == "repeated_id":
            verts, faces = flip_mesh("octahedron")
            faces = torch.cat([faces[:3], torch.tensor([[0, 0, 4], [2, 5, 2]]), faces[3:]])
        elif name == "fin":                                                       # a third face on an edge of the octahedron
            verts, faces = flip_mesh("octahedron")
            verts = torch.cat([verts, torch.tensor([[1.0, 1.0, 1.0]])])
            faces = torch.cat([faces, torch.tensor([[0, 2, 6]])])
        elif name.startswith("ico"):                                              # ico<levels>: radius 0.75
            verts, faces = icosphere(int(name[3:]), 0.75)
        else:
            verts, faces = flip_mesh(name)
        _MESH[name] = (verts.contiguous(), faces.contiguous())
    return _MESH[name]


def spec(name, mass="mixed"):
    """meshing.mesh_adjacency, mesh_cotangent and mesh_curvature of a case on the host, computed once and shared; never modified."""
    from arah_release_amd import meshing
    if (name, mass) not in _SPEC:
        verts, faces = mesh(name)
        adj = meshing.mesh_adjacency(faces, verts.shape[0])
        lap = meshing.mesh_cotangent(verts, faces, mass, adj)
        _SPEC[name, mass] = (adj, lap, meshing.mesh_curvature(verts, faces, mass, adj, lap))
    return _SPEC[name, mass]


def counts_of(lap):
    return dict(zip(NAMES, lap[4].tolist()))


# ---- an independent restatement: plain loops over numpy float64 scalars ----------------------------------------------------------
def dot(x, y):
    return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]


def numpy_face(p):
    """state (0 contributing, 1 degenerate, 2 nonfinite), A2, dot[3], l2[3] of the corners p (3,3) float64."""
    if not np.isfinite(p).all():
        return 2, None, None, None
    a, b = p[1] - p[0], p[2] - p[0]
    N = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    A2 = np.sqrt(dot(N, N))
    if not (np.isfinite(A2) and A2 > 0):
        return 1, None, None, None
    d, l2 = [], []
    for c in range(3):
        u, w, e = p[(c + 1) % 3] - p[c], p[(c + 2) % 3] - p[c], p[(c + 2) % 3] - p[(c + 1) % 3]
        d.append(dot(u, w))
        l2.append(dot(e, e))
    return 0, A2, d, l2


def numpy_cotangent(verts, faces, mass):
    """The whole rule of meshing.mesh_cotangent: weight, diag, area, angle_sum, counts -- and the entries' (v, n)."""
    verts, faces = verts.numpy().astype(np.float64), faces.numpy()
    V, F = verts.shape[0], faces.shape[0]
    valid, vf, _, _, nbr, start = adjacency_np(faces, V)
    with np.errstate(all="ignore"):
        info = [numpy_face(verts[faces[f]]) if valid[f] else None for f in range(F)]
        weight, diag, area, angle_sum = np.zeros(6 * F), np.zeros(V), np.zeros(V), np.zeros(V)
        counts = [0] * 8
        for f in range(F):
            if valid[f]:
                state, _, d, _ = info[f]
                counts[state] += 1
                counts[3] += int(state == 0 and min(d) < 0)
        ev, en = [], []
        for v in range(V):
            for j, n in enumerate(nbr[v]):
                acc = np.float64(0.0)
                for f in vf[v]:
                    ids = faces[f].tolist()
                    if n in ids and info[f][0] == 0:
                        o = 3 - ids.index(v) - ids.index(n)
                        acc = acc + info[f][2][o] / info[f][1]
                w = 0.5 * acc
                weight[start[v] + j] = w
                diag[v] = diag[v] + w
                counts[4] += int(n > v and w < 0)
                ev.append(v)
                en.append(n)
            ang, ar = np.float64(0.0), np.float64(0.0)
            for f in vf[v]:
                state, A2, d, l2 = info[f]
                if state:
                    continue
                c = faces[f].tolist().index(v)
                ang = ang + np.arctan2(A2, d[c])
                if mass == "barycentric":
                    ar = ar + A2
                else:
                    obtuse = [k for k in range(3) if d[k] < 0]
                    a, b = (c + 1) % 3, (c + 2) % 3
                    if not obtuse:
                        ar = ar + (l2[a] * (d[a] / A2) + l2[b] * (d[b] / A2)) * 0.125
                    else:
                        ar = ar + (A2 * 0.25 if obtuse[0] == c else A2 * 0.125)
            angle_sum[v] = ang
            area[v] = ar / 6.0 if mass == "barycentric" else ar
            counts[5] += int(not area[v] > 0)
    return weight, diag, area, angle_sum, np.array(counts, dtype=np.int32), np.array(ev, dtype=np.int64), np.array(en, dtype=np.int64), nbr, start


def numpy_apply(weight, nbr, start, x):
    x = x.astype(np.float64)
    y = np.zeros_like(x)
    with np.errstate(all="ignore"):
        for v in range(x.shape[0]):
            for c in range(x.shape[1]):
                acc = np.float64(0.0)
                for j, n in enumerate(nbr[v]):
                    w = weight[start[v] + j]
                    if np.isfinite(w) and np.isfinite(x[n, c]):
                        acc = acc + w * (x[n, c] - x[v, c])
                y[v, c] = acc if np.isfinite(x[v, c]) else np.nan
    return y


def numpy_curvature(verts, weight, area, angle_sum, normal_sum, flags, nbr, start):
    verts, V = verts.numpy(), verts.shape[0]
    L = numpy_apply(weight, nbr, start, verts)
    curv, mean_normal, valid = np.full((V, 5), np.nan), np.full((V, 3), np.nan), np.zeros(V, dtype=np.uint8)
    with np.errstate(all="ignore"):
        for v in range(V):
            N = normal_sum[v]
            length = np.sqrt(dot(N, N))
            if flags[v] & 6 or not np.isfinite(verts[v]).all() or not (np.isfinite(area[v]) and area[v] > 0) \
                    or not (np.isfinite(length) and length > 0):
                continue
            K = [(-L[v, c]) / area[v] for c in range(3)]
            mean = 0.5 * (dot(K, N) / length)
            gauss = ((math.pi if flags[v] & 1 else 2.0 * math.pi) - angle_sum[v]) / area[v]
            disc = mean * mean - gauss
            root = np.sqrt(disc if disc > 0 else np.float64(0.0))
            curv[v] = [mean, 0.5 * np.sqrt(dot(K, K)), gauss, mean + root, mean - root]
            mean_normal[v] = [0.5 * k for k in K]
            valid[v] = 1
    return curv, mean_normal, valid


def numpy_smooth(verts, faces, steps, factors, pin):
    from arah_release_amd import meshing
    flags = meshing.mesh_adjacency(faces, verts.shape[0])[6].numpy()
    cur = verts.numpy().copy()
    with np.errstate(all="ignore"):
        for step in range(steps):
            f = np.float64(np.float32(factors[step % len(factors)]))
            weight, _, _, _, _, _, _, nbr, start = numpy_cotangent(torch.from_numpy(cur), faces, "mixed")
            new = cur.copy()
            for v in range(cur.shape[0]):
                p = cur[v].astype(np.float64)
                if not np.isfinite(p).all() or (pin and flags[v] & 3):
                    continue
                s, acc = np.float64(0.0), np.zeros(3)
                for j, n in enumerate(nbr[v]):
                    w, q = weight[start[v] + j], cur[n].astype(np.float64)
                    if np.isfinite(q).all() and np.isfinite(w):
                        s = s + abs(w)
                        acc = acc + w * (q - p)
                if np.isfinite(s) and s > 0:
                    new[v] = (p + f * (acc / s)).astype(np.float32)
            cur = new
    return cur


def restatement(name, mass):
    if (name, mass) not in _REST:
        _REST[name, mass] = numpy_cotangent(*mesh(name), mass)
    return _REST[name, mass]


def bits(x):
    x = np.ascontiguousarray(x.numpy() if torch.is_tensor(x) else x)
    return x.view({8: np.int64, 4: np.int32, 1: np.uint8}[x.dtype.itemsize]) if x.dtype.kind == "f" else x


def same_bits(got, want, what):
    g, w = bits(got), bits(want)
    assert g.dtype == w.dtype and g.shape == w.shape, (what, g.dtype, w.dtype, g.shape, w.shape)
    assert np.array_equal(g, w), (what, int((g != w).sum()))


# ---- 1: the specification is the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mass", MASSES)
@pytest.mark.parametrize("name", HOST)
def test_specification_is_the_restatement(name, mass):
    from arah_release_amd import meshing
    verts, faces = mesh(name)
    adj, lap, _ = spec(name, mass)
    weight, diag, area, angle_sum, counts, _, _, nbr, start = restatement(name, mass)
    for key, g, w in zip(("weight", "diag", "area", "counts"), (lap[0], lap[1], lap[2], lap[4]), (weight, diag, area, counts)):
        same_bits(g, w, (name, mass, key))
    # numpy's atan2 (libm) and torch's (a vectorised one) differ in the last bit of a few angles -- equality was tried and fails on
    # one vertex of the sheet -- so angle_sum takes the allowance of the GPU tests: the atan2 term for each of the vertex's faces
    deg = (adj[0][1:] - adj[0][:-1]).numpy()
    off = np.abs(lap[3].numpy() - angle_sum)
    print("%s %s: angle_sum differs from numpy's at %d vertices, by at most %.3g" % (name, mass, int((off > 0).sum()), off.max(initial=0.0)))
    assert (off <= deg * ATAN2_TERM).all(), (name, mass, "angle_sum")
    x = torch.from_numpy(np.random.RandomState(5).standard_normal((verts.shape[0], 5)))
    x[1 % max(verts.shape[0], 1), 2] = float("inf")
    for t in (x, x.float(), verts):
        same_bits(meshing.laplacian_apply(lap[0], adj, t), numpy_apply(weight, nbr, start, t.numpy()), (name, mass, "apply", t.dtype))
    normal_sum = meshing.vertex_normals(verts, faces, adj)[0]
    curv, mean_normal, valid, n_bad = meshing.mesh_curvature(verts, faces, mass, adj, (lap[0], lap[1], lap[2], torch.from_numpy(angle_sum)),
                                                              normal_sum)
    want = numpy_curvature(verts, weight, area, angle_sum, normal_sum.numpy(), adj[6].numpy(), nbr, start)
    for key, g, w in zip(("curv", "mean_normal", "valid"), (curv, mean_normal, valid), want):
        same_bits(g, w, (name, mass, key))
    assert int(n_bad) == int((want[2] == 0).sum())


@pytest.mark.parametrize("name", ["sheet", "nan_vertex", "bicone40", "three_faces", "kite"])
def test_cotangent_smoothing_is_the_restatement(name):
    from arah_release_amd import meshing
    verts, faces = mesh(name)
    for how, factors in (({"method": "taubin", "boundary": "free"}, (0.5, -0.53)), ({"method": "laplacian", "lamb": 0.7}, (0.7,))):
        got = meshing.mesh_smooth(verts, faces, 2, weights="cotangent", **how)
        same_bits(got, numpy_smooth(verts, faces, 2 * len(factors), factors, how.get("boundary", "pin") == "pin"), (name, how))


# ---- 2: symmetry ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", HOST)
def test_weights_are_symmetric_and_rows_sum_to_zero(name):
    from arah_release_amd import geometry
    verts, faces = mesh(name)
    adj, lap, _ = spec(name)
    _, _, _, _, _, ev, en, nbr, start = restatement(name, "mixed")
    w = lap[0].numpy()
    at = {(int(v), int(n)): i for i, (v, n) in enumerate(zip(ev, en))}
    for (v, n), i in at.items():
        assert bits(w[i:i + 1])[0] == bits(w[at[n, v]:at[n, v] + 1])[0], (name, v, n)
    d = geometry.mesh_laplacian(verts, faces)
    same_bits(d["weight"], lap[0], name)
    dense = geometry.laplacian_matrix(d).to_dense()
    assert dense.shape == (verts.shape[0],) * 2 and torch.equal(dense, dense.T)
    want = np.zeros(dense.shape)
    want[ev, en] = w[:len(ev)]
    want[np.arange(len(want)), np.arange(len(want))] = -lap[1].numpy()
    assert np.array_equal(dense.numpy(), want)
    # the diagonal is an ordered sum of deg terms: deg - 1 roundings of partial sums that are at most the sum of the magnitudes; the
    # row sum is taken with fsum so that only the diagonal's rounding is left
    for v in range(len(want)):
        row = w[start[v]:start[v + 1]]
        assert abs(math.fsum(dense[v].tolist())) <= max(len(row) - 1, 0) * 2.0 ** -53 * float(np.abs(row).sum()), (name, v)


# ---- 3: linear precision ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["jgrid9_0", "jgrid33_1"])
def test_linear_precision_on_planar_meshes(name):
    """A planar mesh has no mean curvature: L p = 0 at interior vertices, to rounding.  The bound 2^-52 c sum |w| |q - p| counts the
    roundings on the longest chain from the inputs to y: edge vector 1, dot product 1 + 2, cross product 1 + 1 (its edge vectors are
    the dot's), nn 1 + 2, sqrt 1, cot's division 1, the sum of an edge's two cotangents 1 (the halving is exact), q - p 1, w (q - p)
    1: 15, and the ordered sum over the entries valence - 1 more."""
    from arah_release_amd import meshing
    verts, faces = mesh(name)
    adj, lap, _ = spec(name)
    assert counts_of(lap)["degenerate"] == 0 and counts_of(lap)["faces"] == faces.shape[0]
    y = meshing.laplacian_apply(lap[0], adj, verts).numpy()
    start, nbr, w, p = adj[2].numpy(), adj[3].numpy(), lap[0].numpy(), verts.double().numpy()
    interior = np.nonzero((adj[6].numpy() & 1) == 0)[0]
    assert len(interior) == (int(name[5:].split("_")[0]) - 2) ** 2
    c = 15 + int(adj[7][5]) - 1
    worst = 0.0
    for v in interior:
        rows = slice(start[v], start[v + 1])
        scale = float((np.abs(w[rows])[:, None] * np.abs(p[nbr[rows]] - p[v])).sum(0).max())
        worst = max(worst, float(np.abs(y[v]).max()) / (2.0 ** -52 * scale))
        assert np.abs(y[v]).max() <= 2.0 ** -52 * c * scale, (name, v, y[v], scale)
    one = {"lamb": 0.5, "method": "laplacian", "boundary": "pin"}
    cot = meshing.mesh_smooth(verts, faces, 1, weights="cotangent", **one)
    uni = meshing.mesh_smooth(verts, faces, 1, **one)
    move_cot = float((cot - verts).abs().max())
    move_uni = float((uni - verts)[interior].abs().max())
    print("%s: |L p| at most %.2f of 2^-52 sum |w| |q - p| (c = %d); one lamb = 0.5 step moves an interior vertex by at most %.3g "
          "(cotangent) against %.3g (uniform), ratio %.3g" % (name, worst, c, move_cot, move_uni, move_uni / max(move_cot, 1e-300)))
    # float32 rounding of a coordinate below the grid's size n: half an ulp, and as much again for the residual of L p
    n = float(verts.abs().max())
    assert move_cot <= 2.0 ** -23 * n
    # the uniform step moves by a fraction of a cell (the jitter is a quarter of one): six orders of magnitude more
    assert move_uni > 0.01 and move_uni > 1e4 * move_cot


# ---- 4: the masses partition the area -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mass", MASSES)
@pytest.mark.parametrize("name", HOST + ("ico2",))
def test_vertex_areas_sum_to_the_area(name, mass):
    verts, faces = mesh(name)
    _, lap, _ = spec(name, mass)
    valid = adjacency_np(faces.numpy(), verts.shape[0])[0]
    total = []
    for f in range(faces.shape[0]):
        if valid[f]:
            with np.errstate(all="ignore"):
                state, A2, _, _ = numpy_face(verts.numpy().astype(np.float64)[faces[f].numpy()])
            if state == 0:
                total.append(A2 * 0.5)
    want, got = math.fsum(total), math.fsum(lap[2].tolist())
    assert len(total) == counts_of(lap)["faces"] and want > 0
    assert abs(got - want) <= verts.shape[0] * 2.0 ** -52 * want, (name, mass, got, want, (got - want) / want * 2.0 ** 52)


# ---- 5: Gauss-Bonnet -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tetrahedron", "octahedron", "sphere17", "torus", "open_sphere", "sheet"])
def test_gauss_bonnet(name):
    from arah_release_amd import geometry
    verts, faces = mesh(name)
    adj, lap, _ = spec(name)
    euler = geometry.mesh_topology(verts, faces)["euler"]
    assert name == "open_sphere" or euler == {"tetrahedron": 2, "octahedron": 2, "sphere17": 2, "torus": 0, "sheet": 1}[name]
    boundary = (adj[6].numpy() & 1) != 0
    defect = np.where(boundary, math.pi, 2.0 * math.pi) - lap[3].numpy()
    defect = defect[(adj[6].numpy() & 4) == 0]                                    # mesh_topology's euler leaves the isolated vertices out
    total = math.fsum(defect.tolist())
    # every corner angle within the atan2 allowance; every vertex's ordered sum of deg angles and its subtraction from (2) pi
    # round deg times at a magnitude below 8; 2 pi euler and the V constants carry the rounding of pi itself
    deg = (adj[0][1:] - adj[0][:-1]).numpy()
    tol = 3 * faces.shape[0] * ATAN2_TERM + float(deg.sum()) * 2.0 ** -50 + (verts.shape[0] + abs(euler)) * 2.0 ** -51
    print("%s: sum of defects - 2 pi euler = %.3g (allowed %.3g)" % (name, total - 2.0 * math.pi * euler, tol))
    assert abs(total - 2.0 * math.pi * euler) <= tol


# ---- 6: the sphere ---------------------------------------------------------------------------------------------------------------------
def test_curvatures_converge_on_refined_spheres():
    from arah_release_amd import meshing
    r, rows = 0.75, []
    for level in (2, 3, 4):
        verts, faces = mesh("ico%d" % level)
        _, _, (curv, _, valid, _) = spec("ico%d" % level)
        assert bool(valid.all()) and verts.shape[0] == 10 * 4 ** level + 2
        eh, eg = (curv[:, 1] - 1.0 / r).abs() * r, (curv[:, 2] - 1.0 / r ** 2).abs() * r ** 2
        rows.append((float(eh.median()), float(eh.max()), float(eg.median()), float(eg.max())))
        print("icosphere level %d (V = %d): |mean_abs - 1/r| r median %.3g worst %.3g; |gaussian - 1/r^2| r^2 median %.3g worst %.3g"
              % ((level, verts.shape[0]) + rows[-1]))
        assert bool((curv[:, 0] > 0).all()) and bool((curv[:, 3] >= curv[:, 4]).all())      # counter-clockwise faces: convex, mean > 0
    for a, b in zip(rows, rows[1:]):
        assert all(y < x for x, y in zip(a, b)), rows
    verts, faces = mesh("ico2")
    flipped = meshing.mesh_curvature(verts, faces.flip(1))[0]
    same_bits(flipped[:, 1:3], spec("ico2")[2][0][:, 1:3], "orientation-free")
    assert bool((flipped[:, 0] < 0).all()) and torch.allclose(flipped[:, 0], -spec("ico2")[2][0][:, 0], rtol=1e-12, atol=0)


# ---- 7: known answers -----------------------------------------------------------------------------------------------------------------
def test_regular_solids_by_hand():
    for name, angle, cot_sum in (("tetrahedron", math.pi, 2.0 / math.sqrt(3.0)), ("octahedron", 4.0 * math.pi / 3.0, 2.0 / math.sqrt(3.0))):
        verts, faces = mesh(name)
        for mass in MASSES:
            adj, lap, (curv, _, valid, _) = spec(name, mass)
            E = int(adj[2][-1])
            assert counts_of(lap) == dict(zip(NAMES, (faces.shape[0], 0, 0, 0, 0, 0))) and bool(valid.all())
            assert np.allclose(lap[3].numpy(), angle, rtol=0, atol=4 * ATAN2_TERM)
            assert len(set(bits(lap[0][:E]).tolist())) == 1 and abs(float(lap[0][0]) - 0.5 * cot_sum) <= 2.0 ** -51
            assert np.allclose((curv[:, 2] * lap[2]).numpy(), 2.0 * math.pi - angle, rtol=0, atol=2.0 ** -45)
            assert len(set(lap[2].tolist())) == 1                                 # both masses give every vertex the same cell


def test_kite_has_one_negative_edge():
    _, lap, (curv, _, valid, _) = spec("kite")
    c = counts_of(lap)
    assert c["negative_edges"] == 1 and c["obtuse"] == 2 and c["faces"] == 2
    assert float(lap[0][0]) < 0                                                   # the entry (0, 1): the long diagonal
    # planar: the mean-curvature normal of these boundary vertices lies in the plane, so the signed mean curvature is exactly 0
    assert bool(valid.all()) and bool((curv[:, 0] == 0).all()) and bool((curv[:, 2] != 0).all())


def test_fin_vertices_are_invalid():
    verts, faces = mesh("fin")
    adj, lap, (curv, mean_normal, valid, n_bad) = spec("fin")
    assert valid.tolist() == [0, 1, 0, 1, 1, 1, 1] and int(n_bad) == 2 and bool((adj[6][[0, 2]] & 2).all())
    assert bool(torch.isnan(curv[[0, 2]]).all()) and bool(torch.isnan(mean_normal[[0, 2]]).all())
    assert bool(torch.isfinite(curv[valid.bool()]).all())
    # the fin's edge carries three cotangents
    row = int(adj[2][0]) + adj[3][int(adj[2][0]):int(adj[2][1])].tolist().index(2)
    assert float(lap[0][row]) > float(spec("octahedron")[1][0][0])


def test_nan_vertex_spoils_its_faces_only():
    verts, faces = mesh("nan_vertex")
    adj, lap, (curv, _, valid, _) = spec("nan_vertex")
    around = int((faces == 11).any(1).sum())
    assert counts_of(lap)["nonfinite"] == around > 0 and counts_of(lap)["faces"] == faces.shape[0] - around
    assert bool(torch.isfinite(lap[0]).all()) and bool(torch.isfinite(lap[2]).all()) and bool(torch.isfinite(lap[3]).all())
    nbrs = adj[3][int(adj[2][11]):int(adj[2][12])].long()
    assert valid[11] == 0 and bool(valid[nbrs].all()) and bool(torch.isfinite(curv[nbrs]).all()) and float(lap[2][11]) == 0.0
    assert int(valid.sum()) == verts.shape[0] - 1


# ---- 8: smoothing ----------------------------------------------------------------------------------------------------------------------
def test_smoothing_keeps_what_it_must():
    from arah_release_amd import geometry, meshing
    verts, faces = mesh("nan_vertex")
    same_bits(meshing.mesh_smooth(verts, faces, 0, weights="cotangent"), verts, "no iteration")
    same_bits(geometry.smooth_mesh(verts, faces, iterations=0, weights="cotangent"), verts, "no iteration")
    out = meshing.mesh_smooth(verts, faces, 2, weights="cotangent")
    assert bits(out[11]).tolist() == bits(verts[11]).tolist() and not torch.equal(out[:11], verts[:11])
    verts, faces = mesh("open_sphere")
    flags = meshing.mesh_adjacency(faces, verts.shape[0])[6]
    pinned, free = (flags & 3) != 0, (flags & 7) == 0                             # the faces taken out left isolated vertices
    out = meshing.mesh_smooth(verts, faces, 2, weights="cotangent")
    assert pinned.any() and torch.equal(out[~free], verts[~free]) and bool((out[free] != verts[free]).any(1).all())
    assert not torch.equal(meshing.mesh_smooth(verts, faces, 2, weights="cotangent", boundary="free")[pinned], verts[pinned])
    for how in ({}, {"method": "laplacian", "lamb": 0.3}, {"boundary": "free"}):
        same_bits(meshing.mesh_smooth(verts, faces, 3, weights="uniform", **how), meshing.mesh_smooth(verts, faces, 3, **how), how)
        same_bits(geometry.smooth_mesh(verts, faces, 3, weights="uniform", **how), geometry.smooth_mesh(verts, faces, 3, **how), how)
    same_bits(geometry.smooth_mesh(verts, faces, 2, weights="cotangent"), out, "geometry")


def test_public_surface_on_the_host():
    from arah_release_amd import geometry, meshing
    verts, faces = mesh("open_sphere")
    adj, lap, (curv, mean_normal, valid, n_bad) = spec("open_sphere")
    d = geometry.mesh_laplacian(verts, faces)
    assert set(d) >= {"weight", "diag", "area", "angle_sum", "adjacency", "report"} and d["report"] == counts_of(lap)
    res = geometry.mesh_curvature(verts, faces, laplacian=d)
    assert set(res) == {"mean", "mean_abs", "gaussian", "k1", "k2", "mean_normal", "area", "valid", "report"}
    for i, key in enumerate(meshing.CURVATURE_FIELDS):
        same_bits(res[key], curv[:, i], key)
    same_bits(res["mean_normal"], mean_normal, "mean_normal")
    isolated = int(((adj[6] & 4) != 0).sum())
    assert res["valid"].dtype == torch.bool and res["report"]["invalid_vertices"] == int(n_bad) == isolated == d["report"]["bad_area"]
    same_bits(geometry.mesh_curvature(verts, faces)["gaussian"], curv[:, 2], "built inside")
    x = verts[:, 0].double()
    same_bits(geometry.apply_laplacian(d, x), meshing.laplacian_apply(lap[0], adj, x[:, None])[:, 0], "apply")
    norm = geometry.laplacian_matrix(d, "normalized").to_dense()
    has_area = d["area"] > 0                                                      # the isolated vertices' rows are 0 / 0
    assert torch.equal(norm[has_area], (geometry.laplacian_matrix(d).to_dense() / d["area"][:, None])[has_area])
    assert geometry.check_smooth({"weights": "cotangent", "iterations": 2}) == {"weights": "cotangent", "iterations": 2}
    bary = geometry.mesh_laplacian(verts, faces, mass="barycentric")
    same_bits(bary["weight"], d["weight"], "the mass does not touch the weights")
    assert not torch.equal(bary["area"], d["area"])


# ---- 9: arguments ------------------------------------------------------------------------------------------------------------------------
def test_argument_checks():
    from arah_release_amd import geometry, meshing
    verts, faces = mesh("octahedron")
    adj, lap, _ = spec("octahedron")
    for bad in ("voronoi", 1, None):
        with pytest.raises(ValueError):
            meshing.mesh_cotangent(verts, faces, bad)
        with pytest.raises(ValueError):
            geometry.mesh_curvature(verts, faces, mass=bad)
    with pytest.raises(ValueError):
        meshing.mesh_cotangent(verts.double(), faces)
    with pytest.raises(ValueError):
        meshing.mesh_cotangent(verts, faces, adjacency=adj[:7])
    for x in (verts[:5], verts[:, 0], torch.zeros(6, 33), torch.zeros(6, 0), torch.zeros(6, 2, dtype=torch.float16), torch.zeros(6, 2).long()):
        with pytest.raises(ValueError):
            meshing.laplacian_apply(lap[0], adj, x)
    with pytest.raises(ValueError):
        meshing.laplacian_apply(lap[0].float(), adj, verts)
    with pytest.raises(ValueError):
        meshing.laplacian_apply(lap[0][:-1], adj, verts)
    for bad in ({"weights": "cotan"}, {"weights": None}, {"weights": "cotangent", "method": "tangential"}):
        with pytest.raises(ValueError):
            geometry.smooth_mesh(verts, faces, 1, **bad)
        with pytest.raises(ValueError):
            geometry.check_smooth(bad)
    with pytest.raises(ValueError):
        meshing.mesh_smooth(verts, faces, 1, weights="cot")
    with pytest.raises(ValueError):
        geometry.laplacian_matrix(geometry.mesh_laplacian(verts, faces), "mass")
    with pytest.raises(ValueError):
        geometry.laplacian_matrix({"weight": lap[0]})
    for v, f in ((verts[:0], faces[:0]), (verts, faces[:0]), (verts[:0], faces)):
        out = meshing.mesh_cotangent(v, f)
        assert out[0].shape == (6 * f.shape[0],) and not out[0].any() and out[4].tolist() == [0, 0, 0, 0, 0, v.shape[0], 0, 0]
        curv, _, valid, n_bad = meshing.mesh_curvature(v, f)
        assert curv.shape == (v.shape[0], 5) and not valid.any() and int(n_bad) == v.shape[0] and bool(torch.isnan(curv).all())
        assert geometry.laplacian_matrix(geometry.mesh_laplacian(v, f)).shape == (v.shape[0],) * 2
        same_bits(meshing.mesh_smooth(v, f, 2, weights="cotangent"), v, "empty")


def test_abi_is_declared_and_checks_its_arguments():
    import ctypes as C
    from arah_release_amd import hip, meshing
    with open(os.path.join(REPO, "include", "arah_hip.h")) as fh:
        declared = set(re.findall(r"\b(arah_\w+)\s*\(", fh.read()))
    lib = hip.load_library()
    for name in NEW_EXPORTS:
        assert name in declared and name in hip.EXPORTS and hasattr(lib, name), name
    assert len(hip.EXPORTS) == len(set(hip.EXPORTS))
    with open(os.path.join(REPO, "arah_release_amd", "csrc", "meshlaplace.hpp")) as fh:
        text = fh.read()
    assert "%.15f" % meshing.TWO_PI in text and "%.15f" % meshing.PI in text and meshing.TWO_PI == 2.0 * math.pi and meshing.PI == math.pi
    size = lib.arah_mesh_smooth_cotangent_scratch_bytes
    assert size(10, 10) >= 6 * 10 * 8 + 32 and size(0, 0) > 0 and size(10, 10) % 256 == 0
    for sizes in ((-1, 0), (0, -1), (2 ** 31, 0), (0, 2 ** 28 + 1)):
        assert size(*sizes) == 0
    p = C.c_void_p(256)                                                           # never dereferenced: every call is refused
    i64, i32 = C.c_int64, C.c_int32

    def cot(V=4, F=4, mass=1, verts=p, start=p, counts=p, out=p):
        return lib.arah_mesh_cotangent(verts, i64(V), p, i64(F), start, p, start, p, i32(mass), out, out, out, out, counts, None)
    for bad in ({"V": -1}, {"F": -1}, {"F": 2 ** 28 + 1}, {"mass": 2}, {"mass": -1}, {"verts": None}, {"start": None}, {"counts": None},
                {"out": None}):
        assert cot(**bad) == -1, bad                                              # ARAH_E_BADARG, nothing launched

    def apply(V=4, F=4, n_ch=3, is64=0, x=p, y=p, w=p, start=p):
        return lib.arah_mesh_laplacian_apply(w, start, p, i64(V), i64(F), x, i32(is64), i32(n_ch), y, None)
    for bad in ({"V": -1}, {"F": -1}, {"n_ch": 0}, {"n_ch": 33}, {"is64": 2}, {"x": None}, {"y": None}, {"w": None}, {"start": None}):
        assert apply(**bad) == -1, bad

    def curvature(V=4, F=4, verts=p, out=p, counts=p, start=p):
        return lib.arah_mesh_curvature(verts, i64(V), i64(F), start, p, p, p, p, p, p, out, out, out, counts, None)
    for bad in ({"V": -1}, {"F": 2 ** 28 + 1}, {"verts": None}, {"out": None}, {"counts": None}, {"start": None}):
        assert curvature(**bad) == -1, bad

    def smooth(V=4, F=4, steps=2, factors=(0.5, -0.53), verts=p, tmp=p, out=p, scratch=p, nbytes=1 << 30):
        return lib.arah_mesh_smooth_cotangent(verts, i64(V), p, i64(F), p, p, p, p, p, i32(steps), (C.c_float * 2)(*factors), i32(1), tmp, out,
                                              scratch, C.c_size_t(nbytes), None)
    for bad in ({"V": -1}, {"F": -1}, {"steps": -1}, {"factors": (float("nan"), 0.5)}, {"verts": None}, {"tmp": None}, {"out": None},
                {"scratch": None}):
        assert smooth(**bad) == -1, bad
    assert smooth(nbytes=16) == -3                                                # ARAH_E_WORKSPACE
