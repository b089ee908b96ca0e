"""Edge-collapse decimation on the host: the tensor specification meshing.mesh_collapse_round against a numpy float64 restatement
written with python loops (bit for bit: positions, keys, reasons, selection, outputs), the properties the rule must have (the
smallest closed meshes, a planar grid, pinned rims), geometry.decimate_mesh keeping closed surfaces closed, the composition of
vert_src / face_src, and the argument checks.  Everything here runs on the host; tests/test_mesh_collapse_gpu.py holds the
kernels of csrc/meshcollapse.hpp to the specification."""
import math
import os
import re

import numpy as np
import pytest
import torch

from test_mesh_quadric import flat_grid, mesh as quadric_mesh, sphere_field

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("arah_mesh_collapse_round_scratch_bytes", "arah_mesh_collapse_round")
NAMES = ("n_verts", "n_faces", "selected", "applied", "candidates", "pinned", "link", "long_edges", "nonfinite", "over_error", "flips",
         "fallbacks")
MAX_UNION = 32
_MESH, _SPEC = {}, {}


# ---- meshes -------------------------------------------------------------------------------------------------------------------------
def torus_field(n, R=0.55, r=0.25):
    ax = torch.linspace(-1, 1, n)
    X, Y, Z = torch.meshgrid(ax, ax, ax, indexing="ij")
    return torch.sqrt((torch.sqrt(X ** 2 + Y ** 2) - R) ** 2 + Z ** 2) - r


def two_spheres_field(n, radius=0.3):
    ax = torch.linspace(-1, 1, n)
    X, Y, Z = torch.meshgrid(ax, ax, ax, indexing="ij")
    return torch.minimum(torch.sqrt((X - 0.45) ** 2 + Y ** 2 + Z ** 2), torch.sqrt((X + 0.45) ** 2 + Y ** 2 + Z ** 2)) - radius


def int_grid(n):
    """n x n unit quads in the plane z = 0 over [0, n]^2, two triangles each: integer coordinates."""
    verts, faces = flat_grid(n)
    verts = verts * n
    verts[:, 2] = 0.0
    return verts.round(), faces


def wavy_sheet(n):
    """An open sheet that is not flat: the rim is a boundary, the inside a surface with curvature."""
    verts, faces = flat_grid(n)
    verts = verts.clone()
    verts[:, 2] = 0.1 * torch.sin(5.0 * verts[:, 0]) * torch.cos(4.0 * verts[:, 1])
    return verts, faces


def bicone(n):
    """Two apexes (0 and 1) over an n-gon equator: the apexes have n neighbours, the equator four."""
    ang = torch.arange(n, dtype=torch.float64) * (2.0 * math.pi / n)
    ring = torch.stack([torch.cos(ang), torch.sin(ang), 0.05 * torch.sin(3.0 * ang)], 1)
    verts = torch.cat([torch.tensor([[0.0, 0.0, 0.7], [0.0, 0.0, -0.6]], dtype=torch.float64), ring]).float()
    i = torch.arange(n)
    a, b = 2 + i, 2 + (i + 1) % n
    return verts, torch.cat([torch.stack([torch.zeros_like(i), a, b], 1), torch.stack([torch.ones_like(i), b, a], 1)])


def solid(name):
    if name == "tetrahedron":
        v = [[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]]
        f = [[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]]
    elif name == "octahedron":
        v = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]
        f = [[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]]
    else:                                                                         # two tetrahedra on the face (0, 1, 2)
        v = [[1, 0, 0], [-0.5, 0.8, 0], [-0.5, -0.9, 0], [0.1, 0, 1.1], [0, 0.1, -0.9]]
        f = [[0, 1, 3], [1, 2, 3], [2, 0, 3], [1, 0, 4], [2, 1, 4], [0, 2, 4]]
    return torch.tensor(v, dtype=torch.float32), torch.tensor(f)


def mesh(name):
    """(verts (V,3) float32, faces (F,3) int64) of a named mesh on the host, computed once and shared; never modified."""
    from arah_release_amd import meshing
    if name not in _MESH:
        if name.startswith("sphere") and name[6:].isdigit():
            verts, faces = quadric_mesh(name) if name in ("sphere17", "sphere33") else meshing.marching_cubes_indexed(
                sphere_field(int(name[6:])))[:2]
        elif name == "torus":
            verts, faces = meshing.marching_cubes_indexed(torus_field(25))[:2]
        elif name == "two_spheres":
            verts, faces = meshing.marching_cubes_indexed(two_spheres_field(25))[:2]
        elif name.startswith("grid"):
            verts, faces = int_grid(int(name[4:]))
        elif name == "sheet":
            verts, faces = wavy_sheet(13)
        elif name.startswith("bicone"):
            verts, faces = bicone(int(name[6:]))
        elif name == "three_faces":                                              # a fin on an edge of the sphere: three faces there
            verts, faces = mesh("sphere17")
            a, b = int(faces[40, 0]), int(faces[40, 1])
            verts = torch.cat([verts, (verts[a:a + 1] + verts[b:b + 1]) * 0.7])
            faces = torch.cat([faces[:60], torch.tensor([[a, b, verts.shape[0] - 1]]), faces[60:]])
        elif name == "nan_vertex":
            verts, faces = mesh("sphere17")
            verts = verts.clone()
            verts[11, 1] = float("nan")
        elif name == "bad_ids":
            verts, faces = mesh("sphere17")
            V, a, b = verts.shape[0], int(faces[40, 0]), int(faces[40, 1])
            more = torch.tensor([[3, 4, V + 7], [-1, 8, 9], [a, a, b], [5, V, int(faces[0, 2])]], dtype=faces.dtype)
            faces = torch.cat([faces[:100], more, faces[100:]])
        else:
            verts, faces = solid(name)
        _MESH[name] = (verts.contiguous(), faces.contiguous())
    return _MESH[name]


def shaped(kind):
    """Two shapes for the round tests on the device.  whole_waves: grid10, 640 = 10 x 64 neighbour entries (every other case leaves
    a part of a wave).  isolated: grid8 between two vertices that no face names, the first id and the last."""
    verts, faces = mesh("grid10" if kind == "whole_waves" else "grid8")
    if kind == "isolated":
        verts, faces = torch.cat([verts[:1] + 0.25, verts, verts[-1:] + 0.25]), faces + 1
    return verts, faces


def spec(name, need=10 ** 6, reg=1e-3, max_cost=float("inf")):
    """meshing.mesh_collapse_round of a case on the host with its details, computed once and shared; never modified."""
    from arah_release_amd import meshing
    key = (name, need, reg, max_cost)
    if key not in _SPEC:
        _SPEC[key] = meshing.mesh_collapse_round(*mesh(name), need, reg, max_cost, details=True)
    return _SPEC[key]


def counts_of(out):
    c = dict(zip(NAMES, out[4].tolist()))
    return dict(c, edges=sum(c[k] for k in NAMES[4:11]))


# ---- an independent restatement ---------------------------------------------------------------------------------------------------
def numpy_round(verts, faces, need, reg, max_cost=np.inf):
    """The rule once more with python loops and numpy float64 scalars.  -> the five outputs and edge_pos, edge_key, edge_reason,
    selected, as arrays."""
    v32 = np.asarray(verts, np.float32)
    v64, faces = v32.astype(np.float64), np.asarray(faces, np.int64)
    V, F = v64.shape[0], faces.shape[0]
    reg, max_cost = np.float64(reg), np.float32(max_cost)
    valid = [all(0 <= i < V for i in f) and len(set(f.tolist())) == 3 for f in faces]
    vf = [[] for _ in range(V)]
    out_n, in_n = [dict() for _ in range(V)], [dict() for _ in range(V)]
    for f in range(F):
        if valid[f]:
            a, b, c = (int(i) for i in faces[f])
            for s, d in ((a, b), (b, c), (c, a)):
                out_n[s][d] = out_n[s].get(d, 0) + 1
                in_n[d][s] = in_n[d].get(s, 0) + 1
            for i in (a, b, c):
                vf[i].append(f)                                                   # ascending by construction
    nbr = [sorted(set(out_n[x]) | set(in_n[x])) for x in range(V)]
    start = np.concatenate([[0], np.cumsum([len(n) for n in nbr])]).astype(np.int64)
    pinned = [not np.isfinite(v32[x]).all() or not nbr[x] or any(out_n[x].get(n, 0) != 1 or in_n[x].get(n, 0) != 1 for n in nbr[x])
              for x in range(V)]
    edge_pos = np.zeros((6 * F, 3), np.float32)
    edge_key = np.full(6 * F, -1, np.int64)
    edge_reason = np.full(6 * F, 255, np.uint8)
    fallbacks, edges = 0, []
    with np.errstate(all="ignore"):
        for u in range(V):
            for k, v in enumerate(nbr[u]):
                if v <= u:
                    continue
                i = int(start[u]) + k
                edges.append((i, u, v))
                if pinned[u] or pinned[v]:
                    edge_reason[i] = 1
                    continue
                shared = [f for f in vf[u] if f in vf[v]]
                a, b = (int(faces[f].sum()) - u - v for f in shared)              # exactly two: one face each way
                common = [n for n in nbr[u] if n in nbr[v]]
                if a == b or len(common) != 2 or len(nbr[a]) < 4 or len(nbr[b]) < 4:
                    edge_reason[i] = 2
                    continue
                union = sorted(set(vf[u]) | set(vf[v]))
                n = len(union)
                assert n == len(vf[u]) + len(vf[v]) - 2
                if n > MAX_UNION:
                    edge_reason[i] = 3
                    continue
                m = (v64[u] + v64[v]) * 0.5
                x = []
                for f in union:
                    pa, pb, pc = (v64[faces[f, j]] - m for j in range(3))
                    e1, e2 = pb - pa, pc - pa
                    nx = e1[1] * e2[2] - e1[2] * e2[1]
                    ny = e1[2] * e2[0] - e1[0] * e2[2]
                    nz = e1[0] * e2[1] - e1[1] * e2[0]
                    d = -((nx * pa[0] + ny * pa[1]) + nz * pa[2])
                    x.append(np.array([nx * nx, nx * ny, nx * nz, ny * ny, ny * nz, nz * nz, nx * d, ny * d, nz * d, d * d]))
                stride = 1
                while stride < n:
                    for j in range(0, n, 2 * stride):
                        if j + stride < n:
                            x[j] = x[j] + x[j + stride]
                    stride *= 2
                A00, A01, A02, A11, A12, A22, b0, b1, b2, c = x[0]
                cell = np.abs(v64[u] - v64[v]).max()
                y = None
                t = (A00 + A11) + A22
                if np.isfinite(t) and t > 0:
                    lam = reg * t
                    M00, M11, M22, M01, M02, M12 = A00 + lam, A11 + lam, A22 + lam, A01, A02, A12
                    C00 = M11 * M22 - M12 * M12
                    C01 = M02 * M12 - M01 * M22
                    C02 = M01 * M12 - M02 * M11
                    C11 = M00 * M22 - M02 * M02
                    C12 = M01 * M02 - M00 * M12
                    C22 = M00 * M11 - M01 * M01
                    det = (M00 * C00 + M01 * C01) + M02 * C02
                    if np.isfinite(det) and det > 0:
                        y = [-((C00 * b0 + C01 * b1) + C02 * b2) / det, -((C01 * b0 + C11 * b1) + C12 * b2) / det,
                             -((C02 * b0 + C12 * b1) + C22 * b2) / det]
                        if not all(np.isfinite(ya) and abs(ya) <= cell for ya in y):
                            y = None
                if y is None:
                    fallbacks += 1
                    y = [np.float64(0.0)] * 3
                    pos = m.astype(np.float32)
                else:
                    pos = np.array([np.float32(m[a_] + y[a_]) for a_ in range(3)], np.float32)
                edge_pos[i] = pos
                Ay0 = (A00 * y[0] + A01 * y[1]) + A02 * y[2]
                Ay1 = (A01 * y[0] + A11 * y[1]) + A12 * y[2]
                Ay2 = (A02 * y[0] + A12 * y[1]) + A22 * y[2]
                raw = (((y[0] * Ay0 + y[1] * Ay1) + y[2] * Ay2) + 2.0 * ((b0 * y[0] + b1 * y[1]) + b2 * y[2])) + c
                if not np.isfinite(np.float32(raw)):
                    edge_reason[i] = 4
                    continue
                cost32 = np.float32(raw) if raw > 0 else np.float32(0.0)
                if cost32 > max_cost:
                    edge_reason[i] = 5
                    continue
                flipped = False
                for f in union:
                    if f in shared:
                        continue
                    p = [v64[faces[f, j]].copy() for j in range(3)]
                    q = [pos.astype(np.float64) if int(faces[f, j]) in (u, v) else p[j] for j in range(3)]
                    N, N2 = cross(p), cross(q)
                    if not (N[0] * N2[0] + N[1] * N2[1]) + N[2] * N2[2] > 0:
                        flipped = True
                if flipped:
                    edge_reason[i] = 6
                    continue
                edge_reason[i] = 0
                edge_key[i] = (int(np.array(cost32, np.float32).view(np.int32)) << 32) | i
    EMPTY = 2 ** 63 - 1
    m1 = [EMPTY] * V
    for i, u, v in edges:
        if edge_reason[i] == 0:
            m1[u], m1[v] = min(m1[u], int(edge_key[i])), min(m1[v], int(edge_key[i]))
    m2 = [min([m1[x]] + [m1[n] for n in nbr[x]]) for x in range(V)]
    selected = np.zeros(6 * F, bool)
    chosen = []
    for i, u, v in edges:                                                         # ascending edge id
        if edge_reason[i] == 0 and m2[u] == m2[v] == int(edge_key[i]):
            selected[i] = True
            chosen.append((i, u, v))
    applied = chosen[:need]
    merge_to, moved, src = list(range(V)), v32.copy(), list(range(V))
    for i, u, v in applied:
        merge_to[v] = u
        moved[u] = edge_pos[i]
        d2 = []
        for x in (u, v):
            d = v64[x] - edge_pos[i].astype(np.float64)
            d2.append(np.float32((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
        src[u] = v if d2[1] < d2[0] else u
    new_id, verts_out, vert_src = {}, np.zeros((V, 3), np.float32), np.zeros(V, np.int32)
    for x in range(V):
        if merge_to[x] == x:
            new_id[x] = len(new_id)
            verts_out[new_id[x]], vert_src[new_id[x]] = moved[x], src[x]
    faces_out, face_src, nf = np.zeros((F, 3), np.int32), np.zeros(F, np.int32), 0
    for f in range(F):
        ids = [merge_to[i] if 0 <= i < V else i for i in (int(i) for i in faces[f])]
        if valid[f] and len(set(ids)) < 3:
            continue
        faces_out[nf] = [new_id[i] if 0 <= int(faces[f, j]) < V else i for j, i in enumerate(ids)]
        face_src[nf] = f
        nf += 1
    reasons = [int((edge_reason == r).sum()) for r in range(7)]
    counts = np.array([len(new_id), nf, len(chosen), len(applied)] + reasons + [fallbacks], np.int32)
    return verts_out, faces_out, vert_src, face_src, counts, edge_pos, edge_key, edge_reason, selected


def cross(p):
    e1, e2 = p[1] - p[0], p[2] - p[0]
    return [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]


def same_bits(got, want, what, n=None):
    """The first n outputs (all of `want` by default) equal bit for bit."""
    keys = ("verts", "faces", "vert_src", "face_src", "counts", "edge_pos", "edge_key", "edge_reason", "selected")
    for key, g, w in list(zip(keys, got, want))[:n]:
        g, w = np.asarray(g.cpu() if torch.is_tensor(g) else g), np.asarray(w.cpu() if torch.is_tensor(w) else w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, key, g.dtype, w.dtype, g.shape, w.shape)
        if g.dtype == np.float32:
            g, w = g.view(np.int32), w.view(np.int32)
        assert np.array_equal(g, w), (what, key)


def volume(verts, faces):
    p = verts.double()[faces.long()]
    return float((p[:, 0] * torch.linalg.cross(p[:, 1], p[:, 2])).sum() / 6.0)


# ---- 1: the specification is the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,need,reg", [("sphere9", 10 ** 6, 1e-3), ("sphere9", 3, 0.05), ("grid6", 10 ** 6, 1e-3),
                                           ("bad_ids", 10 ** 6, 1e-3), ("nan_vertex", 5, 1e-3), ("bicone40", 10 ** 6, 1e-3)])
def test_specification_is_the_restatement(name, need, reg):
    verts, faces = mesh(name)
    got, want = spec(name, need, reg), numpy_round(verts.numpy(), faces.numpy(), need, reg)
    same_bits(got, want, (name, need, reg))
    c = counts_of(got)
    assert c["candidates"] == int((got[7] == 0).sum()) and c["edges"] == int((got[7] != 255).sum())
    assert c["applied"] == min(c["selected"], need) > 0 and c["n_faces"] == faces.shape[0] - 2 * c["applied"]
    assert not got[0][c["n_verts"]:].any() and not got[1][c["n_faces"]:].any()
    assert not got[2][c["n_verts"]:].any() and not got[3][c["n_faces"]:].any()


def test_bound_on_the_cost_is_the_restatement():
    verts, faces = mesh("sphere9")
    costs = spec("sphere9")[6]
    bound = float((costs[costs >= 0] >> 32).to(torch.int32).view(torch.float32).median())
    got, want = spec("sphere9", 10 ** 6, 1e-3, bound), numpy_round(verts.numpy(), faces.numpy(), 10 ** 6, 1e-3, bound)
    same_bits(got, want, "max_cost")
    assert 0 < counts_of(got)["over_error"] < counts_of(got)["edges"]
    none = spec("sphere9", 10 ** 6, 1e-3, 0.0)                                    # nothing on a sphere costs nothing
    assert counts_of(none)["applied"] == 0 and counts_of(none)["n_faces"] == faces.shape[0]
    same_bits((none[0], none[1].long()), (verts, faces), "nothing applied")


# ---- 2: the smallest closed meshes ------------------------------------------------------------------------------------------------
def test_tetrahedron_has_no_legal_edge():
    c = counts_of(spec("tetrahedron"))
    assert c["edges"] == c["link"] == 6 and c["selected"] == c["applied"] == 0 and c["n_faces"] == 4 and c["n_verts"] == 4


def test_octahedron_by_the_rule():
    """Every edge of the octahedron passes the rule as it is written: the two ends have exactly the two third vertices in common,
    which have four neighbours each, and moving an end to the midpoint turns no face over.  One edge is collapsed (all share a
    neighbourhood), and what is left -- five vertices, six faces, two tetrahedra on a face -- is closed; an apex edge of that goes
    next, and of the tetrahedron that remains no edge may go: its third vertices have three neighbours."""
    from arah_release_amd import geometry, meshing
    out = spec("octahedron")
    c = counts_of(out)
    assert c["edges"] == 12 and c["link"] == c["pinned"] == c["flips"] == 0 and c["selected"] == c["applied"] == 1
    verts, faces = out[0][:c["n_verts"]], out[1][:c["n_faces"]]
    topo = geometry.mesh_topology(verts, faces)
    assert (c["n_verts"], c["n_faces"]) == (5, 6) and topo["watertight"] and topo["manifold"] and topo["euler"] == 2
    out = meshing.mesh_collapse_round(verts, faces, 10)
    again = counts_of(out)
    assert again["applied"] == 1 and again["link"] == 3 and again["edges"] == 9   # the three edges of the middle triangle stay
    last = counts_of(meshing.mesh_collapse_round(out[0][:4], out[1][:4], 10))
    assert (again["n_verts"], again["n_faces"]) == (4, 4) and last["applied"] == 0 and last["link"] == last["edges"] == 6


def test_bipyramid_only_legal_edges_go():
    from arah_release_amd import geometry
    out = spec("bipyramid")
    c, reason = counts_of(out), out[7]
    verts, faces = mesh("bipyramid")
    # the three edges of the shared triangle have the apexes (three neighbours) as third vertices; the six apex edges are legal
    assert c["edges"] == 9 and c["link"] == 3 and c["applied"] == 1
    adj = geometry.mesh_adjacency(verts, faces)
    owner = torch.repeat_interleave(torch.arange(5), adj.nbr_start[1:] - adj.nbr_start[:-1])
    for i in range(int(adj.nbr_start[5])):
        u, v = int(owner[i]), int(adj.nbr[i])
        assert int(reason[i]) == (255 if v <= u else 2 if v < 3 else int(reason[i]))
        if v > u and v >= 3:
            assert int(reason[i]) in (0, 6)
    left = geometry.mesh_topology(out[0][:4], out[1][:4])
    assert c["n_verts"] == 4 and c["n_faces"] == 4 and left["watertight"] and left["euler"] == 2


# ---- 3: a planar grid ----------------------------------------------------------------------------------------------------------------
def test_planar_grid_keeps_rim_plane_and_area():
    from arah_release_amd import meshing
    verts, faces = mesh("grid8")
    rim = ((verts[:, :2] == 0) | (verts[:, :2] == 8)).any(1)
    for _ in range(4):
        out = meshing.mesh_collapse_round(verts, faces, 10 ** 6, details=True)
        c = counts_of(out)
        if c["applied"] == 0:
            break
        keys = out[6][out[8]]
        assert bool((keys >> 32 == 0).all())                                      # interior collapses cost exactly +0
        new_v, new_f, src = out[0][:c["n_verts"]], out[1][:c["n_faces"]].long(), out[2][:c["n_verts"]].long()
        assert bool((new_v[:, 2] == 0).all()) and c["fallbacks"] == 0             # the solve returns the midpoint: z stays 0
        assert torch.equal(new_v[rim[src]], verts[src][rim[src]]) and int(rim[src].sum()) == int(rim.sum())
        p = new_v.double()[new_f]
        area = torch.linalg.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])[:, 2].abs().sum() / 2
        assert float(area) == 64.0 and bool((torch.linalg.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])[:, 2] != 0).all())
        verts, faces, rim = new_v, new_f, rim[src]
    assert faces.shape[0] < 128


# ---- 4: closed surfaces stay closed ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere17", "torus"])
def test_decimate_keeps_the_surface(name):
    from arah_release_amd import geometry
    verts, faces = mesh(name)
    before = geometry.mesh_topology(verts, faces)
    n_comp = geometry.mesh_components(verts, faces)["n_components"]
    target = faces.shape[0] // 4
    weights = torch.arange(verts.shape[0] * 2, dtype=torch.float32).reshape(-1, 2)
    res = geometry.decimate_mesh(verts, faces, target_faces=target, attributes={"weights": weights})
    after = geometry.mesh_topology(res["verts"], res["faces"])
    assert before["watertight"] and after["manifold"] and after["watertight"] and after["euler"] == before["euler"]
    assert before["euler"] == (2 if name == "sphere17" else 0)
    assert geometry.mesh_components(res["verts"], res["faces"])["n_components"] == n_comp == 1
    assert res["n_tris"] in (target, target - 1) and res["report"]["reached"] and res["report"]["target"] == target
    assert res["report"]["faces"][0] == faces.shape[0] and res["report"]["faces"][-1] == res["n_tris"]
    assert len(res["report"]["faces"]) == res["report"]["rounds"] + 1
    v0, v1 = volume(verts, faces), volume(res["verts"], res["faces"])
    assert v0 * v1 > 0 and abs(v1 / v0 - 1) < 0.1
    if name == "sphere17":
        assert geometry.self_intersections(res["verts"], res["faces"])["count"] == 0
    # composition: every output face is its source face with every corner renamed to the vertex that absorbed it
    assert torch.equal(res["weights"], weights[res["vert_src"]]) and res["faces"].dtype == faces.dtype
    assert bool((res["face_src"][1:] > res["face_src"][:-1]).all())
    assert res["vert_src"].unique().numel() == res["n_verts"]
    own = torch.full((verts.shape[0],), -1, dtype=torch.long)
    own[res["vert_src"]] = torch.arange(res["n_verts"])
    kept = faces[res["face_src"]]
    named = own[kept] >= 0                                                        # corners that survive by themselves keep their place
    assert bool(named.any()) and torch.equal(own[kept][named], res["faces"][named])
    # ... and the renaming is ONE map from the input's vertices to the output's: a vertex never lands in two places
    went = torch.full((verts.shape[0],), -1, dtype=torch.long)
    went[kept.reshape(-1)] = res["faces"].reshape(-1)
    assert torch.equal(went[kept], res["faces"])
    seen = went[res["vert_src"]]                                                  # -1: every face of that source went in later rounds
    assert bool(((seen == torch.arange(res["n_verts"])) | (seen < 0)).all()) and int((seen >= 0).sum()) > res["n_verts"] // 2


def test_decimate_composes_its_rounds():
    from arah_release_amd import geometry, meshing
    verts, faces = mesh("sphere17")
    res = geometry.decimate_mesh(verts, faces, ratio=0.5)
    v, f = verts, faces
    vs, fs = torch.arange(verts.shape[0]), torch.arange(faces.shape[0])
    target = faces.shape[0] // 2
    for r in range(res["report"]["rounds"]):
        out = meshing.mesh_collapse_round(v, f, (f.shape[0] - target + 1) // 2)
        c = counts_of(out)
        v, f = out[0][:c["n_verts"]], out[1][:c["n_faces"]].long()
        vs, fs = vs[out[2][:c["n_verts"]].long()], fs[out[3][:c["n_faces"]].long()]
        assert res["report"]["faces"][r + 1] == c["n_faces"]
    same_bits((res["verts"], res["faces"], res["vert_src"], res["face_src"]), (v, f, vs, fs), "rounds")
    # the bound alone, rounds that run out, and a target that is already met
    far = geometry.decimate_mesh(verts, faces, max_error=1e-9)
    assert faces.shape[0] > far["n_tris"] > 0 and far["report"]["over_error"] > 0 and not far["report"]["reached"]
    one = geometry.decimate_mesh(verts, faces, target_faces=4, max_rounds=1)
    assert one["report"]["rounds"] == 1 and not one["report"]["reached"] and len(one["report"]["faces"]) == 2
    same = geometry.decimate_mesh(verts, faces, target_faces=faces.shape[0])
    assert same["report"]["rounds"] == 0 and same["report"]["reached"] and torch.equal(same["verts"], verts)
    assert torch.equal(same["faces"], faces) and torch.equal(same["vert_src"], torch.arange(verts.shape[0]))


def test_open_sheet_keeps_its_rim():
    from arah_release_amd import geometry
    verts, faces = mesh("sheet")
    before = geometry.mesh_topology(verts, faces)
    res = geometry.decimate_mesh(verts, faces, ratio=0.5)
    after = geometry.mesh_topology(res["verts"], res["faces"])
    assert after["boundary_edges"] == before["boundary_edges"] == 52 and after["manifold"] and after["euler"] == before["euler"] == 1
    rim = ((verts[:, :2] == 0) | (verts[:, :2] == 1)).any(1)
    kept_rim = rim[res["vert_src"]]
    assert int(kept_rim.sum()) == int(rim.sum()) and torch.equal(res["verts"][kept_rim], verts[res["vert_src"]][kept_rim])
    assert res["report"]["pinned"] > 0 and res["n_tris"] < faces.shape[0]


# ---- 5: arguments -------------------------------------------------------------------------------------------------------------------
def test_argument_checks():
    from arah_release_amd import geometry, meshing
    verts, faces = mesh("octahedron")
    for bad in ({}, {"target_faces": 4, "ratio": 0.5}, {"target_faces": -1}, {"target_faces": 2.5}, {"target_faces": True},
                {"ratio": 1.5}, {"ratio": float("nan")}, {"max_error": -1.0}, {"ratio": 0.5, "quadric_reg": -1.0},
                {"ratio": 0.5, "max_rounds": -1}, {"ratio": 0.5, "max_rounds": 2.0}, {"ratio": 0.5, "attributes": {"report": verts}},
                {"ratio": 0.5, "attributes": {"w": verts[:3]}}):
        with pytest.raises(ValueError):
            geometry.decimate_mesh(verts, faces, **bad)
    with pytest.raises(ValueError):
        geometry.decimate_mesh(verts.long(), faces, ratio=0.5)
    for bad in ((-1, 1e-3, 1.0), (1.5, 1e-3, 1.0), (1, -1.0, 1.0), (1, float("inf"), 1.0), (1, 1e-3, -1.0), (1, 1e-3, float("nan")),
                (True, 1e-3, 1.0)):
        with pytest.raises(ValueError):
            meshing.mesh_collapse_round(verts, faces, *bad)
    with pytest.raises(ValueError):
        meshing.mesh_collapse_round(verts.double(), faces, 1)
    empty = meshing.mesh_collapse_round(verts[:0], faces[:0], 3)
    assert empty[0].shape == (0, 3) and empty[1].shape == (0, 3) and empty[4].tolist() == [0] * 12
    lone = meshing.mesh_collapse_round(verts, faces[:0], 3)                       # vertices without a face stay
    assert lone[4].tolist() == [6] + [0] * 11 and torch.equal(lone[0], verts) and lone[2].tolist() == list(range(6))
    gone = meshing.mesh_collapse_round(verts[:0], faces, 3)                       # faces without a vertex stay as they are
    assert gone[4].tolist() == [0, 8] + [0] * 10 and torch.equal(gone[1].long(), faces) and gone[3].tolist() == list(range(8))


def test_simplify_option_takes_the_method():
    from arah_release_amd import geometry
    verts, faces = mesh("sphere17")
    kw = geometry.check_simplify({"method": "collapse", "ratio": 0.25, "max_rounds": 50})
    assert kw == {"method": "collapse", "ratio": 0.25, "max_rounds": 50}
    got, want = geometry.apply_simplify(verts, faces, kw), geometry.decimate_mesh(verts, faces, ratio=0.25, max_rounds=50)
    assert torch.equal(got["verts"], want["verts"]) and torch.equal(got["faces"], want["faces"]) and got["report"] == want["report"]
    for bad in ({"method": "collapse"}, {"method": "collapse", "cell": 0.1}, {"method": "collapse", "ratio": 2.0},
                {"method": "collapse", "target_faces": 10, "ratio": 0.5}, {"method": "melt", "ratio": 0.5},
                {"method": "collapse", "ratio": 0.5, "position": "quadric"}, {"method": "cluster", "ratio": 0.5}):
        with pytest.raises(ValueError):
            geometry.check_simplify(bad)
    # without "method", and with the clustering named, nothing changes: the same keywords, the same bits
    how = {"cell": 0.125, "position": "quadric"}
    assert geometry.check_simplify(how) == how == geometry.check_simplify(dict(how, method="cluster"))
    assert geometry.check_simplify(0.25) == {"cell": 0.25}
    a, b = geometry.apply_simplify(verts, faces, geometry.check_simplify(how)), geometry.simplify_mesh(verts, faces, **how)
    assert set(a) == set(b) and torch.equal(a["verts"], b["verts"]) and torch.equal(a["faces"], b["faces"])
    assert torch.equal(a["vert_src"], b["vert_src"]) and a["quadric"] == b["quadric"] and a["removed"] == b["removed"]


def test_abi_is_declared_and_checks_its_arguments():
    import ctypes as C
    from arah_release_amd import hip
    with open(os.path.join(REPO, "include", "arah_hip.h")) as fh:
        declared = set(re.findall(r"\b(arah_\w+)\s*\(", fh.read()))
    lib = hip.load_library()
    for name in NEW_EXPORTS:
        assert name in declared and name in hip.EXPORTS and hasattr(lib, name), name
    assert len(hip.EXPORTS) == len(set(hip.EXPORTS))
    size = lib.arah_mesh_collapse_round_scratch_bytes
    assert size(10, 10) > 0 and size(0, 0) > 0 and size(10, 10) % 256 == 0
    assert size(10, 10) > lib.arah_mesh_adjacency_scratch_bytes(10, 10)          # the adjacency is built inside
    for sizes in ((-1, 0), (0, -1), (2 ** 31, 0), (0, 2 ** 28 + 1)):
        assert size(*sizes) == 0
    p = C.c_void_p(256)                                                           # never dereferenced: every call is refused

    def call(V=4, F=4, need=1, reg=1e-3, max_cost=1.0, counts=p, scratch=p, verts=p, faces=p, out=p, nbytes=1 << 30):
        return lib.arah_mesh_collapse_round(verts, C.c_int64(V), faces, C.c_int64(F), C.c_int32(need), C.c_double(reg),
                                            C.c_float(max_cost), out, out, out, out, counts, out, out, out, scratch,
                                            C.c_size_t(nbytes), None)
    for bad in ({"V": -1}, {"F": -1}, {"F": 2 ** 28 + 1}, {"need": -1}, {"reg": -1.0}, {"reg": float("nan")}, {"max_cost": -1.0},
                {"max_cost": float("nan")}, {"counts": None}, {"scratch": None}, {"verts": None}, {"faces": None}, {"out": None}):
        assert call(**bad) == -1, bad                                             # ARAH_E_BADARG, nothing launched
    assert call(nbytes=16) == -3                                                  # ARAH_E_WORKSPACE
