"""Isotropic remeshing on the host: the tangential step and the bounded collapse round against plain-loop numpy restatements (bit
for bit), geometry.mesh_quality on meshes with known numbers, geometry.isotropic_remesh on a closed marching-cubes sphere (its
topology, the projection onto the input, the attributes, the quality against the input's), smooth_mesh(method="tangential"), and
the argument checks.  Everything here runs on the host; tests/test_mesh_isotropic_gpu.py holds the kernels to the specifications."""
import math
import os
import re

import numpy as np
import pytest
import torch

from test_mesh_collapse import numpy_round as collapse_numpy_round, same_bits as collapse_same_bits
from test_mesh_flip import adjacency_np, mesh

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("arah_mesh_collapse_round_bounded", "arah_mesh_tangential")
_REMESH = {}


def icosahedron():
    g = (1.0 + math.sqrt(5.0)) / 2.0
    v = [[-1, g, 0], [1, g, 0], [-1, -g, 0], [1, -g, 0], [0, -1, g], [0, 1, g], [0, -1, -g], [0, 1, -g], [g, 0, -1], [g, 0, 1],
         [-g, 0, -1], [-g, 0, 1]]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
         [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    return torch.tensor(v, dtype=torch.float32), torch.tensor(f)


def remeshed(name="sphere33"):
    """geometry.isotropic_remesh(iterations=5) of a mesh on the host with two attributes, computed once and shared; never modified."""
    from arah_release_amd import geometry
    if name not in _REMESH:
        verts, faces = mesh(name)
        attrs = {"w": torch.stack([verts[:, 0] * 2.0, verts[:, 1] + verts[:, 2]], 1).double(), "label": torch.arange(verts.shape[0])}
        _REMESH[name] = geometry.isotropic_remesh(verts, faces, iterations=5, attributes=attrs), attrs
    return _REMESH[name]


def edge_bounds(name):
    """(short_len2, long_len2) around the mean edge length of a mesh: 4/5 and 4/3 of it, squared."""
    from arah_release_amd import geometry
    L = geometry.mesh_quality(*mesh(name))["edge_mean"]
    return (0.8 * L) ** 2, (4.0 / 3.0 * L) ** 2


# ---- 1: the tangential step ----------------------------------------------------------------------------------------------------------
def numpy_tangential(verts, faces, normal_sum, lamb):
    v32 = np.asarray(verts, np.float32)
    v64, N = v32.astype(np.float64), np.asarray(normal_sum, np.float64)
    V = v64.shape[0]
    _, _, out_n, in_n, nbr, _ = adjacency_np(np.asarray(faces, np.int64), V)
    lam, out = np.float64(np.float32(lamb)), v32.copy()
    with np.errstate(all="ignore"):
        for x in range(V):
            odd = any(out_n[x].get(n, 0) + in_n[x].get(n, 0) != 2 for n in nbr[x])
            nn = (N[x, 0] * N[x, 0] + N[x, 1] * N[x, 1]) + N[x, 2] * N[x, 2]
            if not np.isfinite(v32[x]).all() or odd or not (np.isfinite(nn) and nn > 0):
                continue
            s, m = np.zeros(3), 0
            for n in nbr[x]:
                if np.isfinite(v32[n]).all():
                    s, m = s + v64[n], m + 1
            if m == 0:
                continue
            d = s / np.float64(m) - v64[x]
            t = ((d[0] * N[x, 0] + d[1] * N[x, 1]) + d[2] * N[x, 2]) / nn
            out[x] = (v64[x] + lam * (d - t * N[x])).astype(np.float32)
    return out


@pytest.mark.parametrize("name", ["sphere9", "sheet", "three_faces", "nan_vertex", "bad_ids", "bicone40"])
def test_tangential_step_is_the_restatement(name):
    from arah_release_amd import meshing
    verts, faces = mesh(name)
    normal_sum = meshing.vertex_normals(verts, faces)[0]
    for lamb in (0.5, 1.0, 0.3):
        got = meshing.mesh_tangential_step(verts, faces, normal_sum, lamb)
        want = numpy_tangential(verts.numpy(), faces.numpy(), normal_sum.numpy(), lamb)
        assert got.dtype == torch.float32 and np.array_equal(got.numpy().view(np.int32), want.view(np.int32)), (name, lamb)
    moved = (got != verts).any(1)
    adj = meshing.mesh_adjacency(faces, verts.shape[0])
    assert bool(moved.any()) and not bool(moved[(adj[6] & 3) != 0].any())
    zero = torch.zeros_like(normal_sum)                                           # no normal, no move
    assert torch.equal(meshing.mesh_tangential_step(verts, faces, zero)[torch.isfinite(verts).all(1)], verts[torch.isfinite(verts).all(1)])


def test_tangential_smoothing_stays_on_the_sphere():
    from arah_release_amd import geometry, meshing
    verts, faces = mesh("sphere33")
    out = geometry.smooth_mesh(verts, faces, iterations=3, method="tangential")
    v = verts
    for _ in range(3):
        v = meshing.mesh_tangential_step(v, faces, meshing.vertex_normals(v, faces)[0], 0.5)
    assert torch.equal(out, v) and float((out - verts).norm(dim=1).max()) > 0.01
    lap = geometry.smooth_mesh(verts, faces, iterations=3, method="laplacian")
    off = lambda p: float((p.double().norm(dim=1) - 0.8).abs().max())
    print("radius error: input %.2e, tangential %.2e, laplacian %.2e" % (off(verts), off(out), off(lap)))
    assert off(out) < 0.5 * off(lap)
    q0, q1 = geometry.mesh_quality(verts, faces), geometry.mesh_quality(out, faces)
    assert q1["min_angle_mean"] > q0["min_angle_mean"]
    for bad in ({"boundary": "free"}, {"iterations": -1}, {"lamb": 0.0}, {"lamb": 1.5}):
        with pytest.raises(ValueError):
            geometry.smooth_mesh(verts, faces, method="tangential", **bad)
    assert geometry.check_smooth({"method": "tangential", "iterations": 2}) == {"method": "tangential", "iterations": 2}
    # every other method is what it was: the keywords go to the same specification
    assert torch.equal(geometry.smooth_mesh(verts, faces, iterations=2), meshing.mesh_smooth(verts, faces, 2))


# ---- 2: the bounded collapse round -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere9", "bad_ids", "nan_vertex", "sheet"])
def test_without_bounds_the_collapse_round_is_what_it_was(name):
    from arah_release_amd import meshing
    verts, faces = mesh(name)
    plain = meshing.mesh_collapse_round(verts, faces, 10 ** 6, details=True)
    collapse_same_bits(plain, collapse_numpy_round(verts.numpy(), faces.numpy(), 10 ** 6, 1e-3), name)
    assert plain[4].shape == (12,)
    loose = meshing.mesh_collapse_round(verts, faces, 10 ** 6, details=True, short_len2=float("inf"), long_len2=float("inf"))
    assert loose[4].shape == (14,) and int(loose[4][13]) == 0
    if bool(torch.isfinite(verts).all()):
        assert torch.equal(loose[4][:12], plain[4]) and int(loose[4][12]) == 0
        for g, w in zip(loose[:4] + loose[5:], plain[:4] + plain[5:]):
            assert torch.equal(g, w)
    else:                                                                         # an edge without a length is never short: 7, not 1
        moved = int(loose[4][12])
        assert moved > 0 and int(plain[4][5]) == int(loose[4][5]) + moved
        assert torch.equal(loose[4][:5], plain[4][:5]) and torch.equal(loose[4][6:12], plain[4][6:])
        collapse_same_bits(loose, plain, name, n=4)


@pytest.mark.parametrize("name", ["sphere9", "sphere17", "nan_vertex", "sheet"])
def test_bounded_collapse_round_is_the_restatement(name):
    """The tests 1 .. 6 do not read the bounds, so their reasons and positions are the unbounded restatement's; the two new tests
    and the selection are restated here with loops."""
    from arah_release_amd import meshing
    verts, faces = mesh(name)
    short2, long2 = edge_bounds(name)
    got = meshing.mesh_collapse_round(verts, faces, 10 ** 6, details=True, short_len2=short2, long_len2=long2)
    base = collapse_numpy_round(verts.numpy(), faces.numpy(), 10 ** 6, 1e-3)
    v64, fc, V = verts.numpy().astype(np.float64), faces.numpy(), verts.shape[0]
    valid, vf, _, _, nbr, start = adjacency_np(fc, V)
    reason, key = base[7].copy(), base[6].copy()
    edges = []
    with np.errstate(all="ignore"):
        for u in range(V):
            for k, v in enumerate(nbr[u]):
                if v <= u:
                    continue
                i = int(start[u]) + k
                edges.append((i, u, v))
                d = v64[u] - v64[v]
                if not (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] < short2:
                    reason[i], key[i] = 7, -1
                elif reason[i] == 0:
                    pos = base[5][i].astype(np.float64)
                    for f in sorted(set(vf[u]) | set(vf[v])):
                        ids = [int(x) for x in fc[f]]
                        if u in ids and v in ids:
                            continue
                        for x in ids:
                            g = v64[x] - pos
                            if x not in (u, v) and (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2] > long2:
                                reason[i], key[i] = 8, -1
    assert np.array_equal(got[7].numpy(), reason) and np.array_equal(got[6].numpy(), key)
    shown = reason < 7                                                            # position and cost are written before test 8 only
    assert np.array_equal(got[5].numpy()[shown | (reason == 8)].view(np.int32), base[5][shown | (reason == 8)].view(np.int32))
    EMPTY = 2 ** 63 - 1
    m1 = [EMPTY] * V
    for i, u, v in edges:
        if reason[i] == 0:
            m1[u], m1[v] = min(m1[u], int(key[i])), min(m1[v], int(key[i]))
    m2 = [min([m1[x]] + [m1[n] for n in nbr[x]]) for x in range(V)]
    chosen = [i for i, u, v in edges if reason[i] == 0 and m2[u] == m2[v] == int(key[i])]
    assert torch.nonzero(got[8])[:, 0].tolist() == chosen
    c = dict(zip(meshing.COLLAPSE_BOUNDED_COUNTS, got[4].tolist()))
    assert c["selected"] == c["applied"] == len(chosen) and c["n_faces"] == faces.shape[0] - 2 * len(chosen)
    assert got[4][4:11].tolist() + got[4][12:].tolist() == [int((reason == r).sum()) for r in range(9)]
    assert len(meshing.COLLAPSE_BOUNDED_REASONS) == 9 and meshing.COLLAPSE_BOUNDED_COUNTS[12:] == ("not_short", "too_long")
    assert c["not_short"] > 0 and (name != "sphere17" or (c["too_long"] > 0 and c["applied"] > 0))
    # applied: the edges that went were short, and no edge at a new vertex is long
    nv, nf = c["n_verts"], c["n_faces"]
    new_v, new_f = got[0][:nv].double(), got[1][:nf].long()
    moved = torch.zeros(nv, dtype=torch.bool)
    src = got[2][:nv].long()
    for i in chosen:
        moved |= (new_v.float() == got[5][i]).all(1)
    e = torch.cat([new_f[:, [0, 1]], new_f[:, [1, 2]], new_f[:, [2, 0]]])
    e = e[((e >= 0) & (e < nv)).all(1)]
    at_new = moved[e[:, 0]] | moved[e[:, 1]]
    d2 = ((new_v[e[:, 0]] - new_v[e[:, 1]]) ** 2).sum(1)
    assert int(moved.sum()) >= len(chosen) > 0 or len(chosen) == 0
    assert not bool((d2[at_new] > long2 * (1 + 1e-12)).any()) and src.shape[0] == nv


# ---- 3: the yardstick ------------------------------------------------------------------------------------------------------------------
def test_mesh_quality_of_known_meshes():
    from arah_release_amd import geometry
    q = geometry.mesh_quality(*icosahedron())
    assert (q["n_verts"], q["n_faces"], q["n_edges"]) == (12, 20, 30)
    assert abs(q["edge_min"] - 2.0) < 1e-6 and abs(q["edge_max"] - 2.0) < 1e-6 and abs(q["edge_length"] - 2.0) < 1e-6
    assert abs(q["min_angle_min"] - 60.0) < 1e-4 and abs(q["min_angle_mean"] - 60.0) < 1e-4
    assert q["edges_in_range"] == 1.0 and q["small_angle_share"] == 0.0
    assert q["valence6_share"] == 0.0 and q["valence5to7_share"] == 1.0           # twelve vertices of valence five
    far = geometry.mesh_quality(*icosahedron(), edge_length=1.0)
    assert far["edges_in_range"] == 0.0 and far["edge_length"] == 1.0
    verts, faces = mesh("grid8")                                                  # right isosceles triangles
    q = geometry.mesh_quality(verts, faces)
    assert abs(q["min_angle_min"] - 45.0) < 1e-9 and abs(q["min_angle_mean"] - 45.0) < 1e-9 and q["edge_min"] == 1.0
    assert abs(q["edge_max"] - math.sqrt(2.0)) < 1e-12 and q["valence6_share"] == 1.0 and q["small_angle_share"] == 0.0
    dirty = geometry.mesh_quality(*mesh("bad_ids"))
    assert dirty["n_faces"] == mesh("sphere17")[1].shape[0]                       # the four bad rows are skipped
    empty = geometry.mesh_quality(verts[:0], faces[:0])
    assert empty["n_faces"] == 0 and math.isnan(empty["edge_mean"]) and math.isnan(empty["valence6_share"])
    for bad in (0.0, -1.0, float("nan"), True, "long"):
        with pytest.raises(ValueError):
            geometry.mesh_quality(verts, faces, edge_length=bad)


# ---- 4: the remesher ------------------------------------------------------------------------------------------------------------------
def test_remeshed_sphere_is_still_a_sphere():
    from arah_release_amd import geometry
    res, _ = remeshed()
    topo = geometry.mesh_topology(res["verts"], res["faces"])
    assert topo["boundary_edges"] == topo["nonmanifold_edges"] == topo["misoriented_edges"] == 0 and topo["euler"] == 2
    assert topo["skipped_faces"] == 0 and geometry.mesh_components(res["verts"], res["faces"])["n_components"] == 1
    assert res["faces"].dtype == mesh("sphere33")[1].dtype and res["verts"].shape == (res["n_verts"], 3)
    steps = res["report"]["iterations"]
    assert len(steps) == 5 and steps[-1]["faces"] == res["n_tris"] and all(s["splits"] + s["collapses"] + s["flips"] > 0 for s in steps)


def test_remeshed_vertices_lie_on_the_input():
    from arah_release_amd import meshing
    res, _ = remeshed()
    verts, faces = mesh("sphere33")
    d2, face, closest = meshing.soup_closest(verts[faces], res["verts"])
    ulp = float(np.spacing(np.float32(verts.abs().max())))
    print("projection: max d2 %.3g, bound %.3g" % (float(d2.max()), 3.0 * ulp * ulp))
    assert float(d2.max()) <= 3.0 * ulp * ulp                                     # the closest point, rounded once to float32
    assert torch.equal(face.long(), res["src_face"])
    w = res["src_bary"]
    assert bool((w >= 0).all()) and float((w.sum(1) - 1).abs().max()) < 1e-12
    back = (w[:, :, None] * verts.double()[faces[res["src_face"]]]).sum(1)
    assert float((back - res["verts"].double()).abs().max()) < 2.0 * ulp


def test_remeshed_attributes_are_interpolated():
    res, attrs = remeshed()
    _, faces = mesh("sphere33")
    at, w = faces[res["src_face"]], res["src_bary"]
    A = attrs["w"][at]
    want = (w[:, 0, None] * A[:, 0] + w[:, 1, None] * A[:, 1]) + w[:, 2, None] * A[:, 2]
    assert res["w"].dtype == torch.float64 and torch.equal(res["w"], want)
    assert torch.equal(res["label"], attrs["label"][at[torch.arange(at.shape[0]), w.argmax(1)]])


def test_remeshed_sphere_is_more_regular_than_the_input():
    res, _ = remeshed()
    before, after = res["report"]["before"], res["report"]["after"]
    print("edges in [4/5 L, 4/3 L]: %.4f -> %.4f; faces with an angle below 30 degrees: %.4f -> %.4f; valence 6: %.4f -> %.4f"
          % (before["edges_in_range"], after["edges_in_range"], before["small_angle_share"], after["small_angle_share"],
             before["valence6_share"], after["valence6_share"]))
    assert after["edges_in_range"] > before["edges_in_range"]
    assert after["small_angle_share"] < before["small_angle_share"]
    assert before["edge_length"] == after["edge_length"] == res["report"]["edge_length"] == before["edge_mean"]


def test_remesh_options_and_argument_checks():
    from arah_release_amd import geometry
    verts, faces = mesh("sphere17")
    L = geometry.mesh_quality(verts, faces)["edge_mean"]
    coarse = geometry.isotropic_remesh(verts, faces, edge_length=2.0 * L, iterations=2, project=False, max_rounds=8)
    assert coarse["n_tris"] < faces.shape[0] // 2 and geometry.mesh_topology(coarse["verts"], coarse["faces"])["watertight"]
    same = geometry.isotropic_remesh(verts, faces, iterations=0)
    assert torch.equal(same["verts"], verts) and torch.equal(same["faces"], faces) and same["report"]["iterations"] == []
    out = geometry.apply_isotropic(verts, faces, geometry.check_isotropic({"edge_length": 2.0 * L, "iterations": 2, "project": False,
                                                                           "max_rounds": 8}))
    assert torch.equal(out["verts"], coarse["verts"]) and torch.equal(out["faces"], coarse["faces"])
    assert set(out["isotropic"]) == {"src_face", "src_bary", "report"} and out["n_tris"] == coarse["n_tris"]
    assert geometry.check_isotropic(None) is None and geometry.check_isotropic(0.25) == {"edge_length": 0.25}
    for bad in ({"edge_length": 0.0}, {"edge_length": float("inf")}, {"iterations": -1}, {"iterations": 1.5}, {"lamb": 0.0},
                {"project": 1}, {"max_rounds": 0}, {"max_faces": -1}, {"levels": 2}, "fine", True):
        with pytest.raises(ValueError):
            geometry.check_isotropic(bad)
    with pytest.raises(ValueError):
        geometry.isotropic_remesh(verts, faces, edge_length=0.1 * L, max_faces=faces.shape[0])
    with pytest.raises(ValueError):
        geometry.isotropic_remesh(verts, faces, attributes={"report": verts})


def test_abi_is_declared_and_checks_its_arguments():
    import ctypes as C
    from arah_release_amd import hip
    with open(os.path.join(REPO, "include", "arah_hip.h")) as fh:
        declared = set(re.findall(r"\b(arah_\w+)\s*\(", fh.read()))
    lib = hip.load_library()
    for name in NEW_EXPORTS:
        assert name in declared and name in hip.EXPORTS and hasattr(lib, name), name
    p = C.c_void_p(256)                                                           # never dereferenced: every call is refused

    def collapse(V=4, F=4, short=1.0, long=1.0, counts=p, nbytes=1 << 30):
        return lib.arah_mesh_collapse_round_bounded(p, C.c_int64(V), p, C.c_int64(F), C.c_int32(1), C.c_double(1e-3), C.c_float(1.0),
                                                    C.c_double(short), C.c_double(long), p, p, p, p, counts, p, p, p, p,
                                                    C.c_size_t(nbytes), None)
    for bad in ({"V": -1}, {"short": -1.0}, {"short": float("nan")}, {"long": -1.0}, {"long": float("nan")}, {"counts": None}):
        assert collapse(**bad) == -1, bad
    assert collapse(nbytes=16) == -3

    def tangential(V=4, factor=0.5, verts=p, start=p, normal=p):
        return lib.arah_mesh_tangential(verts, C.c_int64(V), start, p, p, normal, C.c_float(factor), p, None)
    for bad in ({"V": -1}, {"V": 2 ** 31}, {"factor": float("nan")}, {"factor": float("inf")}, {"verts": None}, {"start": None},
                {"normal": None}):
        assert tangential(**bad) == -1, bad
