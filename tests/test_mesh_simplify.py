"""Simplification of indexed meshes by vertex clustering: arah_mesh_simplify (csrc/meshsimp.hpp), its tensor specification
meshing.mesh_simplify, geometry.simplify_mesh and the `simplify` option of MetaAvatarRender.posed_mesh / canonical_mesh.

Every decision of the clustering is an integer's, so every result is unique.  CPU tests hold the specification to a numpy
restatement written with python loops and dicts, and to the properties a simplified closed surface must have; GPU tests hold the
kernels to the specification with torch.equal on every output, guard rows included."""
import math

import numpy as np
import pytest
import torch

from conftest import get_model

gpu = pytest.mark.gpu
DEV = "cuda:0"


# ---- fields on the lattice of [-1,1]^3 (those of tests/test_mesh_components.py, restated) --------------------------------------
def _lattice(n):
    ax = torch.linspace(-1, 1, n)
    return torch.meshgrid(ax, ax, ax, indexing="ij")


def sphere(n, radius=0.7123):
    X, Y, Z = _lattice(n)
    return torch.sqrt(X ** 2 + Y ** 2 + Z ** 2) - radius


def torus(n):
    X, Y, Z = _lattice(n)
    return torch.sqrt((torch.sqrt(X ** 2 + Y ** 2) - 0.55) ** 2 + Z ** 2) - 0.2371


def two_blobs(n):
    X, Y, Z = _lattice(n)
    a = torch.sqrt((X - 0.4) ** 2 + Y ** 2 + Z ** 2) - 0.31
    b = torch.sqrt((X + 0.4) ** 2 + Y ** 2 + Z ** 2) - 0.27
    return torch.minimum(a, b)


def noise(n=20, seed=11):
    v = torch.randn(n, n, n, generator=torch.Generator().manual_seed(seed))
    v[0], v[-1], v[:, 0], v[:, -1], v[:, :, 0], v[:, :, -1] = 1, 1, 1, 1, 1, 1
    return v


def quantised(n):
    """Many lattice values exactly at the level: crossing points at t = 0, degenerate triangles, coincident distinct vertices."""
    X, Y, Z = _lattice(n)
    return torch.round(4.0 * (torch.sqrt(X ** 2 + Y ** 2 + Z ** 2) - 0.55)) / 4.0


def body_with_floaters(n=33):
    """A sphere and three tiny blobs of different sizes beside it: a body with floaters."""
    X, Y, Z = _lattice(n)
    d = torch.sqrt(X ** 2 + Y ** 2 + Z ** 2) - 0.45
    for (cx, cy, cz), r in (((0.75, 0.7, 0.7), 0.10), ((-0.7, 0.72, -0.7), 0.14), ((-0.72, -0.7, 0.74), 0.18)):
        d = torch.minimum(d, torch.sqrt((X - cx) ** 2 + (Y - cy) ** 2 + (Z - cz) ** 2) - r)
    return d


FIELDS = {"sphere17": (lambda: sphere(17), 17), "torus33": (lambda: torus(33), 33), "blobs33": (lambda: two_blobs(33), 33),
          "noise20": (noise, 20), "quantised17": (lambda: quantised(17), 17), "floaters33": (body_with_floaters, 33)}
MULTS = (1.0, 2.0, 3.7)                                                          # cells, in lattice steps 2 / (n - 1)
COMBOS = [(name, mult) for name in FIELDS for mult in MULTS]
SMOOTH = ("sphere17", "torus33", "blobs33")
_MESH, _SPEC, _RESTATED = {}, {}, {}


def mesh(name):
    """(verts (V,3), faces (F,3) int64) of a named field on the host, computed once and shared; never modified."""
    from arah_release_amd import meshing
    if name not in _MESH:
        verts, faces, _ = meshing.marching_cubes_indexed(FIELDS[name][0]())
        _MESH[name] = (verts, faces)
    return _MESH[name]


def grid_of(verts, cell):
    """The grid rule, in float32: origin = floor(lo / cell) cell, dims = floor((hi - origin) / cell) + 1 over the vertices' box."""
    v = verts.numpy()[np.isfinite(verts.numpy()).all(1)]
    lo, hi, c = v.min(0).astype(np.float32), v.max(0).astype(np.float32), np.float32(cell)
    origin = (np.floor(lo / c) * c).astype(np.float32)
    dims = [int(x) + 1 for x in np.floor((hi - origin) / c)]
    return [float(x) for x in origin], float(c), dims


def grid(name, mult):
    return grid_of(mesh(name)[0], mult * 2.0 / (FIELDS[name][1] - 1))


def spec(name, mult, position="mean", dedup=True):
    """meshing.mesh_simplify of a named mesh on the host, computed once and shared; never modified."""
    from arah_release_amd import meshing
    key = (name, mult, position, dedup)
    if key not in _SPEC:
        verts, faces = mesh(name)
        _SPEC[key] = meshing.mesh_simplify(verts, faces, *grid(name, mult), position=position, dedup=dedup)
    return _SPEC[key]


# ---- an independent restatement ---------------------------------------------------------------------------------------------------
def numpy_simplify(verts, faces, origin, cell, dims, dedup=True):
    """The semantics of the clustering once more: python loops and dicts for every decision, np.add.at for the sums, first-seen
    dedup.  -> dict of the untrimmed outputs (both positions) as numpy arrays."""
    with np.errstate(over="ignore"):                                             # a far vertex: inf is what float32 gives, and clamps
        return _numpy_simplify(np.asarray(verts, np.float32), np.asarray(faces, np.int64).reshape(-1, 3), origin, cell, dims, dedup)


def _numpy_simplify(v, f, origin, cell, dims, dedup):
    V, F = v.shape[0], f.shape[0]
    o, inv = np.asarray(origin, np.float32), np.float32(1.0) / np.float32(cell)
    extent = max(dims) * float(np.float32(cell))
    e = 0
    while 2.0 ** e < extent:
        e += 1
    while 2.0 ** (e - 1) >= extent:
        e -= 1
    scale = 2.0 ** (36 - e)
    cells = np.floor((v - o) * inv)                                              # float32: one subtraction, one multiplication
    keys = []
    for i in range(V):
        if not all(math.isfinite(x) for x in v[i].tolist()):
            keys.append(None)
            continue
        c = [min(int(min(max(t, 0.0), 2.0 ** 27)), n - 1) for t, n in zip(cells[i].tolist(), dims)]
        keys.append(c[0] + dims[0] * (c[1] + dims[1] * c[2]))
    cluster = {k: j for j, k in enumerate(sorted(set(k for k in keys if k is not None)))}
    K = len(cluster)
    vert_map = np.array([-1 if k is None else cluster[k] for k in keys], np.int64).reshape(-1)
    members = np.nonzero(vert_map >= 0)[0]
    q = np.rint(np.clip((v[members].astype(np.float64) - o.astype(np.float64)) * scale, -2.0 ** 36, 2.0 ** 36)).astype(np.int64)
    S, n = np.zeros((K, 3), np.int64), np.zeros(K, np.int64)
    np.add.at(S, vert_map[members], q)
    np.add.at(n, vert_map[members], 1)
    mean = (o.astype(np.float64) + (S.astype(np.float64) / n[:, None].astype(np.float64)) / scale).astype(np.float32)
    d = v[members].astype(np.float64) - mean[vert_map[members]].astype(np.float64)
    d2 = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(np.float32)
    best = {}
    for i, dist in zip(members.tolist(), d2.tolist()):                          # ascending ids: a tie keeps the lower one
        k = int(vert_map[i])
        if k not in best or dist < best[k][0]:
            best[k] = (dist, i)
    vert_src = np.zeros(V, np.int64)
    vert_src[:K] = [best[k][1] for k in range(K)]
    out_mean, out_member = np.zeros((V, 3), np.float32), np.zeros((V, 3), np.float32)
    out_mean[:K], out_member[:K] = mean, v[vert_src[:K]]
    kept, rows, seen = [], [], set()
    n_invalid = n_collapsed = n_dup = 0
    status = int(dedup and K > 2 ** 21)
    for r, ids in enumerate(f.tolist()):
        if not all(0 <= i < V and vert_map[i] >= 0 for i in ids):
            n_invalid += 1
            continue
        c = [int(vert_map[i]) for i in ids]
        if len(set(c)) < 3:
            n_collapsed += 1
            continue
        if status:
            continue
        if dedup:
            if frozenset(c) in seen:
                n_dup += 1
                continue
            seen.add(frozenset(c))
        kept.append(c)
        rows.append(r)
    faces_out, face_src = np.zeros((F, 3), np.int64), np.zeros(F, np.int64)
    faces_out[:len(kept)] = np.array(kept, np.int64).reshape(-1, 3)
    face_src[:len(rows)] = rows
    return {"mean": out_mean, "member": out_member, "vert_src": vert_src, "vert_map": vert_map, "faces_out": faces_out,
            "face_src": face_src, "counts": np.array([K, len(kept), n_invalid, n_collapsed, n_dup, status], np.int64),
            "d2": d2, "members": members}


def restated(name, mult):
    if (name, mult) not in _RESTATED:
        verts, faces = mesh(name)
        _RESTATED[(name, mult)] = numpy_simplify(verts, faces, *grid(name, mult))
    return _RESTATED[(name, mult)]


def check_against_restatement(out, ref, position):
    verts_out, vert_src, vert_map, faces_out, face_src, counts = out
    assert verts_out.dtype == torch.float32 and all(t.dtype == torch.int32 for t in out[1:])
    assert torch.equal(verts_out.view(torch.int32), torch.from_numpy(ref[position]).view(torch.int32))     # bit for bit
    for got, k in ((vert_src, "vert_src"), (vert_map, "vert_map"), (faces_out, "faces_out"), (face_src, "face_src"), (counts, "counts")):
        assert torch.equal(got.long(), torch.from_numpy(ref[k])), k


# ---- CPU: the specification ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mult", COMBOS)
def test_spec_is_the_numpy_restatement(name, mult):
    ref = restated(name, mult)
    for position in ("mean", "member"):
        check_against_restatement(spec(name, mult, position), ref, position)
    K, kept = ref["counts"][:2]
    verts, faces = mesh(name)
    assert 0 < K <= verts.shape[0] and 0 < kept <= faces.shape[0]
    if mult > 1.0:
        assert K < verts.shape[0] // 2 and kept < faces.shape[0] // 2          # it does simplify


@pytest.mark.parametrize("name", ["noise20", "floaters33"])
def test_spec_without_dedup_and_with_garbage(name):
    from arah_release_amd import meshing
    verts, faces = mesh(name)
    g = grid(name, 2.0)
    ref = numpy_simplify(verts, faces, *g, dedup=False)
    assert ref["counts"][4] == 0 and ref["counts"][1] >= restated(name, 2.0)["counts"][1]
    check_against_restatement(spec(name, 2.0, "mean", False), ref, "mean")
    bad_v, bad_f = garbage(verts, faces)
    for dedup in (True, False):
        ref = numpy_simplify(bad_v, bad_f, *g, dedup=dedup)
        assert ref["counts"][2] == 7 and (ref["vert_map"][-3:] == -1).all()
        for position in ("mean", "member"):
            check_against_restatement(meshing.mesh_simplify(bad_v, bad_f, *g, position=position, dedup=dedup), ref, position)


def garbage(verts, faces):
    """The mesh with three non-finite vertices and a far one appended, and seven faces that must go: ids out of range, and names
    of the non-finite vertices.  The far vertex (outside the grid: clamped into a border cell) is a valid one."""
    V = verts.shape[0]
    more = torch.tensor([[float("nan"), 0.0, 0.0], [0.0, float("inf"), 0.0], [0.1, 0.2, -float("inf")]])
    bad_v = torch.cat([verts, torch.tensor([[3.0e38, -3.0e38, 17.0]]), more])
    rows = [[-1, 0, 1], [0, V + 4, 1], [0, 1, 2 ** 31 - 1], [2 ** 40, 1, 2], [V + 1, 0, 1], [0, V + 2, 1], [0, 1, V + 3], [0, V, 5]]
    bad_f = torch.cat([faces[:100], torch.tensor(rows, dtype=torch.int64), faces[100:]])
    return bad_v, bad_f


@pytest.mark.parametrize("name,mult", COMBOS)
def test_spec_does_not_depend_on_the_order_of_the_vertices(name, mult):
    from arah_release_amd import meshing
    verts, faces = mesh(name)
    V = verts.shape[0]
    perm = torch.randperm(V, generator=torch.Generator().manual_seed(3))         # new vertex i is old vertex perm[i]
    new_id = torch.empty(V, dtype=torch.int64)
    new_id[perm] = torch.arange(V)
    ref = restated(name, mult)
    K = int(ref["counts"][0])
    # per cluster, the old ids that tie at the smallest squared distance
    tied = {}
    for i, dist in zip(ref["members"].tolist(), ref["d2"].tolist()):
        k = int(ref["vert_map"][i])
        if k not in tied or dist < tied[k][0]:
            tied[k] = (dist, [i])
        elif dist == tied[k][0]:
            tied[k][1].append(i)
    n_ties = 0
    for position in ("mean", "member"):
        a = spec(name, mult, position)
        b = meshing.mesh_simplify(verts[perm], new_id[faces], *grid(name, mult), position=position)
        assert torch.equal(a[5], b[5])
        assert torch.equal(a[2].long(), b[2].long()[new_id])                     # the cluster of every vertex
        assert torch.equal(a[3], b[3]) and torch.equal(a[4], b[4])               # the faces, row for row
        src_a, src_b = a[1][:K].long(), b[1][:K].long()
        assert not b[1][K:].any()
        # the lowest NEW id among the tied members wins ...
        assert src_b.tolist() == [min(int(new_id[i]) for i in tied[k][1]) for k in range(K)]
        # ... so a cluster without a tie keeps its vertex.  Ties are of two kinds: the coincident vertices of quantised17 (the same
        # position either way), and members at one distance from the mean to the bit -- the two members of a cluster whose mean is
        # their midpoint in float32, the mirror pairs of the symmetric fields (x <-> y swaps a cell on the diagonal into itself).
        # Those are other vertices, at other positions
        untied = torch.tensor([len(tied[k][1]) == 1 for k in range(K)])
        assert torch.equal(perm[src_b][untied], src_a[untied]) and bool(untied.any())
        moved = perm[src_b] != src_a
        coincident = moved & (verts[perm[src_b]] == verts[src_a]).all(1)
        n_ties += int(coincident.sum())
        if position == "mean":
            assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
        else:
            assert torch.equal(b[0][:K], verts[perm[src_b]]) and torch.equal(a[0][:K][~moved | coincident], b[0][:K][~moved | coincident])
    if name == "quantised17":
        assert n_ties > 0                                                        # the coincident kind is exercised


@pytest.mark.parametrize("name,mult", COMBOS)
def test_spec_invariants(name, mult):
    verts, faces = mesh(name)
    origin, cell, dims = grid(name, mult)
    o = np.array(origin, np.float64)
    v64 = verts.numpy().astype(np.float64)
    for position in ("mean", "member"):
        verts_out, vert_src, vert_map, faces_out, face_src, counts = spec(name, mult, position)
        K, kept, n_invalid, n_collapsed, n_dup, status = counts.tolist()
        assert status == 0 and kept + n_collapsed + n_dup + n_invalid == faces.shape[0] and n_invalid == 0
        vm = vert_map.numpy().astype(np.int64)
        assert vm.min() == 0 and vm.max() == K - 1 and np.unique(vm).shape[0] == K
        # every output vertex lies in the closed box of its cell
        keys = np.zeros(K, np.int64)
        c = np.clip(np.floor((verts.numpy() - np.array(origin, np.float32)) * (np.float32(1) / np.float32(cell))), 0, np.array(dims) - 1)
        keys[vm] = (c[:, 0] + dims[0] * (c[:, 1] + dims[1] * c[:, 2])).astype(np.int64)
        assert bool((np.diff(keys) > 0).all())                                  # clusters in ascending key
        cxyz = np.stack([keys % dims[0], (keys // dims[0]) % dims[1], keys // (dims[0] * dims[1])], 1).astype(np.float64)
        p = verts_out[:K].numpy().astype(np.float64)
        assert bool((p >= o + cxyz * cell).all()) and bool((p <= o + (cxyz + 1) * cell).all())
        # every vertex is within a cell's diagonal of the vertex that replaces it
        assert float(np.linalg.norm(v64 - p[vm], axis=1).max()) <= math.sqrt(3.0) * cell
        src = vert_src[:K].long()
        assert torch.equal(vert_map[src].long(), torch.arange(K))                # a representative is a member
        if position == "member":
            assert torch.equal(verts_out[:K], verts[src])
        fo = faces_out[:kept].long()
        assert bool((fo >= 0).all()) and bool((fo < K).all())
        assert bool(((fo[:, 0] != fo[:, 1]) & (fo[:, 1] != fo[:, 2]) & (fo[:, 0] != fo[:, 2])).all())    # no kept face repeats a cluster
        assert len({frozenset(r) for r in fo.tolist()}) == kept                  # no two kept faces share a cluster set
        assert bool((face_src[:kept].long().diff() > 0).all())                   # original order
        assert torch.equal(fo, vert_map.long()[faces[face_src[:kept].long()]])   # original orientation
        assert not verts_out[K:].any() and not vert_src[K:].any() and not faces_out[kept:].any() and not face_src[kept:].any()


def unreferenced(out):
    K, kept = out[5].tolist()[:2]
    return K - int(torch.unique(out[3][:kept]).shape[0])


@pytest.mark.parametrize("mult", MULTS)
def test_spec_noise_exercises_duplicates_and_unreferenced_clusters(mult):
    out = spec("noise20", mult)
    print("noise20 at %.1f steps: counts %s, unreferenced clusters %d" % (mult, out[5].tolist(), unreferenced(out)))
    assert out[5][4].item() > 100
    assert unreferenced(out) >= 1
    for name in SMOOTH:
        assert unreferenced(spec(name, mult)) == 0


CLOSED = [(n, m, 2) for n in ("sphere17", "quantised17") for m in MULTS] + [("blobs33", m, 4) for m in MULTS] + \
         [("torus33", 1.0, 0), ("torus33", 2.0, 0)]


@pytest.mark.parametrize("name,mult,euler", CLOSED)
def test_spec_keeps_closed_surfaces_closed(name, mult, euler):
    out = spec(name, mult)
    K, kept = out[5].tolist()[:2]
    directed = {}
    for a, b, c in out[3][:kept].tolist():
        for e in ((a, b), (b, c), (c, a)):
            directed[e] = directed.get(e, 0) + 1
    assert all(n == 1 and directed.get((b, a)) == 1 for (a, b), n in directed.items())   # every edge: two faces, opposite ways
    n_verts = len({i for e in directed for i in e})
    assert n_verts - len(directed) // 2 + kept == euler


def test_spec_arguments_and_empty_meshes():
    from arah_release_amd import meshing
    verts, faces = mesh("sphere17")
    g = grid("sphere17", 2.0)
    V, F = verts.shape[0], faces.shape[0]
    for bad in (lambda: meshing.mesh_simplify(verts.double(), faces, *g), lambda: meshing.mesh_simplify(verts.reshape(-1), faces, *g),
                lambda: meshing.mesh_simplify(verts[:, :2], faces, *g), lambda: meshing.mesh_simplify(verts, faces.float(), *g),
                lambda: meshing.mesh_simplify(verts, faces.reshape(-1), *g), lambda: meshing.mesh_simplify(verts, faces, *g, position="median"),
                lambda: meshing.mesh_simplify(verts, faces, g[0], 0.0, g[2]), lambda: meshing.mesh_simplify(verts, faces, g[0], float("nan"), g[2]),
                lambda: meshing.mesh_simplify(verts, faces, g[0], -1.0, g[2]), lambda: meshing.mesh_simplify(verts, faces, g[0][:2], g[1], g[2]),
                lambda: meshing.mesh_simplify(verts, faces, [0.0, float("inf"), 0.0], g[1], g[2]),
                lambda: meshing.mesh_simplify(verts, faces, g[0], g[1], [4, 0, 4]), lambda: meshing.mesh_simplify(verts, faces, g[0], g[1], [4, 4]),
                lambda: meshing.mesh_simplify(verts, faces, g[0], g[1], [4.5, 4, 4]),
                lambda: meshing.mesh_simplify(verts, faces, g[0], g[1], [512, 512, 513])):             # over 2^27 cells
        with pytest.raises(ValueError):
            bad()
    assert meshing.mesh_simplify(verts, faces, g[0], g[1], [512, 512, 512])[5][5].item() == 0          # 2^27 cells exactly
    no_f = torch.zeros(0, 3, dtype=torch.int64)
    out = meshing.mesh_simplify(torch.zeros(0, 3), faces, *g)                    # V = 0: every face names a vertex that is not there
    assert out[5].tolist() == [0, 0, F, 0, 0, 0] and out[0].shape == (0, 3) and out[3].shape == (F, 3) and not out[3].any()
    out = meshing.mesh_simplify(verts, no_f, *g)                                 # F = 0: the clusters alone
    assert out[5].tolist() == [int(spec("sphere17", 2.0)[5][0]), 0, 0, 0, 0, 0] and out[3].shape == (0, 3)
    assert torch.equal(out[0], spec("sphere17", 2.0)[0])
    assert meshing.mesh_simplify(torch.zeros(0, 3), no_f, *g)[5].tolist() == [0] * 6
    nan = torch.full((5, 3), float("nan"))
    out = meshing.mesh_simplify(nan, torch.tensor([[0, 1, 2]]), *g)              # no valid vertex at all
    assert out[5].tolist() == [0, 0, 1, 0, 0, 0] and out[2].tolist() == [-1] * 5
    # int32 faces and tensors for the grid are taken as they are
    out = meshing.mesh_simplify(verts, faces.to(torch.int32), torch.tensor(g[0]), g[1], torch.tensor(g[2]))
    for a, b in zip(out, spec("sphere17", 2.0)):
        assert torch.equal(a, b)


def test_spec_fix_scale_is_a_power_of_two_that_fits():
    from arah_release_amd import meshing
    for cell, dims in ((0.125, [16, 3, 1]), (0.125, [17, 3, 1]), (1.0, [1, 1, 1]), (3.0, [5, 4, 1000]), (1e-3, [7, 7, 7]), (2.0 ** -20, [2 ** 27, 1, 1])):
        o, c, inv, d, scale = meshing.simplify_grid([0.0, 0.0, 0.0], cell, dims)
        extent = max(dims) * c
        assert math.frexp(scale)[0] == 0.5 and 2.0 ** 35 < extent * scale <= 2.0 ** 36
        assert inv == float(np.float32(1.0) / np.float32(cell))


def test_spec_status_when_dedup_meets_too_many_clusters():
    """Three sorted 21-bit ids make a face's key: one cluster more than 2^21, and dedup cannot name its faces."""
    from arah_release_amd import geometry, meshing
    V = 2 ** 21 + 1
    verts = torch.zeros(V, 3)
    verts[:, 0] = torch.arange(V, dtype=torch.float32) + 0.5                     # exact in float32: one vertex per cell
    faces = torch.tensor([[0, 1, 2], [2, 1, 0], [V - 1, 5, 7], [3, 3, 4], [0, 1, V]])
    g = ([0.0, 0.0, 0.0], 1.0, [V, 1, 1])
    out = meshing.mesh_simplify(verts, faces, *g)
    assert out[5].tolist() == [V, 0, 1, 1, 0, 1] and not out[3].any() and not out[4].any()
    assert torch.equal(out[2], torch.arange(V, dtype=torch.int32)) and torch.equal(out[0][:, 0], verts[:, 0])
    out = meshing.mesh_simplify(verts, faces, *g, dedup=False)
    assert out[5].tolist() == [V, 3, 1, 1, 0, 0] and out[3][:3].tolist() == [[0, 1, 2], [2, 1, 0], [V - 1, 5, 7]]
    out = meshing.mesh_simplify(verts[:-1], faces[:2], [0.0, 0.0, 0.0], 1.0, [V - 1, 1, 1])      # 2^21 clusters still fit
    assert out[5].tolist() == [V - 1, 1, 0, 0, 1, 0]
    with pytest.raises(ValueError):
        geometry.simplify_mesh(verts, faces, cell=1.0, bounds=([0.0] * 3, [float(V - 1), 0.0, 0.0]))
    res = geometry.simplify_mesh(verts, faces, cell=1.0, bounds=([0.0] * 3, [float(V - 1), 0.0, 0.0]), dedup=False)
    assert (res["n_verts"], res["n_tris"]) == (6, 3) and res["removed"]["vertices"] == V - 6


# ---- CPU: geometry.simplify_mesh ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mult", [("floaters33", 2.0), ("noise20", 1.0), ("noise20", 3.7)])
def test_simplify_mesh_is_the_specification_without_unreferenced_clusters(name, mult):
    from arah_release_amd import geometry
    verts, faces = mesh(name)
    origin, cell, dims = grid(name, mult)
    ids = torch.arange(verts.shape[0] * 2, dtype=torch.float32).reshape(-1, 2)
    for position in ("mean", "member"):
        verts_out, vert_src, vert_map, faces_out, face_src, counts = spec(name, mult, position)
        K, kept, n_invalid, n_collapsed, n_dup, _ = counts.tolist()
        whole = geometry.simplify_mesh(verts, faces, cell=cell, position=position, drop_unreferenced=False, attributes={"ids": ids})
        assert whole["dims"] == tuple(dims) and whole["cell"] == cell and (whole["n_verts"], whole["n_tris"]) == (K, kept)
        assert torch.equal(whole["verts"], verts_out[:K]) and torch.equal(whole["faces"], faces_out[:kept].long())
        assert whole["faces"].dtype == faces.dtype and whole["vert_src"].dtype == torch.int64
        assert torch.equal(whole["vert_src"], vert_src[:K].long()) and torch.equal(whole["ids"], ids[vert_src[:K].long()])
        assert whole["removed"] == {"vertices": verts.shape[0] - K, "faces_collapsed": n_collapsed, "faces_duplicate": n_dup,
                                    "faces_invalid": n_invalid}
        res = geometry.simplify_mesh(verts, faces.to(torch.int32), cell=cell, position=position, attributes={"ids": ids})
        used = torch.unique(faces_out[:kept].long())                             # ascending: the order is preserved
        assert res["n_verts"] == used.shape[0] == K - unreferenced(spec(name, mult, position)) and res["n_tris"] == kept
        assert torch.equal(res["verts"], verts_out[used]) and torch.equal(res["vert_src"], vert_src.long()[used])
        assert torch.equal(res["verts"][res["faces"].long()], verts_out[faces_out[:kept].long()]) and res["faces"].dtype == torch.int32
        assert torch.equal(res["ids"], ids[res["vert_src"]]) and res["removed"]["vertices"] == verts.shape[0] - used.shape[0]
        if name == "noise20":
            assert res["n_verts"] < K
    # resolution: cells along the longest side of the bounds; bounds of one's own
    lo, hi = verts.min(0).values, verts.max(0).values
    res = geometry.simplify_mesh(verts, faces, resolution=8)
    side = float(np.float32((hi - lo).max().item()) / np.float32(8))
    assert res["cell"] == side and res["dims"] == tuple(grid_of(verts, side)[2]) and 8 <= max(res["dims"]) <= 9
    same = geometry.simplify_mesh(verts, faces, resolution=8, bounds=(lo, hi.tolist()))
    assert same["dims"] == res["dims"] and torch.equal(same["verts"], res["verts"]) and torch.equal(same["faces"], res["faces"])
    wide = geometry.simplify_mesh(verts, faces, cell=0.5, bounds=([-2.0, -2.0, -2.0], [2.0, 2.0, 2.0]))
    assert wide["dims"] == (9, 9, 9) and 0 < wide["n_verts"] <= 64


def test_simplify_mesh_arguments():
    from arah_release_amd import geometry
    verts, faces = mesh("sphere17")
    ok = geometry.simplify_mesh(verts, faces, cell=0.25)
    assert set(ok) == {"verts", "faces", "n_verts", "n_tris", "vert_src", "removed", "cell", "dims"}
    assert set(ok["removed"]) == {"vertices", "faces_collapsed", "faces_duplicate", "faces_invalid"}
    for bad in (lambda: geometry.simplify_mesh(verts, faces), lambda: geometry.simplify_mesh(verts, faces, cell=0.25, resolution=8),
                lambda: geometry.simplify_mesh(verts, faces, cell=0.0), lambda: geometry.simplify_mesh(verts, faces, cell=float("inf")),
                lambda: geometry.simplify_mesh(verts, faces, cell="big"), lambda: geometry.simplify_mesh(verts, faces, resolution=0),
                lambda: geometry.simplify_mesh(verts, faces, resolution=2.5), lambda: geometry.simplify_mesh(verts, faces, resolution=True),
                lambda: geometry.simplify_mesh(verts, faces, cell=0.25, position="centre"),
                lambda: geometry.simplify_mesh(verts.reshape(-1), faces, cell=0.25), lambda: geometry.simplify_mesh(verts.long(), faces, cell=0.25),
                lambda: geometry.simplify_mesh(verts, faces.float(), cell=0.25), lambda: geometry.simplify_mesh(verts, faces.reshape(-1), cell=0.25),
                lambda: geometry.simplify_mesh(verts, faces.tolist(), cell=0.25),
                lambda: geometry.simplify_mesh(verts, faces, cell=0.25, bounds=([0, 0, 0], [1, 1])),
                lambda: geometry.simplify_mesh(verts, faces, cell=0.25, bounds=([0, 0, 0], [1, -1, 1])),
                lambda: geometry.simplify_mesh(verts, faces, cell=0.25, bounds=([0, 0, 0], [1, float("nan"), 1])),
                lambda: geometry.simplify_mesh(verts, faces, cell=1e-3),                                # over 2^27 cells
                lambda: geometry.simplify_mesh(verts, faces, cell=1e-40),                               # a denormal float32: no finite grid
                lambda: geometry.simplify_mesh(verts, faces, cell=1e-40, bounds=([-1.0] * 3, [1.0] * 3)),
                lambda: geometry.simplify_mesh(verts, faces, cell=0.25, attributes={"verts": verts}),
                lambda: geometry.simplify_mesh(verts, faces, cell=0.25, attributes={"w": verts[:-1]}),
                lambda: geometry.check_simplify("fine"), lambda: geometry.check_simplify({"cell": 0.1, "size": 3}),
                lambda: geometry.check_simplify(True), lambda: geometry.check_simplify(-0.1), lambda: geometry.check_simplify({})):
        with pytest.raises(ValueError):
            bad()
    assert geometry.check_simplify(0.05) == {"cell": 0.05} and geometry.check_simplify({"resolution": 64, "dedup": False})["resolution"] == 64
    # empty meshes, vertices that are not numbers, faces that name no vertex
    res = geometry.simplify_mesh(torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int64), cell=0.25)
    assert (res["n_verts"], res["n_tris"], res["dims"]) == (0, 0, (1, 1, 1)) and res["verts"].shape == (0, 3) and res["faces"].shape == (0, 3)
    res = geometry.simplify_mesh(verts, torch.zeros(0, 3, dtype=torch.int64), cell=0.25)
    assert (res["n_verts"], res["n_tris"]) == (0, 0) and res["removed"]["vertices"] == verts.shape[0]
    res = geometry.simplify_mesh(verts, torch.zeros(0, 3, dtype=torch.int64), cell=0.25, drop_unreferenced=False)
    assert res["n_verts"] == ok["n_verts"] and torch.equal(res["verts"], ok["verts"])          # the sphere has no unreferenced cluster
    bad_v, bad_f = garbage(verts, faces)
    res = geometry.simplify_mesh(bad_v[:-4].clone(), bad_f, cell=0.25)                        # the bounds: the finite vertices' box
    assert res["dims"] == ok["dims"] and res["removed"]["faces_invalid"] == 8 and torch.equal(res["verts"], ok["verts"])
    res = geometry.simplify_mesh(torch.cat([verts, bad_v[-3:]]), bad_f, cell=0.25)
    assert res["dims"] == ok["dims"] and res["removed"]["faces_invalid"] == 8 and torch.equal(res["verts"], ok["verts"])
    res = geometry.simplify_mesh(torch.full((4, 3), float("nan")), torch.tensor([[0, 1, 2]]), resolution=4)
    assert (res["n_verts"], res["n_tris"], res["removed"]["faces_invalid"]) == (0, 0, 1)


def test_model_entries_refuse_simplify_on_a_soup():
    model, _ = get_model("zju377_mono")
    model.eval()
    with pytest.raises(ValueError, match="indexed=True"):                        # refused before the frame is looked at
        model.posed_mesh({}, simplify=0.05)
    with pytest.raises(ValueError, match="simplify"):
        model.posed_mesh({}, indexed=True, simplify={"cell": 0.05, "resolution": 8})
    with pytest.raises(ValueError, match="simplify"):
        model.canonical_mesh({}, simplify="coarse")


# ---- GPU: the kernels against the specification ---------------------------------------------------------------------------------
def _kernel_is_the_spec(verts, faces, g, position, dedup, ref=None):
    from arah_release_amd import hip, meshing
    ref = meshing.mesh_simplify(verts, faces, *g, position=position, dedup=dedup) if ref is None else ref
    got = hip.mesh_simplify(verts.to(DEV), faces.to(DEV), *g, position=position, dedup=dedup)
    assert got[0].dtype == torch.float32 and all(t.dtype == torch.int32 for t in got[1:])
    assert torch.equal(got[0].cpu().view(torch.int32), ref[0].view(torch.int32)), "verts_out"
    for name, r, t in zip(("vert_src", "vert_map", "faces_out", "face_src", "counts"), ref[1:], got[1:]):
        assert t.device.type == "cuda" and torch.equal(t.cpu(), r), (name, position, dedup)
    return ref


@gpu
@pytest.mark.parametrize("name,mult", COMBOS)
def test_kernels_are_the_specification_on_level_sets(name, mult):
    verts, faces = mesh(name)
    for position in ("mean", "member"):
        for dedup in (True, False):
            _kernel_is_the_spec(verts, faces, grid(name, mult), position, dedup, spec(name, mult, position, dedup))


@gpu
@pytest.mark.parametrize("dedup", [True, False])
def test_kernels_are_the_specification_on_garbage(dedup):
    verts, faces = mesh("floaters33")
    bad_v, bad_f = garbage(verts, faces)
    for position in ("mean", "member"):
        ref = _kernel_is_the_spec(bad_v, bad_f, grid("floaters33", 2.0), position, dedup)
        assert ref[5][2].item() == 7 and ref[2][-3:].tolist() == [-1, -1, -1]
    # no valid vertex at all, and no vertex at all
    g = grid("floaters33", 2.0)
    _kernel_is_the_spec(torch.full((70, 3), float("nan")), faces[:130] % 70, g, "mean", dedup)
    _kernel_is_the_spec(torch.zeros(0, 3), faces[:130], g, "member", dedup)
    _kernel_is_the_spec(verts, faces[:0], g, "mean", dedup)
    _kernel_is_the_spec(torch.zeros(0, 3), faces[:0], g, "mean", dedup)


@gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1023, 1024, 1025])
def test_kernels_are_the_specification_across_the_chunking(n):
    verts, faces = mesh("noise20")
    assert verts.shape[0] > 1025 and faces.shape[0] > 4 * 1024                   # more than one block of the count / scan / fill
    g = grid("noise20", 2.0)
    low = faces[(faces < n).all(1)]                                              # the faces among the first n vertices
    ref = _kernel_is_the_spec(verts, faces[:n], g, "mean", True)                 # F = n
    assert ref[5][2].item() == 0
    ref = _kernel_is_the_spec(verts[:n], faces, g, "member", True)               # V = n: most faces name a vertex beyond it
    assert ref[5][2].item() == faces.shape[0] - low.shape[0]
    _kernel_is_the_spec(verts[:n], faces[:n], g, "mean", False)
    if low.shape[0]:
        _kernel_is_the_spec(verts[:n], low[:n], g, "member", True)


@gpu
def test_kernels_are_deterministic_and_isolated():
    from arah_release_amd import hip
    small_v, small_f = mesh("sphere17")
    big_v, big_f = mesh("noise20")
    gs, gb = grid("sphere17", 2.0), grid("noise20", 1.0)
    sv, sf, bv, bf = small_v.to(DEV), small_f.to(DEV).to(torch.int32), big_v.to(DEV), big_f.to(DEV).to(torch.int32)
    fresh = hip.mesh_simplify(sv, sf, *gs)
    again = hip.mesh_simplify(sv, sf, *gs)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        first_on_side = hip.mesh_simplify(bv, bf, *gb)                           # sizes this stream's scratch
        other = hip.mesh_simplify(sv, sf, *gs)                                   # ... and reuses it, stale table and all
    side.synchronize()
    big = hip.mesh_simplify(bv, bf, *gb)
    after = hip.mesh_simplify(sv, sf, *gs)                                       # the smaller one on what the larger left behind
    for run in (again, other, after):
        for a, b in zip(fresh, run):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    for a, b in zip(first_on_side, big):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    for a, b in zip(fresh, spec("sphere17", 2.0)):
        assert torch.equal(a.cpu().view(torch.int32), b.view(torch.int32))


@gpu
def test_binding_validates():
    from arah_release_amd import hip
    verts, faces = mesh("sphere17")
    g = grid("sphere17", 2.0)
    v, f = verts.to(DEV), faces.to(DEV)
    for bad in (lambda: hip.mesh_simplify(verts, f, *g), lambda: hip.mesh_simplify(v, faces, *g), lambda: hip.mesh_simplify(v.double(), f, *g),
                lambda: hip.mesh_simplify(v, f.float(), *g), lambda: hip.mesh_simplify(v, f, *g, position="median"),
                lambda: hip.mesh_simplify(v, f, g[0], 0.0, g[2]), lambda: hip.mesh_simplify(v, f, g[0], g[1], [512, 512, 513]),
                lambda: hip.mesh_simplify(v, f, [0.0, float("nan"), 0.0], g[1], g[2])):
        with pytest.raises(ValueError):
            bad()
    lib = hip.load_library()
    assert lib.arah_mesh_simplify_scratch_bytes(10, 10, 10) > 0 and lib.arah_mesh_simplify_scratch_bytes(0, 0, 1) > 0
    for sizes in ((-1, 0, 1), (0, -1, 1), (0, 0, 0), (2 ** 26 + 1, 0, 1), (0, 2 ** 28 + 1, 1), (0, 0, 2 ** 27 + 1)):
        assert lib.arah_mesh_simplify_scratch_bytes(*sizes) == 0


@gpu
@pytest.mark.parametrize("how", [{"cell": 0.125}, {"resolution": 12, "position": "member"}, {"cell": 0.2, "drop_unreferenced": False},
                                 {"cell": 0.125, "dedup": False, "bounds": ([-1.0] * 3, [1.0] * 3)}], ids=str)
def test_simplify_mesh_on_the_device_is_the_host(how):
    from arah_release_amd import geometry
    verts, faces = mesh("floaters33")
    weights = torch.arange(verts.shape[0] * 2, dtype=torch.float32).reshape(-1, 2)
    ref = geometry.simplify_mesh(verts, faces, attributes={"weights": weights}, **how)
    got = geometry.simplify_mesh(verts.to(DEV), faces.to(DEV).to(torch.int32), attributes={"weights": weights.to(DEV)}, **how)
    assert 0 < ref["n_verts"] < verts.shape[0] // 2 and 0 < ref["n_tris"] < faces.shape[0] // 2
    assert set(got) == set(ref) and got["faces"].dtype == torch.int32 and got["verts"].is_cuda
    for k in ref:
        if torch.is_tensor(ref[k]):
            assert torch.equal(got[k].cpu().long() if k == "faces" else got[k].cpu(), ref[k]), k
        else:
            assert got[k] == ref[k], k


# ---- GPU: the model's entries ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def subject(scene):
    dev = torch.device(DEV)
    model, _ = get_model("zju377_mono", dev)
    model.eval()
    return model, scene.make_inputs(32, 32, frame_idx=0, device=dev)


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        if torch.is_tensor(a[k]):
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


@gpu
@pytest.mark.parametrize("method", ["lattice", "skinned"])
def test_posed_mesh_simplify_is_simplify_mesh_of_the_posed_mesh(subject, method):
    from arah_release_amd import geometry
    model, inputs = subject
    with torch.no_grad():
        plain = model.posed_mesh(inputs, n_side=33, method=method, indexed=True)
        _same(plain, model.posed_mesh(inputs, n_side=33, method=method, indexed=True, simplify=None))
        assert set(plain) == {"verts", "faces", "n_verts", "n_tris", "box", "counts"} and plain["n_tris"] > 100
        span = float((plain["verts"].max(0).values - plain["verts"].min(0).values).max())
        for simplify, kw in ((span / 12, {"cell": span / 12}), ({"resolution": 10, "position": "member"},) * 2):
            small = model.posed_mesh(inputs, n_side=33, method=method, indexed=True, simplify=simplify)
            expect = geometry.simplify_mesh(plain["verts"], plain["faces"], **kw)
            assert set(small) == set(plain) | {"vert_src", "removed", "cell", "dims"}
            assert 0 < small["n_tris"] < plain["n_tris"] and 0 < small["n_verts"] < plain["n_verts"]
            for k in expect:
                if torch.is_tensor(expect[k]):
                    assert small[k].dtype == expect[k].dtype and torch.equal(small[k], expect[k]), k
                else:
                    assert small[k] == expect[k], k
        both = model.posed_mesh(inputs, n_side=33, method=method, indexed=True, clean="largest", simplify=span / 12)
        cleaned = model.posed_mesh(inputs, n_side=33, method=method, indexed=True, clean="largest")
        expect = geometry.simplify_mesh(cleaned["verts"], cleaned["faces"], cell=span / 12)      # after clean
        assert torch.equal(both["verts"], expect["verts"]) and torch.equal(both["faces"], expect["faces"])
    with pytest.raises(ValueError):
        model.posed_mesh(inputs, n_side=33, method=method, simplify=0.1)          # a soup has no shared vertices
    with pytest.raises(ValueError):
        model.posed_mesh(inputs, n_side=33, method=method, indexed=True, simplify={"cell": 0.1, "resolution": 4})
    with pytest.raises(ValueError):
        model.posed_mesh(inputs, n_side=33, method=method, indexed=True, simplify="coarse")


@gpu
def test_canonical_mesh_simplifies_before_its_attributes(subject):
    from arah_release_amd import geometry, hip, training
    model, inputs = subject
    names = ("weights", "normal")
    with torch.no_grad():
        bare = model.canonical_mesh(inputs, n_side=33)
        _same(bare, model.canonical_mesh(inputs, n_side=33, simplify=None))
        plain = model.canonical_mesh(inputs, n_side=33, attributes=names)
        _same(plain, model.canonical_mesh(inputs, n_side=33, attributes=names, simplify=None))
        small = model.canonical_mesh(inputs, n_side=33, attributes=names, simplify=4.0 / 32)
        expect = geometry.simplify_mesh(bare["verts"], bare["faces"], cell=4.0 / 32)
        assert set(small) == set(plain) | {"vert_src", "removed", "cell", "dims"}
        for k in expect:
            if torch.is_tensor(expect[k]):
                assert torch.equal(small[k], expect[k]), k
            else:
                assert small[k] == expect[k], k
        V = small["n_verts"]
        assert 0 < V < plain["n_verts"] // 2 and small["weights"].shape == (V, 24) and small["normal"].shape == (V, 3)
        # the attributes are the networks' values AT the simplified positions, not gathered from the full mesh
        frame, ws = model._posed_frame(inputs, "test")
        verts = small["verts"].contiguous()
        x_hat = training.unnormalize_canonical_points(verts.reshape(1, -1, 3), inputs["coord_min"][:1], inputs["coord_max"][:1],
                                                      inputs["center"][:1])[0]
        assert torch.equal(small["weights"], hip.skin_lbs(frame, ws, x_hat)[0])
        grad = hip.sdf_eval(frame, ws, verts, want_grad=True)[2]
        assert torch.equal(small["normal"], grad / grad.norm(dim=1, keepdim=True).clamp_min(1e-20))
        assert not torch.equal(small["weights"], plain["weights"][small["vert_src"]])
        member = model.canonical_mesh(inputs, n_side=33, attributes=names, simplify={"cell": 4.0 / 32, "position": "member"})
        # a member IS a vertex of the full mesh, and the per-point kernels are row-independent (tests/test_pointwise_f64.py)
        assert torch.equal(member["verts"], plain["verts"][member["vert_src"]])
        for k in names:
            assert torch.equal(member[k], plain[k][member["vert_src"]]), k
    with pytest.raises(ValueError):
        model.canonical_mesh(inputs, n_side=33, simplify={"cell": -1.0})
