"""Connected components of indexed meshes and floater removal: arah_mesh_components / arah_mesh_select (csrc/meshcc.hpp), their
tensor specification meshing.mesh_components / meshing.mesh_select, geometry.mesh_components / geometry.clean_mesh and the `clean`
option of MetaAvatarRender.posed_mesh / canonical_mesh / geometry_metrics.

Connectivity is by shared vertex ids and everything is an integer, so every result is unique.  CPU tests hold the specification
to scipy.sparse.csgraph.connected_components and to numpy restatements; GPU tests hold the kernels to the specification with
torch.equal on every output, guard rows included."""
import ctypes as C
import fractions
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO, get_model

gpu = pytest.mark.gpu
DEV = "cuda:0"


# ---- fields on the lattice of [-1,1]^3 (those of tests/test_indexed_mesh.py, restated) ------------------------------------------
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


FIELDS = {"sphere17": lambda: sphere(17), "torus33": lambda: torus(33), "blobs33": lambda: two_blobs(33), "noise20": noise,
          "quantised17": lambda: quantised(17), "floaters33": body_with_floaters}
N_COMPONENTS = {"sphere17": 1, "torus33": 1, "blobs33": 2, "floaters33": 4}

_MESH = {}


def mesh(name):
    """(verts (V,3), faces (F,3) int64) of a named field on the host, computed once and shared; never modified."""
    from arah_release_amd import meshing
    if name not in _MESH:
        verts, faces, _ = meshing.marching_cubes_indexed(FIELDS[name]())
        _MESH[name] = (verts, faces)
    return _MESH[name]


# ---- independent oracles ------------------------------------------------------------------------------------------------------
def scipy_partition(faces, n_verts):
    """Component of every vertex by scipy on the vertex graph of the valid faces, renumbered by first occurrence (which is the
    ascending order of the components' smallest vertex ids); scipy's own numbering is not assumed."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    f = f[((f >= 0) & (f < n_verts)).all(1)]
    rows = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    cols = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    graph = coo_matrix((np.ones(rows.shape[0], np.int8), (rows, cols)), shape=(n_verts, n_verts))
    _, lab = connected_components(graph, directed=False)
    _, first = np.unique(lab, return_index=True)
    rank = np.empty(first.shape[0], np.int64)
    rank[np.argsort(first)] = np.arange(first.shape[0])
    return rank[lab] if n_verts else np.zeros(0, np.int64), f


def numpy_select(faces, n_verts, labels, keep):
    """Order-preserving compaction, restated with numpy: (vert_src, vert_map, faces_out, face_src) trimmed to their sizes."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    kept_v = np.asarray(keep)[np.asarray(labels, np.int64)] != 0 if n_verts else np.zeros(0, bool)
    vert_src = np.nonzero(kept_v)[0]
    vert_map = -np.ones(n_verts, np.int64)
    vert_map[vert_src] = np.arange(vert_src.shape[0])
    kept_f = np.array([all(0 <= i < n_verts and kept_v[i] for i in row) for row in f.tolist()], bool).reshape(-1)
    face_src = np.nonzero(kept_f)[0]
    return vert_src, vert_map, vert_map[f[face_src]].reshape(-1, 3), face_src


def check_select(out, faces, n_verts, labels, keep):
    """The five outputs of a mesh_select against the numpy restatement, guard rows included."""
    vert_src, vert_map, faces_out, face_src, counts = [np.asarray(t.cpu()) for t in out]
    rs, rm, rf, rfs = numpy_select(faces, n_verts, labels, keep)
    nv, nf = counts.tolist()
    assert (nv, nf) == (rs.shape[0], rfs.shape[0])
    assert vert_src.shape == (n_verts,) and vert_map.shape == (n_verts,) and faces_out.shape == (len(faces), 3)
    assert np.array_equal(vert_src[:nv], rs) and np.array_equal(vert_map, rm)
    assert np.array_equal(faces_out[:nf], rf) and np.array_equal(face_src[:nf], rfs)
    assert not vert_src[nv:].any() and not faces_out[nf:].any() and not face_src[nf:].any()
    assert bool((np.diff(vert_src[:nv]) > 0).all()) and bool((np.diff(face_src[:nf]) > 0).all())      # order preserved
    assert np.array_equal(vert_map[vert_src[:nv]], np.arange(nv))


# ---- CPU: the specification against scipy --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere17", "torus33", "blobs33", "noise20", "quantised17"])
def test_spec_partitions_like_scipy(name):
    from arah_release_amd import meshing
    verts, faces = mesh(name)
    V = verts.shape[0]
    labels, comp_verts, comp_faces, counts = meshing.mesh_components(faces, V)
    assert labels.dtype == comp_verts.dtype == comp_faces.dtype == counts.dtype == torch.int32
    assert labels.shape == comp_verts.shape == comp_faces.shape == (V,) and counts.shape == (3,)
    ref, fv = scipy_partition(faces.numpy(), V)
    assert np.array_equal(labels.numpy(), ref)
    n_comp = int(ref.max()) + 1
    # sizes are bincounts of that partition; entries beyond the component count are zero
    assert np.array_equal(comp_verts.numpy(), np.bincount(ref, minlength=V))
    assert np.array_equal(comp_faces.numpy(), np.bincount(ref[fv[:, 0]], minlength=V))
    # labels ascend with each component's smallest vertex id
    smallest = np.array([np.nonzero(ref == c)[0][0] for c in range(n_comp)])
    assert bool((np.diff(smallest) > 0).all()) and np.array_equal(labels.numpy()[smallest], np.arange(n_comp))
    cf = np.bincount(ref[fv[:, 0]], minlength=n_comp)
    assert counts.tolist() == [n_comp, fv.shape[0], int(np.argmax(cf))]      # numpy's argmax takes the first maximum
    if name in N_COMPONENTS:
        assert n_comp == N_COMPONENTS[name]
    if name == "noise20":
        assert n_comp > 20
    if name == "quantised17":   # coincident but distinct vertices exist, and only faces join them
        assert np.unique(verts.numpy(), axis=0).shape[0] < V


def test_spec_blobs_are_two_spheres():
    from arah_release_amd import meshing
    verts, faces = mesh("blobs33")
    labels, comp_verts, comp_faces, counts = meshing.mesh_components(faces, verts.shape[0])
    assert counts[0].item() == 2
    f = faces.numpy()
    for c in range(2):
        fc = f[labels.numpy()[f[:, 0]] == c]
        edges = np.sort(np.concatenate([fc[:, [0, 1]], fc[:, [1, 2]], fc[:, [2, 0]]]), axis=1)
        n_edges = np.unique(edges, axis=0).shape[0]
        assert int(comp_verts[c]) - n_edges + int(comp_faces[c]) == 2 and fc.shape[0] == int(comp_faces[c])


HAND_MADE = {
    # name: (faces, n_verts, labels, comp_verts, comp_faces, counts)
    "empty": ([], 0, [], [], [], [0, 0, -1]),
    "vertices_only": ([], 3, [0, 1, 2], [1, 1, 1], [0, 0, 0], [3, 0, 0]),
    "one_triangle": ([[0, 1, 2]], 3, [0, 0, 0], [3, 0, 0], [1, 0, 0], [1, 1, 0]),
    "shared_vertex": ([[0, 1, 2], [2, 3, 4]], 5, [0] * 5, [5, 0, 0, 0, 0], [2, 0, 0, 0, 0], [1, 2, 0]),
    "shared_edge": ([[0, 1, 2], [2, 1, 3]], 4, [0] * 4, [4, 0, 0, 0], [2, 0, 0, 0], [1, 2, 0]),
    "isolated_vertex": ([[0, 1, 3]], 4, [0, 0, 1, 0], [3, 1, 0, 0], [1, 0, 0, 0], [2, 1, 0]),
    "repeated_id": ([[1, 1, 2]], 4, [0, 1, 1, 2], [1, 2, 1, 0], [0, 1, 0, 0], [3, 1, 1]),
    "ids_out_of_range": ([[0, 1, -1], [0, 1, 5], [2, 3, 4]], 5, [0, 1, 2, 2, 2], [1, 1, 3, 0, 0], [0, 0, 1, 0, 0], [3, 1, 2]),
    "three_components": ([[5, 4, 3], [0, 1, 2], [6, 7, 8], [8, 7, 9]], 10, [0, 0, 0, 1, 1, 1, 2, 2, 2, 2],
                         [3, 3, 4] + [0] * 7, [1, 1, 2] + [0] * 7, [3, 4, 2]),
    "tie_lowest_id_wins": ([[5, 4, 3], [0, 1, 2]], 6, [0, 0, 0, 1, 1, 1], [3, 3, 0, 0, 0, 0], [1, 1, 0, 0, 0, 0], [2, 2, 0]),
}


def _faces_tensor(rows, dtype=torch.int64):
    return torch.tensor(rows, dtype=dtype).reshape(-1, 3)


@pytest.mark.parametrize("name", sorted(HAND_MADE))
def test_spec_hand_made_graphs(name):
    from arah_release_amd import meshing
    rows, V, labels, comp_verts, comp_faces, counts = HAND_MADE[name]
    for dtype in (torch.int64, torch.int32):
        out = meshing.mesh_components(_faces_tensor(rows, dtype), V)
        assert [t.tolist() for t in out] == [labels, comp_verts, comp_faces, counts]
    ref, _ = scipy_partition(np.array(rows, np.int64).reshape(-1, 3), V)
    assert ref.tolist() == labels


def _keep_vectors(comp_faces, counts):
    """Keep vectors that exercise the compaction: the largest, all, none, every other component, those with >= 2 faces."""
    V = comp_faces.shape[0]
    ids = torch.arange(V)
    return {"largest": (ids == counts[2]).to(torch.int32), "all": torch.ones(V, dtype=torch.int32),
            "none": torch.zeros(V, dtype=torch.int32), "odd": (ids % 2).to(torch.int32) * 7,
            "two_faces": (comp_faces >= 2).to(torch.int32)}


@pytest.mark.parametrize("name", ["floaters33", "noise20", "blobs33"])
def test_spec_select_is_the_numpy_restatement(name):
    from arah_release_amd import meshing
    verts, faces = mesh(name)
    V = verts.shape[0]
    labels, _, comp_faces, counts = meshing.mesh_components(faces, V)
    for which, keep in _keep_vectors(comp_faces, counts).items():
        out = meshing.mesh_select(faces, V, labels, keep)
        assert all(t.dtype == torch.int32 for t in out), which
        check_select(out, faces.numpy(), V, labels.numpy(), keep.numpy())


def test_spec_select_hand_made():
    from arah_release_amd import meshing
    rows, V = HAND_MADE["ids_out_of_range"][:2]
    faces = _faces_tensor(rows)
    labels = meshing.mesh_components(faces, V)[0]
    out = meshing.mesh_select(faces, V, labels, torch.tensor([0, 1, 1, 0, 0], dtype=torch.int32))
    assert [t.tolist() for t in out] == [[1, 2, 3, 4, 0], [-1, 0, 1, 2, 3], [[1, 2, 3], [0, 0, 0], [0, 0, 0]], [2, 0, 0], [4, 1]]
    check_select(out, rows, V, labels.numpy(), [0, 1, 1, 0, 0])
    out = meshing.mesh_select(_faces_tensor([]), 0, torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.int32))
    assert [tuple(t.shape) for t in out] == [(0,), (0,), (0, 3), (0,), (2,)] and out[4].tolist() == [0, 0]
    with pytest.raises(ValueError):
        meshing.mesh_select(faces, V, labels[:-1], torch.ones(V, dtype=torch.int32))
    with pytest.raises(ValueError):
        meshing.mesh_select(faces, V, labels, torch.ones(V))
    with pytest.raises(ValueError):
        meshing.mesh_components(faces.float(), V)
    with pytest.raises(ValueError):
        meshing.mesh_components(faces.reshape(-1), V)
    with pytest.raises(ValueError):
        meshing.mesh_components(faces, -1)


def _expected_kept_components(comp_faces, keep):
    """Which components a `keep` policy retains, in Python integers (the share as the exact value of the float)."""
    cf = [int(c) for c in comp_faces]
    most = max(cf) if cf else 0
    if keep == "largest":
        return [c == cf.index(most) for c in range(len(cf))]
    if keep == "referenced":
        return [n > 0 for n in cf]
    if isinstance(keep, int):
        return [n >= keep for n in cf]
    need = math.ceil(fractions.Fraction(keep) * most)
    return [n >= need for n in cf]


KEEPS = ["largest", "referenced", 0, 1, 150, 10 ** 6, 1.0, 0.5, 0.1, 0.02, 1e-9]


@pytest.mark.parametrize("keep", KEEPS, ids=[str(k) for k in KEEPS])
def test_clean_mesh_on_the_host(keep):
    from arah_release_amd import geometry
    verts, faces = mesh("floaters33")
    extra = torch.tensor([[3.0, 3.0, 3.0], [4.0, 4.0, 4.0]])                       # two vertices no face names
    verts = torch.cat([verts[:100], extra, verts[100:]])
    faces = torch.where(faces >= 100, faces + 2, faces)
    faces = torch.cat([faces[:50], torch.tensor([[0, 1, -1], [0, 1, verts.shape[0]]]), faces[50:]])   # two faces to be skipped
    V, F = verts.shape[0], faces.shape[0]
    ref, fv = scipy_partition(faces.numpy(), V)
    n_comp = int(ref.max()) + 1
    assert n_comp == 6
    cf = np.bincount(ref[fv[:, 0]], minlength=n_comp)
    sizes = sorted(cf.tolist())
    assert sizes[0] == sizes[1] == 0 and len(set(sizes[2:])) == 4 and sizes[2] < 150 < sizes[3]
    kept_c = np.array(_expected_kept_components(cf, keep))
    weights = torch.arange(V * 2, dtype=torch.float32).reshape(V, 2)
    res = geometry.clean_mesh(verts, faces, keep=keep, attributes={"weights": weights, "ids": torch.arange(V)})
    rs, rm, rf, rfs = numpy_select(faces.numpy(), V, ref, kept_c)
    assert res["n_verts"] == rs.shape[0] == res["verts"].shape[0] and res["n_tris"] == rf.shape[0] == res["faces"].shape[0]
    assert res["faces"].dtype == faces.dtype and res["vert_src"].dtype == torch.int64
    assert np.array_equal(res["vert_src"].numpy(), rs) and np.array_equal(res["faces"].numpy(), rf)
    assert torch.equal(res["verts"], verts[res["vert_src"]])
    assert torch.equal(res["weights"], weights[res["vert_src"]]) and torch.equal(res["ids"], res["vert_src"])
    assert res["removed"] == {"components": int((~kept_c).sum()), "vertices": V - rs.shape[0], "faces": F - rf.shape[0]}
    assert res["removed"]["faces"] >= 2
    if keep == "largest":
        assert res["n_tris"] == int(cf.max()) and res["removed"]["components"] == 5
    if keep == "referenced":
        assert res["removed"] == {"components": 2, "vertices": 2, "faces": 2}
    if keep == 10 ** 6:
        assert res["n_verts"] == 0 and res["n_tris"] == 0 and res["verts"].shape == (0, 3)
    # cleaning a clean mesh changes nothing
    again = geometry.clean_mesh(res["verts"], res["faces"], keep=keep)
    if res["n_tris"]:
        assert torch.equal(again["verts"], res["verts"]) and torch.equal(again["faces"], res["faces"])
        assert again["removed"] == {"components": 0, "vertices": 0, "faces": 0}
        assert torch.equal(again["vert_src"], torch.arange(res["n_verts"]))


def test_clean_mesh_largest_of_the_two_blobs():
    from arah_release_amd import geometry
    verts, faces = mesh("blobs33")
    ref, fv = scipy_partition(faces.numpy(), verts.shape[0])
    cf = np.bincount(ref[fv[:, 0]])
    assert cf.shape[0] == 2 and cf[0] != cf[1]
    res = geometry.clean_mesh(verts, faces.to(torch.int32))
    assert res["n_tris"] == int(cf.max()) and res["faces"].dtype == torch.int32
    assert res["removed"] == {"components": 1, "vertices": int((ref == np.argmin(cf)).sum()), "faces": int(cf.min())}
    assert torch.equal(res["verts"][res["faces"].long()], verts[faces[torch.from_numpy(ref[faces.numpy()[:, 0]] == np.argmax(cf))]])
    comps = geometry.mesh_components(verts, faces)
    assert comps["n_components"] == 2 and comps["comp_faces"].tolist() == cf.tolist() and comps["largest"] == int(np.argmax(cf))
    assert comps["comp_verts"].shape == (2,) and np.array_equal(comps["labels"].numpy(), ref)
    assert geometry.mesh_components(verts.shape[0], faces)["comp_verts"].tolist() == comps["comp_verts"].tolist()


@pytest.mark.parametrize("keep", ["biggest", True, False, -1, 0.0, 1.5, -0.5, float("nan"), None, [1]])
def test_clean_mesh_rejects_bad_keep(keep):
    from arah_release_amd import geometry
    verts, faces = mesh("sphere17")
    with pytest.raises(ValueError):
        geometry.clean_mesh(verts, faces, keep=keep)


def test_share_threshold_is_exact_in_integers():
    """ceil(share * largest) for floats whose product with the count needs more than 64 bits, against Python's rationals."""
    from arah_release_amd import geometry
    g = torch.Generator().manual_seed(3)
    shares = [1.0, 0.5, 0.1, 0.7, 1e-9, 5e-324, 2.0 ** -26, 2.0 ** -27, 3 * 2.0 ** -28, 1 / 3, 1 - 2.0 ** -53]
    shares += (torch.rand(200, generator=g, dtype=torch.float64) ** 8).clamp_min(1e-300).tolist()
    for share in shares:
        policy = geometry.check_keep(share)
        assert policy[0] == "share" and fractions.Fraction(policy[1], 2 ** policy[2]) == fractions.Fraction(share)
        for most in (0, 1, 10, 1928, 98636, 2 ** 31 - 1):
            got = int(geometry.ceil_share(torch.tensor(most), policy[1], policy[2]))
            assert got == math.ceil(fractions.Fraction(share) * most), (share, most)


def test_clean_mesh_rejects_bad_shapes():
    from arah_release_amd import geometry
    verts, faces = mesh("sphere17")
    V = verts.shape[0]
    for bad_v, bad_f in ((verts[:, :2], faces), (verts, faces[:, :2]), (verts, faces.float()), (verts.reshape(-1), faces), (V, faces)):
        with pytest.raises(ValueError):
            geometry.clean_mesh(bad_v, bad_f)
    with pytest.raises(ValueError):
        geometry.clean_mesh(verts, faces, attributes={"w": torch.zeros(V + 1, 24)})
    with pytest.raises(ValueError):
        geometry.clean_mesh(verts, faces, attributes={"verts": torch.zeros(V, 3)})
    with pytest.raises(ValueError):
        geometry.mesh_components(verts, faces.float())
    with pytest.raises(ValueError):
        geometry.mesh_components(-3, faces)


def test_component_symbols_are_declared_and_exported():
    from arah_release_amd import hip
    header = open(os.path.join(REPO, "include", "arah_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = hip.load_library()
    for name in ("arah_mesh_components_scratch_bytes", "arah_mesh_components", "arah_mesh_select_scratch_bytes", "arah_mesh_select"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in hip.EXPORTS, name
        assert getattr(lib, name) is not None
    # sizes that 32-bit ids cannot hold, and negative ones, have no scratch size (host code: no GPU involved)
    for query in (lib.arah_mesh_components_scratch_bytes, lib.arah_mesh_select_scratch_bytes):
        assert query(0, 0) > 0 and query(2 ** 31 - 1, 2 ** 31 - 1) > 0
        assert query(-1, 0) == 0 and query(0, -1) == 0 and query(2 ** 31, 0) == 0 and query(0, 2 ** 31) == 0


# Every literal below is what the library of commit e16eaee (the last one with a hand-written layout per entry) returned, run on
# the host: callers size their buffers with these queries, so the shared scratch carver must not move a byte.  0 = a rejected size.
_BIG = (2 ** 31 - 1, 2 ** 28)
_VF = ((0, 0), (1, 1), (1024, 1024), (1025, 1025), (1000, 2000), _BIG, (2 ** 31, 0))
SCRATCH_BYTES = {
    "mesh_components": (16, 36, 12312, 12332, 12024, 25786580996, 0),
    "mesh_select": (16, 32, 32, 48, 40, 18874384, 0),
    "mesh_adjacency": (256, 1280, 69632, 70912, 128512, 33285996544, 0),
    "mesh_orient": (256, 1792, 22016, 23296, 43264, 5639241728, 0),
    "mesh_boundary_loops": (256, 2560, 25600, 27136, 25600, 51562676224, 0),
    "mesh_fill_holes": (256, 1792, 33792, 34560, 33280, 68742545408, 0),
}
SIMPLIFY_BYTES = {    # (V, F) -> n_cells = 1, 1000, 2^27; simplification takes at most 2^26 vertices, so _BIG is its rejected size
    (0, 0): (768, 768, 50331648), (1, 1): (3328, 3328, 50334208), (1024, 1024): (70912, 70912, 50401792),
    (1025, 1025): (96768, 96768, 50427648), (1000, 2000): (99072, 99072, 50429952), _BIG: (0, 0, 0),
}
MCUBES_BYTES = {2: 72, 33: 160652, 894: 2870841416, 895: 0}    # 3 * 895^3 edge keys do not fit int32


def test_scratch_sizes_of_the_indexed_mesh_entries_are_those_of_the_hand_written_layouts():
    from arah_release_amd import hip
    lib = hip.load_library()
    for name, want in SCRATCH_BYTES.items():
        query = getattr(lib, "arah_%s_scratch_bytes" % name)
        assert tuple(int(query(v, f)) for v, f in _VF) == want, name
    for (v, f), want in SIMPLIFY_BYTES.items():
        assert tuple(int(lib.arah_mesh_simplify_scratch_bytes(v, f, c)) for c in (1, 1000, 2 ** 27)) == want, (v, f)
    assert int(lib.arah_mesh_simplify_scratch_bytes(1, 1, 0)) == 0
    assert {n: int(lib.arah_marching_cubes_indexed_scratch_bytes(n)) for n in MCUBES_BYTES} == MCUBES_BYTES
    # The one value that is NOT e16eaee's: its simplify layout took max() of two size_t through a 32-bit overload and returned
    # 1612710656, this sum modulo 2^32, for the largest mesh it accepts -- and the entry checked the caller's buffer against that.
    # The blocks add up to: bitmap, wcount, wbase 256 each; vkey 2^28; sums 3 * 2^29; members 2^28; best 2^29; fslot 2^30; 2^29
    # slots of 8 + 4 bytes; two block arrays of 2^18 ints
    want = 3 * 256 + 2 ** 28 + 3 * 2 ** 29 + 2 ** 28 + 2 ** 29 + 2 ** 30 + 12 * 2 ** 29 + 2 * 2 ** 20
    assert want == 10202645248 and want % 2 ** 32 == 1612710656
    assert int(lib.arah_mesh_simplify_scratch_bytes(2 ** 26, 2 ** 28, 1)) == want


# The query side.  Every literal below is what the library of commit e191f2c (the last one with a hand-written layout per index)
# returned, run on the host: from the smallest to the largest size each query accepts, then the sizes it rejects (0).
_N = (1, 2, 1000, 1024, 1025, 100000, 2 ** 20, 2 ** 26, 2 ** 27, 2 ** 31 - 1, 0, -1)
INDEX_BYTES = {
    "contains_index": (((0, 2), (1, 2), (1000, 512), (1025, 513), (2 ** 28, 4096), (0, 4096),
                        (-1, 512), (2 ** 28 + 1, 512), (5, 1), (5, 4097), (5, 0)),
                       (1024, 2048, 2251008, 2264064, 40936473088, 134283776, 0, 0, 0, 0, 0)),
    "winding_index": (((0, 0), (0, -1), (1, -1), (1000, -1), (1025, 3), (2 ** 28, 7), (2 ** 28, -1), (7, 7),     # depth -1: chosen from F
                       (-1, 0), (2 ** 28 + 1, 0), (5, 8), (5, -2)),
                      (1024, 1024, 2304, 66048, 38912, 8606712576, 8606712576, 16779264, 0, 0, 0, 0)),
    "mesh_index": (tuple((n,) for n in _N),
                   (58368, 58368, 93952, 94720, 96000, 7617280, 79708672, 2457879040, 4873798144, 77351371264, 0, 0)),
    "point_index": (tuple((n,) for n in _N),
                    (1156864, 1156864, 1212160, 1213952, 1214976, 10715648, 101778944, 1242629632, 2316371456, 34528626176, 0, 0)),
    "mesh_sdf_grid": (((0, 1, 1, 1), (1, 1, 1, 1), (1000, 5, 3, 70), (1025, 33, 17, 65), (2 ** 26, 1290, 1290, 1290), (2 ** 26, 2 ** 31 - 1, 1, 1),
                       (-1, 1, 1, 1), (2 ** 26 + 1, 1, 1, 1), (1, 0, 1, 1), (1, 2 ** 31, 1, 1), (1, 2 ** 16, 2 ** 16, 1), (1, 2048, 1024, 1024)),
                      (256, 1024, 32512, 33792, 2147483904, 2147483904, 0, 0, 0, 0, 0, 0)),
}


def test_index_sizes_of_the_query_side_are_those_of_the_hand_written_layouts():
    from arah_release_amd import hip
    lib = hip.load_library()
    for name, (sizes, want) in INDEX_BYTES.items():
        query = getattr(lib, "arah_%s_bytes" % name)
        assert tuple(int(query(*a)) for a in sizes) == want, name


# ---- GPU: the kernels against the specification ---------------------------------------------------------------------------------
def strip(n_faces):
    i = torch.arange(n_faces)
    return torch.stack([i, i + 1, i + 2], 1)


def _stress_graphs():
    g = torch.Generator().manual_seed(5)
    s = strip(2999)                                                              # 3 001 vertices
    cases = {"strip_ascending": (s, 3001), "strip_descending": (3000 - s, 3001),
             "strip_permuted": (torch.randperm(3001, generator=g)[s], 3001),
             "disjoint_triangles_2049": (torch.randperm(6147, generator=g).reshape(2049, 3), 6147),
             "fan_1025": (torch.stack([torch.zeros(1025, dtype=torch.int64), torch.arange(1, 1026), torch.arange(2, 1027)], 1), 1027),
             "empty": (torch.zeros(0, 3, dtype=torch.int64), 0), "vertices_only_70": (torch.zeros(0, 3, dtype=torch.int64), 70),
             "faces_without_vertices": (strip(5), 0)}
    for F in (1, 63, 64, 65, 1023, 1025):                                        # V = F + 5: never a multiple of 64
        f = strip(F)[torch.randperm(F, generator=g)]
        cases["strip_F%d" % F] = (torch.where(f >= F // 2 + 1, f + 3, f), F + 5)   # three isolated vertices in the middle
    bad = strip(130).clone()
    bad[7, 1], bad[64, 0], bad[129, 2] = -1, 132, 2 ** 31 - 1                     # three faces to be skipped
    cases["strip_with_bad_ids"] = (bad, 132)
    return cases


STRESS = _stress_graphs()
KERNEL_FIELDS = ["sphere17", "torus33", "blobs33", "noise20", "quantised17", "floaters33"]


def _kernels_against_spec(faces, V):
    from arah_release_amd import hip, meshing
    ref = meshing.mesh_components(faces, V)
    d = faces.to(DEV).to(torch.int32)
    got = hip.mesh_components(d, V)
    for r, g in zip(ref, got):
        assert g.dtype == torch.int32 and g.device.type == "cuda" and torch.equal(g.cpu(), r)
    for which, keep in _keep_vectors(ref[2], ref[3]).items():
        ref_s = meshing.mesh_select(faces, V, ref[0], keep)
        got_s = hip.mesh_select(d, V, got[0], keep.to(DEV))
        for r, g in zip(ref_s, got_s):
            assert g.dtype == torch.int32 and torch.equal(g.cpu(), r), which
    return ref


@gpu
@pytest.mark.parametrize("name", KERNEL_FIELDS)
def test_kernels_are_the_specification_on_level_sets(name):
    verts, faces = mesh(name)
    ref = _kernels_against_spec(faces, verts.shape[0])
    if name in N_COMPONENTS:
        assert ref[3][0].item() == N_COMPONENTS[name]


@gpu
@pytest.mark.parametrize("name", sorted(STRESS))
def test_kernels_are_the_specification_on_stress_graphs(name):
    faces, V = STRESS[name]
    assert V % 64 != 0 or V == 0
    ref = _kernels_against_spec(faces, V)
    n_comp = ref[3][0].item()
    if name.startswith("strip_F"):
        assert n_comp == 4
    if name in ("strip_ascending", "strip_descending", "strip_permuted", "fan_1025"):
        assert n_comp == 1
    if name == "disjoint_triangles_2049":
        assert n_comp == 2049 and 2049 * 3 > 4 * 1024                            # more than one block of the count / scan / fill
    if name == "strip_with_bad_ids":
        assert ref[3].tolist()[:2] == [2, 127]                              # vertex 131 lost its only face
    if name == "faces_without_vertices":
        assert ref[3].tolist() == [0, 0, -1]


@gpu
def test_binding_takes_int64_faces_and_validates():
    from arah_release_amd import hip, meshing
    faces, V = STRESS["strip_with_bad_ids"]
    big = faces.clone()
    big[3, 0] = 2 ** 40                                                          # does not fit int32: skipped, not wrapped
    ref = meshing.mesh_components(big, V)
    got = hip.mesh_components(big.to(DEV), V)
    for r, g in zip(ref, got):
        assert torch.equal(g.cpu(), r)
    for dtype in (torch.int16, torch.uint8):                                     # narrower than int32: cast, never compared with 2^31
        small = STRESS["strip_F63"][0].to(dtype)
        for r, g in zip(meshing.mesh_components(small, 68), hip.mesh_components(small.to(DEV), 68)):
            assert torch.equal(g.cpu(), r)
    d = faces.to(DEV)
    for bad in (lambda: hip.mesh_components(d.float(), V), lambda: hip.mesh_components(d.reshape(-1), V),
                lambda: hip.mesh_components(d, -1), lambda: hip.mesh_components(d, 2 ** 31), lambda: hip.mesh_components(faces, V),
                lambda: hip.mesh_select(d, V, got[0][:-1], got[1]), lambda: hip.mesh_select(d, V, got[0], got[1].float()),
                lambda: hip.mesh_select(d, V, got[0].cpu(), got[1])):
        with pytest.raises(ValueError):
            bad()


@gpu
@pytest.mark.parametrize("keep", ["largest", 150, 0.1, "referenced", 10 ** 6], ids=str)
def test_clean_mesh_on_the_device_drops_floaters_like_the_host(keep):
    from arah_release_amd import geometry
    verts, faces = mesh("floaters33")
    weights = torch.arange(verts.shape[0] * 2, dtype=torch.float32).reshape(-1, 2)
    ref = geometry.clean_mesh(verts, faces, keep=keep, attributes={"weights": weights})
    got = geometry.clean_mesh(verts.to(DEV), faces.to(DEV).to(torch.int32), keep=keep, attributes={"weights": weights.to(DEV)})
    if keep in ("largest", 150, 0.1):
        assert 0 < ref["n_verts"] < verts.shape[0] and ref["removed"]["components"] > 0      # vertices really go
    assert set(got) == set(ref) and got["faces"].dtype == torch.int32
    for k in ref:
        if torch.is_tensor(ref[k]):
            assert torch.equal(got[k].cpu().long() if k == "faces" else got[k].cpu(), ref[k]), k
        else:
            assert got[k] == ref[k], k


@gpu
def test_kernels_are_deterministic_and_isolated():
    from arah_release_amd import hip
    small_f, small_v = STRESS["strip_permuted"]
    big_f, big_v = STRESS["disjoint_triangles_2049"]
    ds, db = small_f.to(DEV).to(torch.int32), big_f.to(DEV).to(torch.int32)

    def run(d, V):
        comps = hip.mesh_components(d, V)
        keep = (torch.arange(V, device=DEV) % 2 == 0).to(torch.int32)
        return comps + hip.mesh_select(d, V, comps[0], keep)

    hip._mesh_cc_scratch.clear()
    fresh = run(ds, small_v)
    again = run(ds, small_v)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        first_on_side = run(db, big_v)                                           # sizes this stream's scratch
        other = run(ds, small_v)                                                 # ... and reuses it
        side_key = (torch.device(DEV), side.cuda_stream)
        assert side_key in hip._mesh_cc_scratch
    side.synchronize()
    big = run(db, big_v)                                                         # a larger mesh on this stream's scratch
    key = (torch.device(DEV), torch.cuda.current_stream().cuda_stream)
    grown = hip._mesh_cc_scratch[key]
    after = run(ds, small_v)                                                     # the smaller one on what it left behind
    assert hip._mesh_cc_scratch[key] is grown
    for other_run in (again, other, after):
        for a, b in zip(fresh, other_run):
            assert torch.equal(a, b)
    for a, b in zip(first_on_side, big):
        assert torch.equal(a, b)
    _kernels_against_spec(small_f, small_v)


@gpu
def test_abi_writes_nothing_beyond_its_arrays_and_refuses_bad_sizes():
    from arah_release_amd import hip, meshing
    lib = hip.load_library()
    faces, V = STRESS["strip_with_bad_ids"]
    F, guard, mark = faces.shape[0], 64, 0x5EA1BEEF
    d = faces.to(DEV).to(torch.int32)
    ref = meshing.mesh_components(faces, V)
    keep = (ref[2] >= 2).to(torch.int32)
    ref_s = meshing.mesh_select(faces, V, ref[0], keep)
    new = lambda n: torch.full((n + guard,), mark, dtype=torch.int32, device=DEV)
    labels, comp_verts, comp_faces, counts = new(V), new(V), new(V), new(3)
    vert_src, vert_map, faces_out, face_src, kept = new(V), new(V), new(3 * F), new(F), new(2)
    scratch = torch.empty(int(max(lib.arah_mesh_components_scratch_bytes(V, F), lib.arah_mesh_select_scratch_bytes(V, F))),
                          dtype=torch.uint8, device=DEV)
    keep_d = keep.to(DEV)

    def components(n_faces, n_verts, nbytes):
        return lib.arah_mesh_components(hip._ptr(d), C.c_int64(n_faces), C.c_int64(n_verts), hip._ptr(labels), hip._ptr(comp_verts),
                                        hip._ptr(comp_faces), hip._ptr(counts), hip._ptr(scratch), C.c_size_t(nbytes), hip._stream())

    def select(n_faces, n_verts, nbytes):
        return lib.arah_mesh_select(hip._ptr(d), C.c_int64(n_faces), C.c_int64(n_verts), hip._ptr(labels), hip._ptr(keep_d),
                                    hip._ptr(vert_src), hip._ptr(vert_map), hip._ptr(faces_out), hip._ptr(face_src), hip._ptr(kept),
                                    hip._ptr(scratch), C.c_size_t(nbytes), hip._stream())

    with hip._on_device(torch.device(DEV)):
        # refused without a launch: every output still holds the mark
        for call in (components, select):
            assert call(-1, V, scratch.numel()) == -1 and call(F, -1, scratch.numel()) == -1                # ARAH_E_BADARG
            assert call(2 ** 31, V, scratch.numel()) == -1 and call(F, 2 ** 31, scratch.numel()) == -1
            assert call(F, V, 8) == -3                                                                        # ARAH_E_WORKSPACE
        torch.cuda.synchronize()
        for buf in (labels, comp_verts, comp_faces, counts, vert_src, vert_map, faces_out, face_src, kept):
            assert bool((buf == mark).all())
        assert components(F, V, scratch.numel()) == 0 and select(F, V, scratch.numel()) == 0
    for buf, r, n in ((labels, ref[0], V), (comp_verts, ref[1], V), (comp_faces, ref[2], V), (counts, ref[3], 3),
                      (vert_src, ref_s[0], V), (vert_map, ref_s[1], V), (faces_out, ref_s[2].reshape(-1), 3 * F),
                      (face_src, ref_s[3], F), (kept, ref_s[4], 2)):
        assert torch.equal(buf[:n].cpu(), r) and bool((buf[n:] == mark).all())


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
def test_posed_mesh_clean_is_clean_mesh_of_the_posed_mesh(subject, method):
    from arah_release_amd import geometry
    model, inputs = subject
    with torch.no_grad():
        plain = model.posed_mesh(inputs, n_side=64, method=method, indexed=True)
        none = model.posed_mesh(inputs, n_side=64, method=method, indexed=True, clean=None)
        cleaned = model.posed_mesh(inputs, n_side=64, method=method, indexed=True, clean="largest")
    assert set(plain) == {"verts", "faces", "n_verts", "n_tris", "box", "counts"} and plain["n_tris"] > 100
    _same(plain, none)                                                            # clean=None: today's keys and tensors
    expect = geometry.clean_mesh(plain["verts"], plain["faces"], keep="largest")
    assert set(cleaned) == set(plain) | {"vert_src", "removed"}
    for k in expect:
        if torch.is_tensor(expect[k]):
            assert torch.equal(cleaned[k], expect[k]), k
        else:
            assert cleaned[k] == expect[k], k
    comps = geometry.mesh_components(cleaned["verts"], cleaned["faces"])
    assert comps["n_components"] == 1 and comps["comp_faces"].tolist() == [cleaned["n_tris"]]
    # the kernels' labelling of the posed mesh against scipy's
    ref, _ = scipy_partition(plain["faces"].cpu().numpy(), plain["n_verts"])
    assert np.array_equal(geometry.mesh_components(plain["n_verts"], plain["faces"])["labels"].cpu().numpy(), ref)
    assert cleaned["removed"]["components"] == int(ref.max())
    # the synthetic subject is ONE component, so "largest" drops nothing above; a face count nothing reaches drops everything
    with torch.no_grad():
        nothing = model.posed_mesh(inputs, n_side=64, method=method, indexed=True, clean=2 ** 31 - 1)
    assert nothing["n_verts"] == 0 and nothing["n_tris"] == 0 and nothing["verts"].shape == (0, 3) and nothing["faces"].shape == (0, 3)
    assert nothing["removed"] == {"components": int(ref.max()) + 1, "vertices": plain["n_verts"], "faces": plain["n_tris"]}
    with pytest.raises(ValueError):
        model.posed_mesh(inputs, n_side=64, method=method, clean="largest")      # a soup has no shared vertices
    with pytest.raises(ValueError):
        model.posed_mesh(inputs, n_side=64, method=method, indexed=True, clean="nope")


@gpu
def test_canonical_mesh_cleans_before_its_attributes(subject):
    from arah_release_amd import geometry
    model, inputs = subject
    names = ("weights", "verts_posed", "normal", "color")
    with torch.no_grad():
        bare = model.canonical_mesh(inputs, n_side=64)
        _same(bare, model.canonical_mesh(inputs, n_side=64, clean=None))
        assert set(bare) == {"verts", "faces", "n_verts", "n_tris"}
        plain = model.canonical_mesh(inputs, n_side=64, attributes=names)
        _same(plain, model.canonical_mesh(inputs, n_side=64, attributes=names, clean=None))
        cleaned = model.canonical_mesh(inputs, n_side=64, attributes=names, clean="largest")
    expect = geometry.clean_mesh(plain["verts"], plain["faces"], keep="largest")
    assert set(cleaned) == set(plain) | {"vert_src", "removed"}
    for k in ("verts", "faces", "vert_src"):
        assert torch.equal(cleaned[k], expect[k]), k
    assert (cleaned["n_verts"], cleaned["n_tris"], cleaned["removed"]) == (expect["n_verts"], expect["n_tris"], expect["removed"])
    # the per-point kernels are row-independent (tests/test_pointwise_f64.py): evaluating fewer vertices changes no bit of the others
    for k in names:
        assert torch.equal(cleaned[k], plain[k][cleaned["vert_src"]]), k
    # the subject is one component: vert_src above is the identity.  Dropping everything takes the other way out: no vertex
    # is left, and no attribute kernel is launched for none
    with torch.no_grad():
        nothing = model.canonical_mesh(inputs, n_side=64, attributes=names, clean=2 ** 31 - 1)
    assert nothing["n_verts"] == 0 and nothing["n_tris"] == 0 and nothing["removed"]["vertices"] == plain["n_verts"]
    assert [tuple(nothing[k].shape) for k in names] == [(0, 24), (0, 3), (0, 3), (0, 3)]
    with pytest.raises(ValueError):
        model.canonical_mesh(inputs, n_side=64, clean=2.0)


@gpu
def test_geometry_metrics_clean_and_file_round_trip(subject, tmp_path):
    from arah_release_amd import geometry
    model, inputs = subject
    with torch.no_grad():
        cleaned = model.posed_mesh(inputs, n_side=64, indexed=True, clean="largest")
        gt = (cleaned["verts"], cleaned["faces"])
        with_clean = model.geometry_metrics(inputs, gt, n_side=64, n_samples=20000, clean="largest")
        without = model.geometry_metrics(inputs, gt, n_side=64, n_samples=20000)
        _same(without, model.geometry_metrics(inputs, gt, n_side=64, n_samples=20000, clean=None))
    print("chamfer_l1 cleaned %.3e uncleaned %.3e, removed %s" % (float(with_clean["chamfer_l1"]), float(without["chamfer_l1"]),
                                                                  cleaned["removed"]))
    assert with_clean["n_tris"] == cleaned["n_tris"] <= without["n_tris"]
    assert float(with_clean["chamfer_l1"]) <= float(without["chamfer_l1"])
    for ext in (".npz", ".ply"):
        path = str(tmp_path / ("cleaned" + ext))
        geometry.save_mesh(path, cleaned["verts"], cleaned["faces"])
        v, f = geometry.load_mesh(path, device=cleaned["verts"].device)
        assert torch.equal(v, cleaned["verts"]) and torch.equal(f, cleaned["faces"].long())
