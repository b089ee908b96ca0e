"""Edge flips on the host: the tensor specification meshing.mesh_flip_round against a numpy float64 restatement written with
python loops (bit for bit: faces, flags, counts, keys, reasons, selection), the cases with a known answer (tetrahedron, a flat
bipyramid, rims, fins, misoriented faces, non-finite vertices, a kite between boundary vertices), jittered planar grids against
scipy's Delaunay triangulation, the valence criterion's bookkeeping, the topology of a closed mesh, and the argument checks.
Everything here runs on the host; tests/test_mesh_flip_gpu.py holds the kernels of csrc/meshflip.hpp to the specification."""
import os
import re

import numpy as np
import pytest
import torch

from test_mesh_collapse import mesh as collapse_mesh
from test_mesh_quadric import flat_grid

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("arah_mesh_flip_round_scratch_bytes", "arah_mesh_flip_round")
NAMES = ("edges", "candidates", "selected", "not_interior", "same_corner", "exists", "nonfinite", "criterion", "normals")
CRITERIA = ("delaunay", "valence")
_MESH, _SPEC = {}, {}


# ---- meshes -------------------------------------------------------------------------------------------------------------------------
def jittered_grid(n, seed, amount=0.25):
    """n x n vertices on the integer lattice of the plane z = 0, every cell cut along the same diagonal; the interior vertices
    moved by up to `amount` of a cell in x and y, the rim unmoved."""
    verts, faces = flat_grid(n - 1)
    verts = (verts * (n - 1)).round()
    verts[:, 2] = 0.0
    inner = ((verts[:, :2] > 0) & (verts[:, :2] < n - 1)).all(1)
    shift = np.random.RandomState(seed).uniform(-amount, amount, (verts.shape[0], 2)).astype(np.float32)
    verts[:, :2] += torch.from_numpy(shift) * inner[:, None]
    return verts, faces


def flat_bipyramid(h=0.3):
    """Two apexes (3 above, 4 below) close to the centre of the ring (0, 1, 2): the angles at the apexes opposite to a ring edge
    are obtuse, so every ring edge fails the Delaunay test, and the flip of each would create the edge {3, 4}."""
    r = [[np.cos(a), np.sin(a), 0.0] for a in (0.0, 2.0 * np.pi / 3.0, 4.0 * np.pi / 3.0)]
    verts = torch.tensor(r + [[0.0, 0.0, h], [0.0, 0.0, -h]], dtype=torch.float32)
    return verts, torch.tensor([[0, 1, 3], [1, 2, 3], [2, 0, 3], [1, 0, 4], [2, 1, 4], [0, 2, 4]])


def kite():
    """Two faces on the long diagonal (0, 1) of a kite; all four vertices lie on the boundary, the diagonal is interior."""
    verts = torch.tensor([[-2.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 0.5, 0.0], [0.0, -0.5, 0.0]])
    return verts, torch.tensor([[0, 1, 2], [1, 0, 3]])


def mesh(name):
    """(verts (V,3) float32, faces (F,3) int64) of a named mesh on the host, computed once and shared; never modified."""
    if name not in _MESH:
        if name.startswith("jgrid"):                                              # jgrid<n>_<seed>
            n, seed = (int(x) for x in name[5:].split("_"))
            verts, faces = jittered_grid(n, seed)
        elif name == "flat_bipyramid":
            verts, faces = flat_bipyramid()
        elif name == "kite":
            verts, faces = kite()
        elif name == "misoriented":                                               # one face of the sphere turned over
            verts, faces = collapse_mesh("sphere9")
            faces = faces.clone()
            faces[17] = faces[17][[0, 2, 1]]
        elif name == "open_sphere":                                               # a hole with a ragged rim
            verts, faces = collapse_mesh("sphere17")
            faces = faces[:-60]
        elif name == "f10":
            from test_mesh_contains import f10
            verts, faces = f10()[:2]
            verts, faces = verts.to(torch.float32), faces.long()
        else:
            verts, faces = collapse_mesh(name)
        _MESH[name] = (verts.contiguous(), faces.contiguous())
    return _MESH[name]


def spec(name, criterion="delaunay", salt=0):
    """meshing.mesh_flip_round of a case on the host with its details, computed once and shared; never modified."""
    from arah_release_amd import meshing
    key = (name, criterion, salt)
    if key not in _SPEC:
        _SPEC[key] = meshing.mesh_flip_round(*mesh(name), criterion, salt, details=True)
    return _SPEC[key]


def counts_of(out):
    return dict(zip(NAMES, out[2].tolist()))


# ---- an independent restatement ---------------------------------------------------------------------------------------------------
def hash32(x):
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xffffffff
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xffffffff
    return x ^ (x >> 16)


def cross(p0, p1, p2):
    e1, e2 = p1 - p0, p2 - p0
    return [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]


def dot(x, y):
    return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]


def wants(s, t, x, y, Nx, Ny):
    """The Delaunay test of the edge {s, t} with the opposite corners x, y, whose faces have the cross products Nx, Ny."""
    dx, dy = dot(s - x, t - x), dot(s - y, t - y)
    cx, cy = dot(Nx, Nx), dot(Ny, Ny)
    if dx < 0 and dy < 0:
        return True
    if dx < 0 and dy >= 0:
        return bool((dx * dx) * cy > (dy * dy) * cx)
    if dy < 0 and dx >= 0:
        return bool((dy * dy) * cx > (dx * dx) * cy)
    return False


def adjacency_np(faces, V):
    """valid, vf (ascending faces of every vertex), out_n / in_n (directed counts), nbr (ascending), start of the entries."""
    F = faces.shape[0]
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
                vf[i].append(f)
    nbr = [sorted(set(out_n[x]) | set(in_n[x])) for x in range(V)]
    start = np.concatenate([[0], np.cumsum([len(n) for n in nbr])]).astype(np.int64)
    return valid, vf, out_n, in_n, nbr, start


def numpy_round(verts, faces, criterion, salt):
    """The rule once more with python loops and numpy float64 scalars.  -> faces_out, face_flag, counts, edge_key, edge_reason,
    selected, as arrays, and the quadruple (u, v, a, b) of every candidate by its entry."""
    v32 = np.asarray(verts, np.float32)
    v64, faces = v32.astype(np.float64), np.asarray(faces, np.int64)
    V, F = v64.shape[0], faces.shape[0]
    valid, vf, out_n, in_n, nbr, start = adjacency_np(faces, V)
    rim = [any(out_n[x].get(n, 0) + in_n[x].get(n, 0) == 1 for n in nbr[x]) for x in range(V)]
    edge_key = np.full(6 * F, -1, np.int64)
    edge_reason = np.full(6 * F, 255, np.uint8)
    quads, keys, n_edges = {}, {}, 0
    mix = (salt * 0x9e3779b9) & 0xffffffff
    with np.errstate(all="ignore"):
        for u in range(V):
            for k, v in enumerate(nbr[u]):
                if v <= u:
                    continue
                i = int(start[u]) + k
                n_edges += 1
                if out_n[u].get(v, 0) != 1 or in_n[u].get(v, 0) != 1:
                    edge_reason[i] = 1
                    continue
                fa = fb = None
                for f in vf[u]:
                    ids = [int(x) for x in faces[f]]
                    if v in ids:
                        if ids[(ids.index(u) + 1) % 3] == v:
                            fa, a = f, sum(ids) - u - v
                        else:
                            fb, b = f, sum(ids) - u - v
                assert fa is not None and fb is not None
                if a == b:
                    edge_reason[i] = 2
                    continue
                if b in nbr[a]:
                    edge_reason[i] = 3
                    continue
                if not all(np.isfinite(v32[x]).all() for x in (u, v, a, b)):
                    edge_reason[i] = 4
                    continue
                pu, pv, pa, pb = v64[u], v64[v], v64[a], v64[b]
                Na, Nb = cross(pa, pu, pv), cross(pb, pv, pu)
                N1, N2 = cross(pa, pu, pb), cross(pb, pv, pa)
                if criterion == "delaunay":
                    asks = wants(pu, pv, pa, pb, Na, Nb) and not wants(pa, pb, pu, pv, N1, N2)
                else:
                    before = sum(abs(len(nbr[x]) - (4 if rim[x] else 6)) for x in (u, v, a, b))
                    after = sum(abs(len(nbr[x]) + s - (4 if rim[x] else 6)) for x, s in ((u, -1), (v, -1), (a, 1), (b, 1)))
                    asks = after < before
                if not asks:
                    edge_reason[i] = 5
                    continue
                if not all(dot(N, M) > 0 for N in (N1, N2) for M in (Na, Nb)):
                    edge_reason[i] = 6
                    continue
                edge_reason[i] = 0
                keys[i] = (hash32(i ^ mix) << 32) | i
                edge_key[i] = keys[i] - (1 << 64) if keys[i] >= 1 << 63 else keys[i]
                quads[i] = (u, v, a, b, fa, fb)
    lock = {}
    for i, q in quads.items():
        for x in q[:4]:
            lock[x] = min(lock.get(x, 1 << 64), keys[i])
    faces_out = np.where((faces >= 0) & (faces < 2 ** 31), faces, -1).astype(np.int32)
    face_flag, selected = np.zeros(F, np.uint8), np.zeros(6 * F, bool)
    for i, (u, v, a, b, fa, fb) in quads.items():
        if all(lock[x] == keys[i] for x in (u, v, a, b)):
            selected[i] = True
            faces_out[fa], faces_out[fb] = (a, u, b), (b, v, a)
            face_flag[fa] = face_flag[fb] = 1
    counts = np.array([n_edges, len(quads), int(selected.sum())] + [int((edge_reason == r).sum()) for r in range(1, 7)], np.int32)
    return (faces_out, face_flag, counts, edge_key, edge_reason, selected), quads


def same_bits(got, want, what, n=None):
    """The first n outputs (all of `want` by default) equal bit for bit."""
    keys = ("faces", "face_flag", "counts", "edge_key", "edge_reason", "selected")
    for key, g, w in list(zip(keys, got, want))[:n]:
        g, w = np.asarray(g.cpu() if torch.is_tensor(g) else g), np.asarray(w.cpu() if torch.is_tensor(w) else w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, key, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (what, key)


def deviation(verts, faces):
    """The sum over the vertices of |valence - target|, target 4 on a boundary and 6 elsewhere."""
    from arah_release_amd import geometry
    adj = geometry.mesh_adjacency(verts, faces)
    deg = (adj.nbr_start[1:] - adj.nbr_start[:-1]).long()
    target = torch.where((adj.vert_flags & 1) != 0, 4, 6)
    return int((deg - target).abs().sum())


# ---- 1: the specification is the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere9", "jgrid9_0", "bad_ids", "nan_vertex", "three_faces", "misoriented", "bicone40", "sheet",
                                  "open_sphere", "flat_bipyramid", "kite"])
def test_specification_is_the_restatement(name):
    verts, faces = mesh(name)
    for criterion, salt in (("delaunay", 0), ("valence", 0), ("delaunay", 7), ("valence", 2 ** 32 - 1)):
        got, (want, _) = spec(name, criterion, salt), numpy_round(verts.numpy(), faces.numpy(), criterion, salt)
        same_bits(got, want, (name, criterion, salt))
        c = counts_of(got)
        assert c["candidates"] == int((got[4] == 0).sum()) and c["edges"] == int((got[4] != 255).sum()) == sum(c[k] for k in NAMES[3:]) + c["candidates"]
        assert int(got[1].sum()) == 2 * c["selected"] and (c["selected"] > 0) == (c["candidates"] > 0)


def test_salt_changes_the_order_not_the_candidates():
    a, b = spec("sphere9", "valence", 0), spec("sphere9", "valence", 1)
    assert torch.equal(a[4], b[4]) and counts_of(a)["candidates"] == counts_of(b)["candidates"] > 8
    assert not torch.equal(a[3], b[3]) and not torch.equal(a[5], b[5])
    assert torch.equal(a[3] & 0xffffffff, b[3] & 0xffffffff)                      # the lower half is the entry


# ---- 2: cases with a known answer -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("criterion", CRITERIA)
def test_tetrahedron_has_no_candidate(criterion):
    out = spec("tetrahedron", criterion)
    c = counts_of(out)
    assert c["edges"] == c["exists"] == 6 and c["candidates"] == c["selected"] == 0
    assert torch.equal(out[0].long(), mesh("tetrahedron")[1]) and not out[1].any()


def test_flat_bipyramid_flips_one_of_three():
    from arah_release_amd import geometry
    verts, faces = mesh("flat_bipyramid")
    out = spec("flat_bipyramid")
    c = counts_of(out)
    assert c["edges"] == 9 and c["candidates"] == 3 and c["selected"] == 1 and c["exists"] == 6   # the apex edges' flips exist
    new = out[0].long()
    assert int(out[1].sum()) == 2 and int(((new == 3).any(1) & (new == 4).any(1)).sum()) == 2       # the edge {3, 4}
    topo = geometry.mesh_topology(verts, new)
    assert topo["watertight"] and topo["manifold"] and topo["euler"] == 2
    res = geometry.flip_edges(verts, faces)
    assert res["converged"] and res["flips"] == 1 and res["rounds"] == 2 and torch.equal(res["faces"], new)


@pytest.mark.parametrize("criterion", CRITERIA)
def test_rims_fins_turned_faces_and_bad_vertices_never_flip(criterion):
    from arah_release_amd import geometry
    for name in ("sheet", "three_faces", "misoriented", "nan_vertex"):
        verts, faces = mesh(name)
        adj = geometry.mesh_adjacency(verts, faces)
        E = int(adj.nbr_start[-1])
        owner = torch.repeat_interleave(torch.arange(verts.shape[0]), (adj.nbr_start[1:] - adj.nbr_start[:-1]).long())
        nbr = adj.nbr[:E].long()
        out = spec(name, criterion)
        reason = out[4][:E]
        edge = nbr > owner
        odd = (adj.nbr_out[:E] != 1) | (adj.nbr_in[:E] != 1)
        assert bool((reason[edge & odd] == 1).all()) and bool((reason[edge & ~odd] != 1).all())
        assert (int((edge & odd).sum()) > 0) == (name != "nan_vertex")
        bad = ~torch.isfinite(verts).all(1)
        at_bad = edge & (bad[owner] | bad[nbr])
        assert not bool((reason[at_bad] == 0).any()) and (name != "nan_vertex" or int((reason[at_bad] == 4).sum()) > 0)
        regular = name == "sheet" and criterion == "valence"                     # a regular grid: every valence is on target
        assert (counts_of(out)["selected"] > 0) != regular and not bool(out[5][:E][edge & odd].any())
        # a face at a non-finite vertex is never rewritten
        assert not bool(out[1][bad[faces].any(1)].any())


@pytest.mark.parametrize("criterion", CRITERIA)
def test_interior_edge_between_boundary_vertices_may_flip(criterion):
    out = spec("kite", criterion)
    c = counts_of(out)
    assert c["edges"] == 5 and c["not_interior"] == 4
    if criterion == "delaunay":
        assert c["selected"] == 1 and out[0].tolist() == [[2, 0, 3], [3, 1, 2]] and out[1].tolist() == [1, 1]
    else:                                                                         # valences 3, 3, 2, 2 against the target 4
        assert c["criterion"] == 1 and c["selected"] == 0 and torch.equal(out[0].long(), mesh("kite")[1])


# ---- 3: Delaunay against an independent answer ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,seed", [(5, 3), (9, 0), (33, 1)])
def test_jittered_grid_reaches_the_delaunay_triangulation(n, seed):
    from arah_release_amd import geometry
    verts, faces = mesh("jgrid%d_%d" % (n, seed))
    res = geometry.flip_edges(verts, faces, "delaunay", max_rounds=64)
    print("jittered %d x %d grid, seed %d: %d flips in %d rounds" % (n, n, seed, res["flips"], res["rounds"]))
    assert res["converged"] and res["rounds"] <= 64 and res["flips"] > 0 and res["candidates"][-1] == 0
    assert res["faces"].shape == faces.shape and res["faces"].dtype == faces.dtype
    p = verts.double()[res["faces"]]
    z = ((p[:, 1, 0] - p[:, 0, 0]) * (p[:, 2, 1] - p[:, 0, 1]) - (p[:, 1, 1] - p[:, 0, 1]) * (p[:, 2, 0] - p[:, 0, 0]))
    assert bool((z > 0).all()) or bool((z < 0).all())                             # no face turned over
    spatial = pytest.importorskip("scipy.spatial")
    want = {tuple(sorted(int(i) for i in t)) for t in spatial.Delaunay(verts[:, :2].double().numpy()).simplices}
    got = {tuple(sorted(int(i) for i in t)) for t in res["faces"]}
    assert len(got) == faces.shape[0] and got == want, len(got ^ want)


# ---- 4: valence ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere17", "open_sphere"])
def test_valence_rounds_lower_the_deviation_by_their_gains(name):
    from arah_release_amd import meshing
    verts, faces = mesh(name)
    total, rounds = deviation(verts, faces), 0
    first = total
    while True:
        out = meshing.mesh_flip_round(verts, faces, "valence", rounds, details=True)
        c = counts_of(out)
        if c["candidates"] == 0:
            break
        _, quads = numpy_round(verts.numpy(), faces.numpy(), "valence", rounds)
        _, _, _, _, nbr, _ = adjacency_np(faces.numpy(), verts.shape[0])
        rim = ((torch.as_tensor(meshing.mesh_adjacency(faces, verts.shape[0])[6]) & 1) != 0).tolist()
        gain = 0
        for i in torch.nonzero(out[5])[:, 0].tolist():
            u, v, a, b = quads[i][:4]
            off = [len(nbr[x]) - (4 if rim[x] else 6) for x in (u, v, a, b)]
            g = sum(abs(o) for o in off) - sum(abs(o + s) for o, s in zip(off, (-1, -1, 1, 1)))
            assert g > 0
            gain += g
        faces = out[0].long()
        now = deviation(verts, faces)
        assert c["selected"] > 0 and now == total - gain
        total, rounds = now, rounds + 1
        assert rounds < 64
    print("%s: sum |valence - target| %d -> %d in %d rounds" % (name, first, total, rounds))
    assert total < first


# ---- 5: topology ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("criterion", CRITERIA)
def test_closed_surface_stays_closed(criterion):
    from arah_release_amd import geometry
    verts, faces = mesh("sphere33")
    res = geometry.flip_edges(verts, faces, criterion)
    topo = geometry.mesh_topology(verts, res["faces"])
    assert res["converged"] and res["flips"] > 100 and res["faces"].shape == faces.shape
    assert topo["boundary_edges"] == topo["nonmanifold_edges"] == topo["misoriented_edges"] == 0 and topo["euler"] == 2
    assert topo["faces"] == faces.shape[0] and geometry.mesh_components(verts, res["faces"])["n_components"] == 1
    assert geometry.flip_edges(verts, res["faces"], criterion)["flips"] == 0        # a fixed point


# ---- 6: arguments -------------------------------------------------------------------------------------------------------------------
def test_argument_checks():
    from arah_release_amd import geometry, meshing
    verts, faces = mesh("octahedron")
    for bad in ({"criterion": "angle"}, {"criterion": 0}, {"salt": -1}, {"salt": 2 ** 32}, {"salt": 1.0}, {"salt": True}):
        with pytest.raises(ValueError):
            meshing.mesh_flip_round(verts, faces, **bad)
    with pytest.raises(ValueError):
        meshing.mesh_flip_round(verts.double(), faces)
    for bad in ({"criterion": "angle"}, {"max_rounds": -1}, {"max_rounds": 2.0}, {"max_rounds": True}):
        with pytest.raises(ValueError):
            geometry.flip_edges(verts, faces, **bad)
    none = geometry.flip_edges(verts, faces, max_rounds=0)
    assert none["rounds"] == 0 and not none["converged"] and torch.equal(none["faces"], faces)
    empty = meshing.mesh_flip_round(verts[:0], faces[:0])
    assert empty[0].shape == (0, 3) and empty[1].shape == (0,) and empty[2].tolist() == [0] * 9
    lone = meshing.mesh_flip_round(verts, faces[:0], details=True)
    assert lone[2].tolist() == [0] * 9 and lone[3].shape == (0,)
    gone = meshing.mesh_flip_round(verts[:0], faces, details=True)                # faces without a vertex stay as they are
    assert gone[2].tolist() == [0] * 9 and torch.equal(gone[0].long(), faces) and bool((gone[4] == 255).all())


def test_abi_is_declared_and_checks_its_arguments():
    import ctypes as C
    from arah_release_amd import hip
    with open(os.path.join(REPO, "include", "arah_hip.h")) as fh:
        declared = set(re.findall(r"\b(arah_\w+)\s*\(", fh.read()))
    lib = hip.load_library()
    for name in NEW_EXPORTS:
        assert name in declared and name in hip.EXPORTS and hasattr(lib, name), name
    assert len(hip.EXPORTS) == len(set(hip.EXPORTS))
    size = lib.arah_mesh_flip_round_scratch_bytes
    assert size(10, 10) > 0 and size(0, 0) > 0 and size(10, 10) % 256 == 0
    assert size(10, 10) > lib.arah_mesh_adjacency_scratch_bytes(10, 10)          # the adjacency is built inside
    for sizes in ((-1, 0), (0, -1), (2 ** 31, 0), (0, 2 ** 28 + 1)):
        assert size(*sizes) == 0
    p = C.c_void_p(256)                                                           # never dereferenced: every call is refused

    def call(V=4, F=4, criterion=0, counts=p, scratch=p, verts=p, faces=p, out=p, nbytes=1 << 30):
        return lib.arah_mesh_flip_round(verts, C.c_int64(V), faces, C.c_int64(F), C.c_int32(criterion), C.c_uint32(3), out, out, counts,
                                        out, out, scratch, C.c_size_t(nbytes), None)
    for bad in ({"V": -1}, {"F": -1}, {"F": 2 ** 28 + 1}, {"criterion": 2}, {"criterion": -1}, {"counts": None}, {"scratch": None},
                {"verts": None}, {"faces": None}, {"out": None}):
        assert call(**bad) == -1, bad                                             # ARAH_E_BADARG, nothing launched
    assert call(nbytes=16) == -3                                                  # ARAH_E_WORKSPACE
