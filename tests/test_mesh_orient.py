"""Orientation, boundary loops and hole filling of indexed meshes on the host: the tensor specifications meshing.mesh_orient /
mesh_boundary_loops / mesh_fill_holes and geometry.orient_mesh / boundary_loops / fill_holes / repair_mesh.  (The kernels of
csrc/meshorient.hpp against the specification: tests/test_mesh_orient_gpu.py, which shares the meshes built here.)

Every decision is an integer's and the one float result goes through one exact rule, so every result is unique.  The
specification is held to a restatement written with python loops, dicts, a breadth-first search and python ints, and to known
answers on hand-made meshes and on level sets with 30 % of their faces reversed."""
import collections
import os
import re

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POLICIES = ("seed", "majority", "negative", "positive")
ORIENT_NAMES = ("flip", "face_comp", "faces_out", "comp_faces", "comp_flags", "comp_vol_hi", "comp_vol_lo", "counts")
LOOP_NAMES = ("edges", "edge_face", "edge_loop", "loop_edges", "loop_simple", "loop_vert", "counts")
FILL_NAMES = ("verts_out", "vert_src", "faces_out", "face_loop", "counts")
NEW_EXPORTS = ("arah_mesh_orient_scratch_bytes", "arah_mesh_orient", "arah_mesh_boundary_loops_scratch_bytes",
               "arah_mesh_boundary_loops", "arah_mesh_fill_holes_scratch_bytes", "arah_mesh_fill_holes")


# ---- fields on the lattice of [-1,1]^3 (those of tests/test_mesh_adjacency.py, restated) ----------------------------------------
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


FIELDS = {"sphere17": lambda: sphere(17), "torus33": lambda: torus(33), "blobs33": lambda: two_blobs(33), "noise20": noise,
          "sphere33": lambda: sphere(33), "clipped17": lambda: sphere(17, 1.2)}    # the last leaves the lattice through six sides
FAN = 4096
HOLE_STARS = (10, 500, 900)


def _random_verts(n, seed):
    return torch.randn(n, 3, generator=torch.Generator().manual_seed(seed))


def _reverse_some(faces, seed=3, share=0.3):
    """The faces with the rows where torch.rand(F) < share reversed, and the mask of those rows."""
    pick = torch.rand(faces.shape[0], generator=torch.Generator().manual_seed(seed)) < share
    return torch.where(pick[:, None], faces[:, [0, 2, 1]], faces), pick


def _without_stars(faces, stars):
    keep = torch.ones(faces.shape[0], dtype=torch.bool)
    for v in stars:
        keep &= (faces != v).all(1)
    return faces[keep]


CUBE_QUADS = ((0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5))   # outward, vertex id = x + 2 y + 4 z


def _cube():
    verts = torch.tensor([[i & 1, (i >> 1) & 1, (i >> 2) & 1] for i in range(8)], dtype=torch.float32) * 0.9 - 0.31
    faces = [t for a, b, c, d in CUBE_QUADS for t in ((a, b, c), (a, c, d))]
    return verts, torch.tensor(faces, dtype=torch.int64)


def _touching_stars(faces, n_verts):
    """Two vertices that are not adjacent and whose rims share exactly one vertex: removing both stars leaves two holes that
    touch there.  The first such pair in ascending order, found with python sets."""
    ring = collections.defaultdict(set)
    for a, b, c in faces.tolist():
        ring[a] |= {b, c}
        ring[b] |= {a, c}
        ring[c] |= {a, b}
    for u in range(100, n_verts):
        for m in sorted(ring[u]):
            for w in sorted(ring[m]):
                if w > u and w not in ring[u] and len(ring[u] & ring[w]) == 1:
                    return u, w
    raise AssertionError("no such pair")


def _stars_of_valence(faces, wanted):
    """One vertex of each wanted valence (the last: at least that many neighbours), the lowest ids whose closed stars are disjoint."""
    ring = collections.defaultdict(set)
    for a, b, c in faces.tolist():
        ring[a] |= {b, c}
        ring[b] |= {a, c}
        ring[c] |= {a, b}
    picked, taken = [], set()
    for k, n in enumerate(wanted):
        for v in sorted(ring):
            fits = len(ring[v]) >= n if k == len(wanted) - 1 else len(ring[v]) == n
            if fits and not (ring[v] | {v}) & taken:
                picked.append(v)
                taken |= ring[v] | {v}
                break
    assert len(picked) == len(wanted)
    return picked


def _hand(name):
    """The hand-made meshes: -> (verts (V,3) float32, faces (F,3) int64)."""
    t = lambda rows: torch.tensor(rows, dtype=torch.int64).reshape(-1, 3)
    if name == "empty":
        return torch.zeros(0, 3), t([])
    if name == "no_faces":
        return _random_verts(5, 1), t([])
    if name == "one_tri":
        return _random_verts(3, 2), t([[0, 1, 2]])
    if name == "pair_opposite":
        return _random_verts(4, 3), t([[0, 1, 2], [1, 0, 3]])
    if name == "pair_same":
        return _random_verts(4, 4), t([[0, 1, 2], [0, 1, 3]])
    if name == "three_on_edge":
        return _random_verts(5, 5), t([[0, 1, 2], [1, 0, 3], [0, 1, 4]])
    if name == "same_face_twice":
        return _random_verts(4, 8), t([[0, 1, 2], [0, 1, 2], [2, 1, 3]])
    if name == "bad_faces":                                                       # out of range, negative, repeated (twice): four skipped
        return _random_verts(6, 6), t([[0, 1, 2], [0, 1, 6], [2, -1, 3], [4, 4, 5], [3, 1, 2], [5, 3, 5]])
    if name == "nonfinite":                                                       # a NaN corner: no volume from its three faces
        verts, faces = _cube()
        verts = verts.clone()
        verts[7, 1] = float("nan")
        return verts, _reverse_some(faces, seed=5)[0]
    if name == "moebius16":                                                       # 8 columns of (top i, bottom i + 8), closed with a twist
        top = lambda i: i if i < 8 else 8
        bot = lambda i: i + 8 if i < 8 else 0
        rows = [r for i in range(8) for r in ((top(i), bot(i), top(i + 1)), (bot(i), bot(i + 1), top(i + 1)))]
        return _random_verts(16, 12), t(rows)
    if name == "two_tets":                                                        # they share vertex 0 and no edge
        tet = lambda a, b, c, d: [(a, c, b), (a, b, d), (b, c, d), (a, d, c)]
        return _random_verts(7, 13), t(tet(0, 1, 2, 3) + tet(0, 4, 5, 6))
    if name == "cube_pair":                                                       # the two triangles of the side +y reversed
        verts, faces = _cube()
        faces = faces.clone()
        faces[6:8] = faces[6:8][:, [0, 2, 1]]
        return verts, faces
    if name == "fan4096_r":                                                       # apex 0, rim 1 .. 4097, rows shuffled, 30 % reversed
        i = torch.arange(1, FAN + 1)
        faces = torch.stack([torch.zeros_like(i), i, i + 1], 1)
        faces = faces[torch.randperm(FAN, generator=torch.Generator().manual_seed(10))]
        return _random_verts(FAN + 2, 9), _reverse_some(faces)[0]
    raise KeyError(name)


HAND = ("empty", "no_faces", "one_tri", "pair_opposite", "pair_same", "three_on_edge", "same_face_twice", "bad_faces", "nonfinite",
        "moebius16", "two_tets", "cube_pair", "fan4096_r")
REVERSED = ("sphere17_r", "torus33_r", "blobs33_r", "noise20_r")
HOLED = ("sphere33_h", "sphere33_hr", "sphere33_sizes", "sphere33_touch", "clipped17")
ALL_MESHES = HAND + REVERSED + HOLED
_MESH, _RESTATED = {}, {}


def mesh(name):
    """(verts (V,3) float32, faces (F,3) int64) of a named mesh on the host, computed once and shared; never modified."""
    from arah_release_amd import meshing
    if name not in _MESH:
        if name in FIELDS:
            verts, faces, _ = meshing.marching_cubes_indexed(FIELDS[name]())
        elif name in REVERSED:
            verts, faces = mesh(name[:-2])
            faces = _reverse_some(faces)[0]
        elif name == "sphere33_h":
            verts, faces = mesh("sphere33")
            faces = _without_stars(faces, HOLE_STARS)
        elif name == "sphere33_hr":                                               # 30 % reversed, then the three holes
            verts, faces = mesh("sphere33")
            faces = _without_stars(_reverse_some(faces)[0], HOLE_STARS)
        elif name == "sphere33_sizes":
            verts, faces = mesh("sphere33")
            faces = _without_stars(faces, _stars_of_valence(faces, (4, 5, 7)))
        elif name == "sphere33_touch":
            verts, faces = mesh("sphere33")
            faces = _without_stars(faces, _touching_stars(faces, verts.shape[0]))
        else:
            verts, faces = _hand(name)
        _MESH[name] = (verts.contiguous(), faces.long().contiguous())
    return _MESH[name]


# ---- the restatement: python loops, dicts, a breadth-first search, python ints --------------------------------------------------
def _valid_faces(faces, V):
    rows = faces.tolist()
    return rows, [all(0 <= i < V for i in r) and len(set(r)) == 3 for r in rows]


def _edge_dict(rows, ok):
    """undirected edge -> [(face, traverses it from its lower to its higher end)] in ascending (face, corner) order"""
    on = collections.defaultdict(list)
    for f, r in enumerate(rows):
        if ok[f]:
            for c in range(3):
                a, b = r[c], r[(c + 1) % 3]
                on[(min(a, b), max(a, b))].append((f, a < b))
    return on


def _quantise(x, origin, scale, limit):
    return int(round(min(max((float(x) - float(origin)) * scale, -limit), limit)))   # round(): half to even, like llrint


def restate_orient(verts, faces, policy, quant):
    """-> dict of python lists: labels, b, flags, vol (python ints, one per component), hi, lo, flip, counts"""
    V = verts.shape[0]
    rows, ok = _valid_faces(faces, V)
    F = len(rows)
    pairs = collections.defaultdict(list)
    for members in _edge_dict(rows, ok).values():
        if len(members) == 2:
            (f, df), (g, dg) = members
            pairs[f].append((g, int(df == dg)))
            pairs[g].append((f, int(df == dg)))
    label, b, nonor = [-1] * F, [0] * F, []
    for seed in range(F):
        if not ok[seed] or label[seed] >= 0:
            continue
        c, twisted = len(nonor), False
        label[seed] = c
        queue = collections.deque([seed])
        while queue:
            f = queue.popleft()
            for g, s in pairs[f]:
                if label[g] < 0:
                    label[g], b[g] = c, b[f] ^ s
                    queue.append(g)
                elif b[g] != b[f] ^ s:
                    twisted = True
        nonor.append(twisted)
    C = len(nonor)
    for f in range(F):
        if label[f] >= 0 and nonor[label[f]]:
            b[f] = 0
    size, ones = [0] * C, [0] * C
    for f in range(F):
        if label[f] >= 0:
            size[label[f]] += 1
            ones[label[f]] += b[f]
    vol, hi, lo = [0] * C, [0] * C, [0] * C
    if policy in ("negative", "positive"):
        origin, scale = quant
        pts = verts.tolist()
        for f in range(F):
            p = [pts[i] for i in rows[f]] if label[f] >= 0 else None
            if p is None or not all(np.isfinite(x) for corner in p for x in corner):
                continue
            q = [[_quantise(x, o, scale, 2.0 ** 18) for x, o in zip(corner, origin)] for corner in p]
            d = (q[0][0] * (q[1][1] * q[2][2] - q[1][2] * q[2][1]) - q[0][1] * (q[1][0] * q[2][2] - q[1][2] * q[2][0])
                 + q[0][2] * (q[1][0] * q[2][1] - q[1][1] * q[2][0]))
            d = -d if b[f] else d
            vol[label[f]] += d
            hi[label[f]] += d >> 32
            lo[label[f]] += d & 0xFFFFFFFF
    rev = []
    for c in range(C):
        majority = ones[c] > size[c] - ones[c]
        if policy == "seed":
            r = False
        elif policy == "majority" or vol[c] == 0:
            r = majority
        else:
            r = vol[c] > 0 if policy == "negative" else vol[c] < 0
        rev.append(r and not nonor[c])
    flip = [int(label[f] >= 0 and not nonor[label[f]] and bool(b[f]) != rev[label[f]]) for f in range(F)]
    counts = [sum(ok), C, sum(nonor), sum(b), sum(rev), sum(flip)]
    return {"labels": label, "b": b, "flags": [int(n) | int(r) << 1 for n, r in zip(nonor, rev)], "vol": vol, "hi": hi, "lo": lo,
            "size": size, "flip": flip, "counts": counts}


def restate_loops(faces, V):
    """-> dict of python lists: edges, edge_face, edge_loop, loop_edges, loop_simple, loop_vert"""
    rows, ok = _valid_faces(faces, V)
    on = _edge_dict(rows, ok)
    edges, edge_face = [], []
    for f, r in enumerate(rows):
        if ok[f]:
            for c in range(3):
                a, b = r[c], r[(c + 1) % 3]
                if len(on[(min(a, b), max(a, b))]) == 1:
                    edges.append((a, b))
                    edge_face.append(f)
    touch, out, inn = collections.defaultdict(set), collections.Counter(), collections.Counter()
    for a, b in edges:
        touch[a].add(b)
        touch[b].add(a)
        out[a] += 1
        inn[b] += 1
    loop_of, loop_vert, loop_simple = {}, [], []
    for seed in sorted(touch):
        if seed in loop_of:
            continue
        l = len(loop_vert)
        loop_vert.append(seed)
        loop_of[seed] = l
        queue, simple = collections.deque([seed]), True
        while queue:
            v = queue.popleft()
            simple = simple and out[v] == 1 and inn[v] == 1
            for n in touch[v]:
                if n not in loop_of:
                    loop_of[n] = l
                    queue.append(n)
        loop_simple.append(int(simple))
    edge_loop = [loop_of[a] for a, _ in edges]
    loop_edges = [edge_loop.count(l) for l in range(len(loop_vert))]
    return {"edges": edges, "edge_face": edge_face, "edge_loop": edge_loop, "loop_edges": loop_edges, "loop_simple": loop_simple,
            "loop_vert": loop_vert}


def restate_fill(verts, faces, max_edges, quant):
    """-> (new vertices as float32 rows, their sources, new faces, their loops)"""
    origin, scale = quant
    V, pts = verts.shape[0], verts.tolist()
    r = restate_loops(faces, V)
    new_v, src, rank = [], [], {}
    for l, (n, simple, low) in enumerate(zip(r["loop_edges"], r["loop_simple"], r["loop_vert"])):
        members = [a for (a, _), el in zip(r["edges"], r["edge_loop"]) if el == l]
        if not simple or not 3 <= n <= max_edges or not all(np.isfinite(x) for a in members for x in pts[a]):
            continue
        rank[l] = len(new_v)
        S = [sum(_quantise(pts[a][k], origin[k], scale, 2.0 ** 36) for a in members) for k in range(3)]
        new_v.append([np.float32(float(origin[k]) + (float(S[k]) / float(n)) / scale) for k in range(3)])
        src.append(low)
    new_f = [(b, a, V + rank[l]) for (a, b), l in zip(r["edges"], r["edge_loop"]) if l in rank]
    return new_v, src, new_f, [l for l in r["edge_loop"] if l in rank]


# ---- shared results -------------------------------------------------------------------------------------------------------------
def quant_of(name):
    from arah_release_amd import meshing
    key = ("quant", name)
    if key not in _RESTATED:
        verts, _ = mesh(name)
        _RESTATED[key] = (meshing.orient_quant(verts), meshing.fill_quant(verts))
    return _RESTATED[key]


def spec_orient(name, policy):
    """meshing.mesh_orient of a named mesh on the host, computed once and shared; never modified."""
    from arah_release_amd import meshing
    key = ("orient", name, policy)
    if key not in _RESTATED:
        verts, faces = mesh(name)
        _RESTATED[key] = meshing.mesh_orient(verts, faces, policy=policy)
    return _RESTATED[key]


def spec_loops(name):
    from arah_release_amd import meshing
    key = ("loops", name)
    if key not in _RESTATED:
        verts, faces = mesh(name)
        _RESTATED[key] = meshing.mesh_boundary_loops(faces, verts.shape[0])
    return _RESTATED[key]


def spec_fill(name, max_edges=64):
    from arah_release_amd import meshing
    key = ("fill", name, max_edges)
    if key not in _RESTATED:
        verts, faces = mesh(name)
        _RESTATED[key] = meshing.mesh_fill_holes(verts, faces, max_edges=max_edges)
    return _RESTATED[key]


def topology(verts, faces):
    from arah_release_amd import geometry
    return geometry.mesh_topology(verts, faces)


# ---- the specification against the restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_MESHES)
def test_orient_is_the_restatement(name):
    verts, faces = mesh(name)
    F = faces.shape[0]
    for policy in POLICIES:
        flip, face_comp, faces_out, comp_faces, comp_flags, vol_hi, vol_lo, counts = spec_orient(name, policy)
        r = restate_orient(verts, faces, policy, quant_of(name)[0])
        C = r["counts"][1]
        assert counts.tolist() == r["counts"], (name, policy)
        assert face_comp.tolist() == r["labels"] and flip.tolist() == r["flip"], (name, policy)
        assert comp_faces.tolist() == r["size"] + [0] * (F - C) and comp_flags.tolist() == r["flags"] + [0] * (F - C)
        assert vol_hi.tolist() == r["hi"] + [0] * (F - C) and vol_lo.tolist() == r["lo"] + [0] * (F - C)
        assert [(h << 32) + l for h, l in zip(vol_hi.tolist(), vol_lo.tolist())][:C] == r["vol"]
        expect = [[a, c, b] if fl else [a, b, c] for (a, b, c), fl in zip(faces.tolist(), r["flip"])]
        assert faces_out.tolist() == expect
        assert (flip.dtype, face_comp.dtype, faces_out.dtype, vol_hi.dtype, counts.dtype) == (
            torch.uint8, torch.int32, torch.int32, torch.int64, torch.int32)
        # b, seen through "seed": the flips of that policy are b itself
        if policy == "seed":
            assert flip.tolist() == [int(x) for x in r["b"]]


@pytest.mark.parametrize("name", ALL_MESHES)
def test_loops_and_fill_are_the_restatement(name):
    verts, faces = mesh(name)
    V, F = verts.shape[0], faces.shape[0]
    edges, edge_face, edge_loop, loop_edges, loop_simple, loop_vert, counts = spec_loops(name)
    r = restate_loops(faces, V)
    B, L = len(r["edges"]), len(r["loop_vert"])
    assert counts.tolist() == [B, L, sum(r["loop_simple"])]
    assert edges.tolist() == [list(e) for e in r["edges"]] + [[0, 0]] * (3 * F - B)
    assert edge_face.tolist() == r["edge_face"] + [0] * (3 * F - B) and edge_loop.tolist() == r["edge_loop"] + [0] * (3 * F - B)
    assert loop_edges.tolist() == r["loop_edges"] + [0] * (V - L) and loop_simple.tolist() == r["loop_simple"] + [0] * (V - L)
    assert loop_vert.tolist() == r["loop_vert"] + [0] * (V - L)
    assert loop_simple.dtype == torch.uint8 and edges.dtype == torch.int32
    for max_edges in (64, 5):
        verts_out, vert_src, faces_out, face_loop, fcounts = spec_fill(name, max_edges)
        new_v, src, new_f, new_l = restate_fill(verts, faces, max_edges, quant_of(name)[1])
        Lf, Bf = len(new_v), len(new_f)
        assert fcounts.tolist() == [B, L, sum(r["loop_simple"]), Lf, Bf]
        assert tuple(verts_out.shape) == (V + V // 3, 3) and tuple(faces_out.shape) == (4 * F, 3)
        assert torch.equal(verts_out[:V].view(torch.int32), verts.view(torch.int32))   # bits: a NaN stays the NaN it was
        assert torch.equal(verts_out[V:V + Lf], torch.tensor(np.array(new_v, np.float32).reshape(-1, 3)))
        assert not verts_out[V + Lf:].any() and not vert_src[V + Lf:].any()
        assert vert_src[:V + Lf].tolist() == list(range(V)) + src
        assert faces_out[:F + Bf].tolist() == faces.tolist() + [list(t) for t in new_f] and not faces_out[F + Bf:].any()
        assert face_loop.tolist() == [-1] * F + new_l + [0] * (3 * F - Bf)


# ---- hand meshes with known answers ------------------------------------------------------------------------------------------------
def _public(name, policy, **kw):
    from arah_release_amd import geometry
    verts, faces = mesh(name)
    return geometry.orient_mesh(verts, faces, policy=policy, **kw)


def test_empty_meshes_and_one_triangle_are_defined():
    for name, n_faces in (("empty", 0), ("no_faces", 0), ("one_tri", 1)):
        for policy in POLICIES:
            res = _public(name, policy)
            assert res["n_components"] == n_faces and res["n_nonorientable"] == 0
            assert res["n_flipped"] == 0 or policy in ("negative", "positive")      # a lone triangle has a sign of its own
            assert tuple(res["faces"].shape) == (n_faces, 3) and tuple(res["component_faces"].shape) == (n_faces,)
        assert spec_loops(name)[6].tolist() == [3 * n_faces, n_faces, n_faces]
        assert spec_fill(name)[4].tolist() == [3 * n_faces, n_faces, n_faces, n_faces, 3 * n_faces]   # a triangle is a loop of 3


def test_pairs_across_one_edge():
    assert _public("pair_opposite", "seed")["flip"].tolist() == [0, 0]
    res = _public("pair_same", "seed")
    assert res["flip"].tolist() == [0, 1] and res["faces"].tolist() == [[0, 1, 2], [0, 3, 1]] and res["n_components"] == 1
    assert _public("pair_same", "majority")["flip"].tolist() == [0, 1]              # a tie goes to the seed


def test_three_faces_on_one_edge_are_three_components():
    for policy in ("seed", "majority"):
        res = _public("three_on_edge", policy)
        assert res["n_components"] == 3 and res["n_flipped"] == 0 and res["face_component"].tolist() == [0, 1, 2]


def test_the_same_face_twice():
    """The copies share their three edges: 1-2 carries three faces (no constraint), 0-1 and 2-0 carry the two copies in the same
    direction.  One component of the two, inconsistent with each other; the neighbour is on its own."""
    res = _public("same_face_twice", "seed")
    assert res["face_component"].tolist() == [0, 0, 1] and res["flip"].tolist() == [0, 1, 0]
    assert res["component_faces"].tolist() == [2, 1]


def test_invalid_faces_have_no_label_and_are_never_flipped():
    verts, faces = mesh("bad_faces")
    for policy in POLICIES:
        res = _public("bad_faces", policy)
        assert res["face_component"].tolist()[1:4] == [-1, -1, -1] and res["face_component"][5] == -1
        assert res["flip"][[1, 2, 3, 5]].tolist() == [0, 0, 0, 0]
        assert torch.equal(res["faces"][[1, 2, 3, 5]], faces[[1, 2, 3, 5]])         # copied as they came, bad ids included
        assert res["n_components"] == 1


def test_moebius_strip_is_one_nonorientable_component():
    for policy in POLICIES:
        res = _public("moebius16", policy)
        assert res["n_components"] == 1 and res["n_nonorientable"] == 1 and res["n_flipped"] == 0
        assert res["component_nonorientable"].tolist() == [True] and res["component_faces"].tolist() == [16]
        assert torch.equal(res["faces"], mesh("moebius16")[1])
    assert spec_orient("moebius16", "majority")[4][0] == 1
    t = topology(*mesh("moebius16"))
    assert t["boundary_edges"] == 16 and t["nonmanifold_edges"] == 0 and t["misoriented_edges"] >= 1   # the twist shows somewhere
    loops = spec_loops("moebius16")
    assert loops[6].tolist()[:2] == [16, 1]                                        # one boundary curve


def test_two_tetrahedra_sharing_a_vertex_are_two_components():
    res = _public("two_tets", "negative")
    assert res["n_components"] == 2 and res["component_faces"].tolist() == [4, 4] and res["n_nonorientable"] == 0
    assert topology(mesh("two_tets")[0], res["faces"])["misoriented_edges"] == 0


def _signed_volume(verts, faces):
    p = verts.double()[faces]
    return float((p[:, 0] * torch.linalg.cross(p[:, 1], p[:, 2])).sum()) / 6.0


def test_cube_with_a_reversed_pair_under_the_sign_policies():
    verts, faces = mesh("cube_pair")
    assert topology(*_cube())["watertight"] and _signed_volume(*_cube()) > 0        # the quads are listed outward
    neg, pos = _public("cube_pair", "negative"), _public("cube_pair", "positive")
    assert (neg["flip"] ^ pos["flip"]).tolist() == [1] * 12                         # mirror results
    assert torch.equal(pos["faces"], _cube()[1]) and torch.equal(neg["faces"], _cube()[1][:, [0, 2, 1]])
    assert _signed_volume(verts, neg["faces"]) < 0 < _signed_volume(verts, pos["faces"])
    assert torch.equal(_public("cube_pair", "majority")["faces"], _cube()[1])
    hi, lo = spec_orient("cube_pair", "positive")[5:7]
    assert (int(hi[0]) << 32) + int(lo[0]) > 0 and not hi[1:].any() and not lo[1:].any()


def test_fan_with_reversed_rows():
    verts, faces = mesh("fan4096_r")
    res = _public("fan4096_r", "majority")
    assert res["n_components"] == 1 and topology(verts, res["faces"])["misoriented_edges"] == 0
    original = torch.stack([faces[:, 0], faces[:, 1:].min(1).values, faces[:, 1:].max(1).values], 1)   # (0, i, i + 1)
    assert torch.equal(res["faces"], original)                                     # 70 % hold the original orientation


# ---- level sets with 30 % of their faces reversed ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name,misoriented,components", [("sphere17", 771, 1), ("blobs33", 1008, 2), ("torus33", 2359, 1)])
def test_reversed_level_sets_come_back_bit_for_bit(name, misoriented, components):
    """The misoriented edges BEFORE are a property of the input alone (mesh_topology, which this feature does not touch): 771,
    1008 and 2359.  The issue's table lists 770 and 2358 for the sphere and the torus; those cannot be: on a closed manifold every
    face has three neighbours, so the edges between the k reversed faces and the others number 3 k - 2 (edges inside the reversed
    set), of the parity of k, and the seeded draw reverses k = 367 and k = 1111 faces, both odd (482 for the blobs, even).  A
    restatement with a python dict counts 771 / 1008 / 2359 as well.  Everything the issue asks AFTER orienting is asserted as
    it states it: zero misoriented edges, the component counts, the original faces bit for bit."""
    from arah_release_amd import geometry, meshing
    verts, original = mesh(name)
    _, faces = mesh(name + "_r")
    assert topology(verts, faces)["misoriented_edges"] == misoriented > 0
    assert (misoriented - int(_reverse_some(original)[1].sum())) % 2 == 0           # the parity argument above
    assert meshing.winding_orient(verts, original)[0] == -1
    res = geometry.orient_mesh(verts, faces, policy="negative")
    assert torch.equal(res["faces"], original) and res["faces"].dtype == faces.dtype
    assert res["n_components"] == components and res["n_nonorientable"] == 0
    assert topology(verts, res["faces"])["misoriented_edges"] == 0
    assert torch.equal(res["flip"].bool(), _reverse_some(original)[1])
    assert torch.equal(geometry.orient_mesh(verts, faces)["faces"], original)       # "majority", the default, agrees
    assert torch.equal(geometry.orient_mesh(verts.shape[0], faces, policy="majority")["faces"], original)
    mirrored = geometry.orient_mesh(verts, faces, policy="positive")["faces"]
    assert torch.equal(mirrored, original[:, [0, 2, 1]])


def test_noise_field_has_no_misoriented_edge_inside_an_orientable_component():
    """Many small components: recovery is not asserted (a small component's majority can be the reversed side), consistency is."""
    from arah_release_amd import geometry
    verts, faces = mesh("noise20_r")
    for policy in POLICIES:
        res = geometry.orient_mesh(verts, faces, policy=policy)
        assert res["n_components"] > 10
        label = res["face_component"].long()
        keep = (label >= 0) & ~res["component_nonorientable"][label.clamp_min(0)]
        assert topology(verts, res["faces"][keep])["misoriented_edges"] == 0


# ---- holes ------------------------------------------------------------------------------------------------------------------------
def test_three_holes_are_filled_watertight():
    from arah_release_amd import geometry
    verts, faces = mesh("sphere33_h")
    V, F = verts.shape[0], faces.shape[0]
    loops = geometry.boundary_loops(verts, faces)
    assert loops["n_loops"] == 3 and loops["n_edges"] == 18 and loops["n_simple"] == 3 and loops["loop_simple"].all()
    assert tuple(loops["edges"].shape) == (18, 2) and int(loops["loop_edges"].sum()) == 18
    colour = torch.rand(V, 3, generator=torch.Generator().manual_seed(4))
    res = geometry.fill_holes(verts, faces, attributes={"colour": colour})
    assert res["filled"] == {"loops": 3, "faces": 18, "skipped_loops": 0}
    assert (res["n_verts"], res["n_tris"]) == (V + 3, F + 18) and res["faces"].dtype == faces.dtype
    assert torch.equal(res["verts"][:V], verts) and torch.equal(res["faces"][:F], faces)
    t = topology(res["verts"], res["faces"])
    assert t["boundary_edges"] == 0 and t["watertight"] and t["euler"] == 2
    # the new vertices: the fixed-point means, within half a float32 step of the float64 mean of their loops' vertices
    for j in range(3):
        members = loops["edges"][loops["edge_loop"] == j][:, 0].long()
        mean = verts[members].double().mean(0)
        assert torch.allclose(res["verts"][V + j].double(), mean, rtol=0, atol=2.0 ** -24)
        assert res["vert_src"][V + j] == loops["loop_vert"][j] == members.min()
    assert res["vert_src"].dtype == torch.int64 and res["vert_src"][:V].tolist() == list(range(V))
    assert torch.equal(res["colour"], colour[res["vert_src"]])                      # gathered, never averaged


def test_max_edges_bounds_the_loops_that_are_filled():
    from arah_release_amd import geometry
    verts, faces = mesh("sphere33_h")
    assert geometry.boundary_loops(verts, faces)["loop_edges"].tolist() == [6, 6, 6]
    assert geometry.fill_holes(verts, faces, max_edges=5)["filled"] == {"loops": 0, "faces": 0, "skipped_loops": 3}
    assert geometry.fill_holes(verts, faces, max_edges=6)["filled"] == {"loops": 3, "faces": 18, "skipped_loops": 0}
    # holes of 4, 5 and 7 or more edges: the bound separates them
    verts, faces = mesh("sphere33_sizes")
    sizes = geometry.boundary_loops(verts, faces)["loop_edges"].tolist()
    assert sorted(sizes)[:2] == [4, 5] and sorted(sizes)[2] >= 7
    for bound in (3, 4, 5, 6, 64):
        res = geometry.fill_holes(verts, faces, max_edges=bound)
        small = [n for n in sizes if n <= bound]
        assert res["filled"] == {"loops": len(small), "faces": sum(small), "skipped_loops": 3 - len(small)}, bound
        assert topology(res["verts"], res["faces"])["boundary_edges"] == sum(sizes) - sum(small)
    with pytest.raises(ValueError):
        geometry.fill_holes(verts, faces, max_edges=-1)
    with pytest.raises(ValueError):
        geometry.fill_holes(verts, faces, max_edges=2.5)


def test_clipped_sphere_reports_its_loops_and_fills_nothing():
    from arah_release_amd import geometry
    verts, faces = mesh("clipped17")
    loops = geometry.boundary_loops(verts.shape[0], faces)
    assert loops["n_loops"] == 6 and loops["n_simple"] == 6 and min(loops["loop_edges"].tolist()) > 8
    res = geometry.fill_holes(verts, faces, max_edges=8)
    assert res["filled"] == {"loops": 0, "faces": 0, "skipped_loops": 6}
    assert torch.equal(res["verts"], verts) and torch.equal(res["faces"], faces)


def test_two_holes_touching_at_a_vertex_are_reported_and_left_alone():
    from arah_release_amd import geometry
    verts, faces = mesh("sphere33_touch")
    loops = geometry.boundary_loops(verts, faces)
    assert loops["n_loops"] == 1 and loops["n_simple"] == 0 and loops["loop_simple"].tolist() == [False]
    res = geometry.fill_holes(verts, faces)
    assert res["filled"] == {"loops": 0, "faces": 0, "skipped_loops": 1} and torch.equal(res["faces"], faces)


def test_repair_mesh_orients_then_fills():
    from arah_release_amd import geometry
    verts, faces = mesh("sphere33_hr")
    before = topology(verts, faces)
    assert before["misoriented_edges"] > 0 and before["boundary_edges"] == 18
    # a hole in a misoriented neighbourhood is not simple: filling alone leaves some
    assert geometry.fill_holes(verts, faces)["filled"]["skipped_loops"] > 0
    res = geometry.repair_mesh(verts, faces)
    assert res["topology"]["watertight"] and res["topology"]["euler"] == 2
    assert res["filled"] == {"loops": 3, "faces": 18, "skipped_loops": 0}
    assert res["oriented"]["n_components"] == 1 and res["oriented"]["n_flipped"] > 0 and "faces" not in res["oriented"]
    assert torch.equal(res["faces"][:faces.shape[0]], mesh("sphere33_h")[1])        # majority: the original orientation
    assert topology(res["verts"], res["faces"]) == res["topology"]


# ---- arguments, types, exports ------------------------------------------------------------------------------------------------------
def test_arguments_and_types():
    from arah_release_amd import geometry, meshing
    verts, faces = mesh("sphere17_r")
    a = geometry.orient_mesh(verts, faces.to(torch.int32), policy="negative")
    b = geometry.orient_mesh(verts.double(), faces, policy="negative", adjacency=geometry.mesh_adjacency(verts, faces))
    assert a["faces"].dtype == torch.int32 and b["faces"].dtype == torch.int64 and torch.equal(a["faces"].long(), b["faces"])
    assert set(a) == {"faces", "flip", "face_component", "n_components", "n_nonorientable", "n_flipped", "component_faces",
                      "component_nonorientable"}
    for policy in ("negative", "positive"):
        with pytest.raises(ValueError):
            geometry.orient_mesh(verts.shape[0], faces, policy=policy)             # a volume needs the vertices
    for bad in ("largest", None, 1):
        with pytest.raises(ValueError):
            geometry.orient_mesh(verts, faces, policy=bad)
    with pytest.raises(ValueError):
        geometry.orient_mesh(verts, faces.float())
    with pytest.raises(ValueError):
        geometry.fill_holes(verts, faces, attributes={"verts": verts})
    with pytest.raises(ValueError):
        geometry.fill_holes(verts, faces, attributes={"short": verts[:-1]})
    # the lattices: powers of two, the volume's coordinates inside 2^18 and the means' inside 2^36
    (origin, scale), (lo, fix_scale) = meshing.orient_quant(verts), meshing.fill_quant(verts)
    for s, bits, o in ((scale, 18, origin), (fix_scale, 36, lo)):
        assert np.frexp(s)[0] == 0.5 and float((verts.double() - torch.tensor(o, dtype=torch.float64)).abs().max()) * s <= 2.0 ** bits
    assert meshing.orient_quant(torch.zeros(0, 3)) == ([0.0, 0.0, 0.0], 1.0)
    assert meshing.fill_quant(torch.full((4, 3), float("nan"))) == ([0.0, 0.0, 0.0], 1.0)
    # the mesh_topology key set stays what it was
    assert set(topology(verts, faces)) == {"faces", "edges", "boundary_edges", "nonmanifold_edges", "misoriented_edges",
                                           "isolated_vertices", "max_valence", "euler", "skipped_faces", "manifold", "watertight"}


def test_new_entries_are_declared_and_exported():
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
    source = open(os.path.join(REPO, "arah_release_amd", "csrc", "meshorient.hpp")).read()
    kernels = set(re.findall(r"__global__[^\n]*?void (k_[a-z0-9_]+)\(", source))
    assert kernels and all(k.startswith("k_mo_") for k in kernels)
