"""Casting rays against meshes (DESIGN.md "Casting rays against meshes on the device"), the host side: the specification
meshing.mesh_raycast against a scalar restatement of its rule, its watertightness on jittered spheres, and the entries of
`geometry` built on it -- cast_rays, occluded, vertex_visibility, ambient_occlusion, camera_rays -- against each other and against
the rasteriser.  The kernel is held to the specification in test_mesh_raycast_gpu.py, which takes its cases from here."""
import math

import numpy as np
import pytest
import torch

F32 = torch.float32
INF = float("inf")
NAN = float("nan")


def T(x, dtype=F32):
    return torch.tensor(x, dtype=dtype)


# ---- the rule, one ray and one face at a time, in Python floats (IEEE double, one rounding per operation) -------------------
def scalar_face(o, d, tri, cull):
    """-> None (not accepted whatever the window) or (t, bary_0, bary_1, bary_2); o, d: 3 floats, tri: 3 x 3 floats."""
    ad = [abs(x) for x in d]
    kz = 0 if (ad[0] >= ad[1] and ad[0] >= ad[2]) else (1 if ad[1] >= ad[2] else 2)
    kx = (kz + 1) % 3
    ky = (kx + 1) % 3
    if d[kz] < 0:
        kx, ky = ky, kx
    Sx, Sy, Sz = d[kx] / d[kz], d[ky] / d[kz], 1.0 / d[kz]
    if not all(math.isfinite(x) for p in tri for x in p):
        return None
    P, P0 = [], []
    for p in tri:
        x0, y0, z = p[kx] - o[kx], p[ky] - o[ky], p[kz] - o[kz]
        P0.append((x0, y0, z))
        P.append((x0 - Sx * z, y0 - Sy * z, z))
    (Ax, Ay, Az), (Bx, By, Bz), (Cx, Cy, Cz) = P
    U = Cx * By - Cy * Bx
    V = Ax * Cy - Ay * Cx
    W = Bx * Ay - By * Ax
    if (U < 0 or V < 0 or W < 0) and (U > 0 or V > 0 or W > 0):
        return None
    det = (U + V) + W
    if det == 0 or det != det:
        return None
    if (cull == "back" and det < 0) or (cull == "front" and det > 0):
        return None
    t = ((U * (Sz * Az) + V * (Sz * Bz)) + W * (Sz * Cz)) / det
    if not math.isfinite(t):
        return None
    # on the ray: bary . (corners - o) against t d, per axis, within 2^-26 of the largest coordinate magnitude
    b = (U / det, V / det, W / det)
    tol = max(abs(x) for p in list(tri) + [o] for x in p) * 2.0 ** -26
    for axis, k in enumerate((kx, ky, kz)):
        r = ((b[0] * P0[0][axis] + b[1] * P0[1][axis]) + b[2] * P0[2][axis]) - t * d[k]
        if not abs(r) <= tol:
            return None
    return (t,) + b


def scalar_raycast(tris, origins, dirs, t_min=0.0, t_max=INF, cull="none"):
    tris, origins, dirs = (np.asarray(x, np.float32).astype(np.float64).tolist() for x in (tris, origins, dirs))
    ts, faces, barys = [], [], []
    for o, d in zip(origins, dirs):
        best = (INF, -1, (0.0, 0.0, 0.0))
        if all(math.isfinite(x) for x in o + d) and any(x != 0 for x in d):
            for f, tri in enumerate(tris):
                r = scalar_face(o, d, tri, cull)
                if r is None:
                    continue
                t = r[0]
                if not (t_min <= t <= t_max):
                    continue
                if best[1] < 0 or t < best[0]:          # faces in ascending order: a tie keeps the lower id
                    best = (t, f, r[1:])
        ts.append(best[0])
        faces.append(best[1])
        barys.append(best[2])
    return np.array(ts, np.float64), np.array(faces, np.int32), np.array(barys, np.float64).reshape(-1, 3)


def bits(x):
    x = x.detach().cpu().contiguous()
    return x.view(torch.int64) if x.dtype == torch.float64 else (x.view(torch.int32) if x.dtype == F32 else x)


def assert_same(got, want, what=""):
    """t, face, bary equal bit for bit (sign of zero included)."""
    for k, (g, w) in enumerate(zip(got[:3], want[:3])):
        g = g if isinstance(g, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(g))
        w = w if isinstance(w, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(w))
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        same = bits(g) == bits(w)
        assert bool(same.all()), (what, ("t", "face", "bary")[k], int((~same).sum()), torch.nonzero(~same)[:4].tolist())


# ---- the handmade set ----------------------------------------------------------------------------------------------------------
TRI = [[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]]          # normal (b-a)x(c-a) = +z
E = 2.0 ** -20


def _down(points, z=1.0):
    """rays from height z straight down (z < 0: straight up) through the (x, y) given"""
    return [[x, y, z] for x, y in points], [[0.0, 0.0, -1.0 if z > 0 else 1.0]] * len(points)


def box_tris(h=1.0):
    """the 12 triangles of the cube [-h, h]^3, outward normals"""
    v = [[x, y, z] for z in (-h, h) for y in (-h, h) for x in (-h, h)]
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    return [[v[q[0]], v[q[i]], v[q[i + 1]]] for q in quads for i in (1, 2)]


NINE = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [1, 1, 0], [1, -1, 1], [-1, -1, -1]]


def handmade_cases():
    """-> list of (name, tris, origins, dirs, keywords).  Every face is finite except in the case "nan_vertex"."""
    cases = []
    inside = [(0.25, 0.25), (0.5, 0.125), (0.0625, 0.75)]
    edges = [(0.5, 0.0), (0.0, 0.5), (0.5, 0.5), (0.25, 0.0), (0.25, 0.75)]
    corners = [(0.0, 0.0), (1.0, 0.0), (0.0, 1.0)]
    outside = [(0.5, -E), (-E, 0.5), (0.5 + E, 0.5 + E), (-E, -E), (1.0 + E, 0.0), (0.0, 1.0 + E)]
    for z in (1.0, -1.0):
        o, d = _down(inside + edges + corners + outside, z)
        for cull in ("none", "back", "front"):
            cases.append(("triangle_z%+d_%s" % (z, cull), TRI, o, d, {"cull": cull}))
    # a slanted ray through the same points, so that Sx and Sy are not zero
    pts = inside + edges + corners + outside
    cases.append(("triangle_slanted", TRI, [[x - 0.5, y + 0.25, 1.0] for x, y in pts], [[0.5, -0.25, -1.0]] * len(pts), {}))
    # in the triangle's plane: det == 0
    cases.append(("in_plane", TRI, [[-1.0, 0.25, 0.0], [0.25, -1.0, 0.0], [2.0, 2.0, 0.0]],
                  [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [-1.0, -1.0, 0.0]], {}))
    # in the plane of a face that is NOT an axis plane, passing far beside the face: two of U, V, W are exactly 0, the third and
    # det are rounding noise, and only the rule's on-the-ray condition makes these the misses they are.  Then rays in the same
    # plane that do cross the face (through an edge and out through a corner): in-plane they are, det noise or 0, misses too.
    slanted = [[[-5.0, -3.0, 11.0], [-7.0, 0.0, 11.0], [-4.0, -8.0, 6.0]]]
    cases.append(("in_plane_slanted", slanted,
                  [[45.0, 97.0, 261.0], [-5.0, -3.0, 11.0], [-7.0, 0.0, 11.0], [-6.0, -1.5, 11.0], [-3.0, -13.0, 1.0]],
                  [[-5.0, 4.0, -5.0], [2.0, -3.0, 0.0], [3.0, -8.0, -5.0], [2.0, -6.5, -5.0], [-2.0, 3.0, 0.0]],
                  {"t_min": -INF}))
    # t exactly at the ends of the window (the hit is at t = 1 and, with the direction halved, at t = 2), and just beyond
    o, d = _down([(0.25, 0.25)])
    up, below = math.nextafter(1.0, 2.0), math.nextafter(1.0, 0.0)
    for name, kw in (("t_at_min", {"t_min": 1.0}), ("t_at_max", {"t_max": 1.0}), ("t_past_min", {"t_min": up}),
                     ("t_before_max", {"t_max": below}), ("t_window_point", {"t_min": 1.0, "t_max": 1.0}),
                     ("t_negative", {"t_min": -INF, "t_max": INF})):
        cases.append((name, TRI, o + [[0.25, 0.25, -1.0]], d + d, kw))
    cases.append(("t_half_dir", TRI, o, [[0.0, 0.0, -0.5]], {"t_min": 2.0, "t_max": 2.0}))
    # the nine directions from the centre of a cube: through faces' diagonals, an edge and a corner
    cases.append(("nine_directions", box_tris(), [[0.0, 0.0, 0.0]] * 9, [[float(x) for x in v] for v in NINE], {}))
    cases.append(("nine_directions_off_centre", box_tris(), [[0.125, -0.25, 0.0625]] * 9, [[float(x) for x in v] for v in NINE], {}))
    # rays that are no rays
    o, d = _down([(0.25, 0.25)] * 5)
    d[0] = [0.0, 0.0, 0.0]
    o[1] = [NAN, 0.25, 1.0]
    d[2] = [INF, 0.0, -1.0]
    o[3] = [0.25, INF, 1.0]
    d[4] = [0.0, NAN, -1.0]
    cases.append(("bad_rays", TRI, o + [[0.25, 0.25, 1.0]], d + [[0.0, 0.0, -1.0]], {}))
    # degenerate faces (two equal corners; three collinear ones) next to a real one
    degenerate = [[[0.0, 0.0, 0.5], [1.0, 0.0, 0.5], [1.0, 0.0, 0.5]], [[0.0, 0.0, 0.25], [0.5, 0.5, 0.25], [1.0, 1.0, 0.25]]] + TRI
    o, d = _down(inside + [(0.5, 0.0), (0.5, 0.5), (0.25, 0.25), (1.0, 0.0)])
    cases.append(("degenerate", degenerate, o, d, {}))
    # a face with a corner that is not finite, in front of a real one
    bad = [[[NAN, 0.0, 0.5], [1.0, 0.0, 0.5], [0.0, 1.0, 0.5]], [[0.0, 0.0, 0.75], [INF, 0.0, 0.75], [0.0, 1.0, 0.75]]] + TRI
    o, d = _down(inside + corners)
    cases.append(("nan_vertex", bad, o, d, {}))
    # two identical coplanar faces, and one behind them: the lower id wins
    twin = [[[0.0, 0.0, -1.0], [1.0, 0.0, -1.0], [0.0, 1.0, -1.0]]] + TRI + TRI
    o, d = _down(inside + edges + corners)
    cases.append(("twins", twin, o, d, {}))
    return cases


def case_tensors(case, dev="cpu"):
    name, tris, o, d, kw = case
    return T(tris).to(dev), T(o).to(dev), T(d).to(dev), kw


def test_specification_equals_the_scalar_rule_on_the_handmade_set():
    from arah_release_amd import meshing
    hits = {}
    for case in handmade_cases():
        tris, o, d, kw = case_tensors(case)
        got = meshing.mesh_raycast(tris, o, d, **kw)
        assert got[0].dtype == torch.float64 and got[1].dtype == torch.int32 and got[2].dtype == torch.float64
        assert_same(got, scalar_raycast(tris.numpy(), o.numpy(), d.numpy(), **kw), case[0])
        hits[case[0]] = got[1].tolist()
        miss = got[1] < 0
        assert bool(torch.isinf(got[0][miss]).all()) and bool((got[2][miss] == 0).all()), case[0]
    # what the set is there for, spelt out.  Rays 0..10 of the triangle cases are inside or on the closed triangle, 11.. outside.
    assert hits["triangle_z+1_none"] == [0] * 11 + [-1] * 6 and hits["triangle_z-1_none"] == [0] * 11 + [-1] * 6
    # THE SIGN: a ray coming down on the face whose normal points up meets its FRONT: det > 0, kept by cull="back"
    assert hits["triangle_z+1_back"] == [0] * 11 + [-1] * 6 and hits["triangle_z+1_front"] == [-1] * 17
    assert hits["triangle_z-1_front"] == [0] * 11 + [-1] * 6 and hits["triangle_z-1_back"] == [-1] * 17
    assert hits["in_plane"] == [-1] * 3
    assert hits["in_plane_slanted"][0] == -1          # without the on-the-ray condition: face 0 at t = 10.4, 138 units off the ray
    assert hits["t_at_min"] == [0, -1] and hits["t_at_max"] == [0, -1] and hits["t_window_point"] == [0, -1]
    assert hits["t_past_min"] == [-1, -1] and hits["t_before_max"] == [-1, -1] and hits["t_negative"] == [0, 0]
    assert hits["t_half_dir"] == [0]
    assert all(f >= 0 for f in hits["nine_directions"] + hits["nine_directions_off_centre"])
    assert hits["bad_rays"] == [-1] * 5 + [0]
    assert all(f == 2 for f in hits["degenerate"]) and all(f == 2 for f in hits["nan_vertex"])
    assert all(f == 1 for f in hits["twins"])


def random_scene(n_faces=600, n_rays=512, seed=0):
    g = torch.Generator().manual_seed(seed)
    centre = torch.rand(n_faces, 1, 3, generator=g) * 2.0 - 1.0
    tris = (centre + (torch.rand(n_faces, 3, 3, generator=g) - 0.5) * 0.3).to(F32)
    o = (torch.rand(n_rays, 3, generator=g) * 2.0 - 1.0).to(F32)
    d = torch.randn(n_rays, 3, generator=g).to(F32)
    return tris, o, d


def test_specification_equals_the_scalar_rule_on_random_faces():
    from arah_release_amd import meshing
    tris, o, d = random_scene()
    for kw in ({}, {"cull": "back", "t_min": 0.25, "t_max": 1.5}):
        got = meshing.mesh_raycast(tris, o, d, **kw)
        assert_same(got, scalar_raycast(tris.numpy(), o.numpy(), d.numpy(), **kw), str(kw))
        assert 0.05 < float((got[1] >= 0).float().mean()) < 1.0   # the scene is neither empty nor a wall
    # the chunking changes nothing
    assert_same(meshing.mesh_raycast(tris, o, d, chunk_bytes=1 << 16), meshing.mesh_raycast(tris, o, d))


def in_plane_scene(n_faces=40, rays_per_face=100, seed=11):
    """Faces with small integer corners, and for each face rays that lie in ITS plane: from a point of the plane (an integer
    combination of the corners, up to 60 away) towards another.  Most of them pass beside the face."""
    g = torch.Generator().manual_seed(seed)
    tris = torch.randint(-9, 10, (n_faces, 3, 3), generator=g).to(torch.float64)
    o, d = [], []
    for f in range(n_faces):
        a, e1, e2 = tris[f, 0], tris[f, 1] - tris[f, 0], tris[f, 2] - tris[f, 0]
        c = torch.randint(-6, 7, (rays_per_face, 4), generator=g).to(torch.float64)
        p, q = a + c[:, 0:1] * e1 + c[:, 1:2] * e2, a + c[:, 2:3] * e1 + c[:, 3:4] * e2
        o.append(p)
        d.append(q - p)
    return tris.to(F32), torch.cat(o).to(F32), torch.cat(d).to(F32)


def test_rays_in_the_plane_of_a_face_miss_it():
    """What the on-the-ray condition is for: no in-plane ray may be answered with a point that is not on it.  For every accepted
    hit the point bary . corners is recomputed here and must lie within 1e-5 of o + t d (the coordinates are below 200; 2^-26 of
    them is 3e-6)."""
    from arah_release_amd import meshing
    tris, o, d = in_plane_scene()
    for kw in ({"t_min": -INF}, {}):
        got = meshing.mesh_raycast(tris, o, d, **kw)
        assert_same(got, scalar_raycast(tris.numpy(), o.numpy(), d.numpy(), **kw), "in-plane " + str(kw))
        hit = got[1] >= 0
        q = (got[2][:, :, None] * tris.double()[got[1].long().clamp_min(0)]).sum(1)
        on = q - (o.double() + got[0][:, None] * d.double())
        off = float(on[hit].abs().max()) if bool(hit.any()) else 0.0
        print("in-plane rays %s: %d of %d hit something, farthest accepted point %.3g off its ray" % (kw, int(hit.sum()), o.shape[0], off))
        assert int(hit.sum()) > 100 and off <= 1e-5            # they do hit OTHER faces, on the ray
    # a ray against the one face whose plane it lies in: a miss, or -- where the ray does cross the face and the noise in det
    # lets it through -- a point on the ray AND in the face's box; never the corner far beside the ray that Woop's test alone gives
    own = torch.arange(tris.shape[0]).repeat_interleave(o.shape[0] // tris.shape[0])
    n_hit = 0
    for f in range(tris.shape[0]):
        rows = own == f
        t, face, bary = meshing.mesh_raycast(tris[f:f + 1], o[rows], d[rows], t_min=-INF)
        hit = face >= 0
        p = (o[rows].double() + t[:, None] * d[rows].double())[hit]
        lo, hi = tris[f].double().min(0).values, tris[f].double().max(0).values
        assert bool(((p >= lo - 1e-5) & (p <= hi + 1e-5)).all()), f
        n_hit += int(hit.sum())
    print("in-plane rays against their own face alone: %d of %d accepted, all on the face" % (n_hit, o.shape[0]))


# ---- watertightness ------------------------------------------------------------------------------------------------------------
def uv_sphere(n_lon=24, n_lat=16, jitter=0.0, seed=0):
    """-> verts (V,3) float32, faces (F,3) int64 with outward normals: two poles, n_lat - 1 rings; every vertex's radius is
    1 +- jitter and its angles move by up to jitter / 4 of a step."""
    g = torch.Generator().manual_seed(seed)
    lat = torch.arange(1, n_lat, dtype=torch.float64)[:, None].expand(n_lat - 1, n_lon)
    lon = torch.arange(n_lon, dtype=torch.float64)[None, :].expand(n_lat - 1, n_lon)
    lat = (lat + (torch.rand(lat.shape, generator=g, dtype=torch.float64) - 0.5) * jitter * 0.5) * (math.pi / n_lat)
    lon = (lon + (torch.rand(lon.shape, generator=g, dtype=torch.float64) - 0.5) * jitter * 0.5) * (2.0 * math.pi / n_lon)
    ring = torch.stack([torch.sin(lat) * torch.cos(lon), torch.sin(lat) * torch.sin(lon), torch.cos(lat)], dim=-1).reshape(-1, 3)
    verts = torch.cat([torch.tensor([[0.0, 0.0, 1.0]], dtype=torch.float64), ring, torch.tensor([[0.0, 0.0, -1.0]], dtype=torch.float64)])
    verts = verts * (1.0 + (torch.rand(verts.shape[0], 1, generator=g, dtype=torch.float64) * 2.0 - 1.0) * jitter)
    idx = lambda i, j: 1 + i * n_lon + (j % n_lon)
    south = 1 + (n_lat - 1) * n_lon
    faces = []
    for j in range(n_lon):
        faces.append([0, idx(0, j), idx(0, j + 1)])
        for i in range(n_lat - 2):
            faces.append([idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)])
            faces.append([idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)])
        faces.append([south, idx(n_lat - 2, j + 1), idx(n_lat - 2, j)])
    return verts.to(F32), torch.tensor(faces, dtype=torch.int64)


def sphere_targets(verts, faces, n_random=0, seed=0):
    """the points the rays go through: every vertex, every edge's midpoint and quarter point (per face and edge: an edge is met
    from both of its faces, so its midpoint twice and its quarter points from either end), every centroid; then n_random
    random directions"""
    p = verts[faces].double()
    a, b = p, p.roll(-1, dims=1)
    parts = [verts.double(), (0.5 * (a + b)).reshape(-1, 3), (a + 0.25 * (b - a)).reshape(-1, 3), p.mean(1)]
    if n_random:
        parts.append(torch.randn(n_random, 3, generator=torch.Generator().manual_seed(seed), dtype=torch.float64))
    return torch.cat(parts)


def sphere_rays(k, n_random=0):
    """sphere k of the six: -> verts, faces, origins, dirs -- the targets seen from a random interior point and from exactly 0,
    then the nine directions from 0"""
    verts, faces = uv_sphere(jitter=0.2, seed=100 + k)
    g = torch.Generator().manual_seed(200 + k)
    inner = ((torch.rand(3, generator=g) * 2.0 - 1.0) * 0.3).to(F32)
    targets = sphere_targets(verts, faces, n_random, seed=300 + k)
    o, d = [], []
    for origin in (inner, torch.zeros(3)):
        o.append(origin[None, :].expand(targets.shape[0], 3))
        d.append((targets - origin.double()).to(F32))
    o.append(torch.zeros(9, 3))
    d.append(T(NINE))
    return verts, faces, torch.cat(o).contiguous(), torch.cat(d).contiguous()


def test_the_rule_is_watertight_on_jittered_spheres():
    from arah_release_amd import meshing
    total = misses = fan = 0
    for k in range(6):
        verts, faces, o, d = sphere_rays(k, n_random=2000)
        assert verts.shape[0] == 362 and faces.shape[0] == 720
        t, face, bary = meshing.mesh_raycast(verts[faces], o, d)
        total += int(o.shape[0])
        misses += int((face < 0).sum())
        assert bool((t[face >= 0] > 0).all())
        # the ray from 0 through the north pole: all 24 faces of the fan accept it, the tie rule is exercised
        n_t = 362 + 4 * 2160 // 2 + 720 + 2000
        pole = n_t   # first ray of the second origin: the target is vertex 0
        assert bool((o[pole] == 0).all()) and torch.equal(d[pole], verts[0])
        accepted = sum(scalar_raycast(verts[faces][f:f + 1].numpy(), o[pole:pole + 1].numpy(), d[pole:pole + 1].numpy())[1][0] >= 0
                       for f in range(720))
        fan += accepted
        assert int(face[pole]) % 30 == 0 and int(face[pole]) < 720   # a face of the fan: the first of its column
    print("watertightness: %d rays, %d misses, pole rays accepted by %d faces in all" % (total, misses, fan))
    assert total == 88878 and misses == 0
    assert fan == 6 * 24


# ---- cameras ---------------------------------------------------------------------------------------------------------------------
def opencv_camera(H, W, dist=3.0):
    a, b = 0.3, -0.2
    Ry = torch.tensor([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]], dtype=torch.float64)
    Rx = torch.tensor([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]], dtype=torch.float64)
    R = (Rx @ Ry).to(F32)
    return {"cam_rot": R, "cam_trans": T([0.05, -0.1, dist]), "K": T([[1.1 * W, 0, W / 2 + 0.3], [0, 1.1 * W, H / 2 - 0.7], [0, 0, 1]])}


CAMERAS = [("opencv", lambda H, W: opencv_camera(H, W)), ("lookat", lambda H, W: {"azim": 30.0, "dist": 3.0, "fov": 50.0}),
           ("lookat_at", lambda H, W: {"azim": 200.0, "dist": 2.5, "at": (0.1, -0.2, 0.05)})]
# Measured here (host, float32 project_mesh of float32 origin + dir, 48 x 64 and 37 x 23 images): the largest distance of the
# re-projected point from the pixel centre is 1.53e-5 pixels (opencv), 7.63e-6 (lookat), 7.63e-6 (lookat_at); the view depth is
# within 2.38e-7 of 1 (two float32 steps).
REPROJECTION_TOL = 4 * 1.53e-5
REPROJECTION_DEPTH_TOL = 4 * 2.38e-7


@pytest.mark.parametrize("name,make", CAMERAS)
def test_camera_rays_go_through_the_pixel_centres_of_project_mesh(name, make):
    from arah_release_amd import geometry
    worst = worst_z = 0.0
    for H, W in ((48, 64), (37, 23)):
        cam = make(H, W)
        o, d = geometry.camera_rays(cam, H, W)
        assert o.shape == (H * W, 3) and d.shape == (H * W, 3) and o.dtype == F32 and d.dtype == F32
        uvz = geometry.project_mesh(o + d, cam, H, W)
        jj = (torch.arange(W, dtype=F32) + 0.5)[None, :].expand(H, W).reshape(-1)
        ii = (torch.arange(H, dtype=F32) + 0.5)[:, None].expand(H, W).reshape(-1)
        worst = max(worst, float(torch.maximum((uvz[:, 0] - jj).abs(), (uvz[:, 1] - ii).abs()).max()))
        worst_z = max(worst_z, float((uvz[:, 2] - 1.0).abs().max()))
    print("camera_rays %s: re-projection error %.3g pixels, depth error %.3g" % (name, worst, worst_z))
    assert worst <= REPROJECTION_TOL and worst_z <= REPROJECTION_DEPTH_TOL


def test_camera_rays_argument_checks():
    from arah_release_amd import geometry
    for cam, H, W in (({"azim": 0.0, "K": torch.eye(3)}, 8, 8), ({"azim": 0.0}, 0, 8), ({"azim": 0.0}, 8, 2.5), (None, 8, 8)):
        with pytest.raises(ValueError):
            geometry.camera_rays(cam, H, W)


# ---- the entries of geometry on the host ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere():
    return uv_sphere()


@pytest.fixture(scope="module")
def dented():
    """the sphere with vertex 100 pushed inward to a third of the radius"""
    verts, faces = uv_sphere()
    verts = verts.clone()
    verts[100] *= 1.0 / 3.0
    return verts, faces


def test_argument_checks():
    from arah_release_amd import geometry, meshing
    verts, faces = uv_sphere(8, 6)
    o, d = torch.zeros(4, 3), torch.ones(4, 3)
    bad = [lambda: meshing.mesh_raycast(verts[faces].double(), o, d), lambda: meshing.mesh_raycast(verts[faces], o.double(), d),
           lambda: meshing.mesh_raycast(verts[faces], o, d[:3]), lambda: meshing.mesh_raycast(verts[faces][:0], o, d),
           lambda: meshing.mesh_raycast(verts[faces], o, d, cull="both"), lambda: meshing.mesh_raycast(verts[faces], o, d, t_min=NAN),
           lambda: meshing.mesh_raycast(verts[faces], o, d, t_max="far"), lambda: meshing.mesh_raycast(verts[faces], o[:, :2], d),
           lambda: geometry.cast_rays((verts, faces), o, d[:3]), lambda: geometry.cast_rays((verts, faces.float()), o, d),
           lambda: geometry.cast_rays(verts[faces], o, d, attributes={"vertex_normal": True}),
           lambda: geometry.cast_rays((verts, faces), o, d, attributes={"colour": torch.zeros(3, 3)}),
           lambda: geometry.cast_rays((verts, faces), o, d, attributes={"t": torch.zeros(verts.shape[0], 3)}),
           lambda: geometry.cast_rays((verts, faces), o, d, attributes={"face_normal": True}),
           lambda: geometry.cast_rays((verts, faces), o, d, index=object()),
           lambda: geometry.cast_rays((verts, faces), o, d, cull="sideways"),
           lambda: geometry.occluded((verts, faces), o, d.long(), 0.0, 1.0), lambda: geometry.occluded((verts, faces), o, d, 0.0, NAN),
           lambda: geometry.vertex_visibility(verts, faces, (0.0, 1.0)), lambda: geometry.vertex_visibility(verts, faces, (0.0, 0.0, 3.0), eps=-1.0),
           lambda: geometry.ambient_occlusion(verts, faces, n_rays=0), lambda: geometry.ambient_occlusion(verts, faces, n_rays=2.5),
           lambda: geometry.ambient_occlusion(verts, faces, radius=0.0), lambda: geometry.ambient_occlusion(verts, faces, eps=-1e-3),
           lambda: geometry.ambient_occlusion(verts[:, :2], faces)]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail("call %d was accepted" % k)
    res = geometry.cast_rays((verts, faces), o[:0], d[:0], attributes={"vertex_normal": True})
    assert res["t"].shape == (0,) and res["points"].shape == (0, 3) and res["vertex_normal"].shape == (0, 3)


def test_a_face_with_an_id_out_of_range_is_never_hit(sphere):
    from arah_release_amd import geometry
    verts, faces = sphere
    o, d = T([[0.0, 0.0, 0.0]] * 2), T([[0.3, 0.2, -1.0], [-0.4, 0.1, 0.7]])
    good = geometry.cast_rays((verts, faces), o, d)
    assert bool(good["hit"].all())
    broken = faces.clone()
    broken[good["face"].long()[0], 1] = verts.shape[0]                  # the face the first ray hits names a vertex that is not there
    res = geometry.cast_rays((verts, broken), o, d, attributes={"vertex_normal": True})
    assert not bool(res["hit"][0]) and bool(res["hit"][1]) and int(res["face"][1]) == int(good["face"][1])
    assert bool((res["vertex_normal"][0] == 0).all())
    assert geometry.occluded((verts, broken), o, d, 0.0, INF).tolist() == [False, True]


def test_a_convex_mesh_is_open_and_visible(sphere):
    from arah_release_amd import geometry
    verts, faces = sphere
    ao = geometry.ambient_occlusion(verts, faces)
    assert ao.shape == (verts.shape[0],) and ao.dtype == F32 and bool((ao == 1.0).all())
    n = geometry.vertex_normals(verts, faces)
    for v in (0, 57, 200, 361):   # from outside, along the vertex's own normal, every vertex it faces is seen, the far side is not
        seen = geometry.vertex_visibility(verts, faces, verts[v] + 2.0 * n[v])
        assert seen.dtype == torch.bool and bool(seen[v])
        facing = (n * (verts[v] + 2.0 * n[v] - verts)).sum(1)
        # (the horizon of the unit sphere from an eye at radius 3 is facing = 0; the faces sag below the sphere by up to 1.3 %,
        # which lets the eye see a little beyond it)
        assert bool(seen[facing > 0.2].all()) and not bool(seen[facing < -0.5].any())
        assert 0 < int(seen.sum()) < verts.shape[0] // 2
    # every vertex from its own eye: one segment per vertex
    eyes = verts + 2.0 * n
    start = verts + 1e-4 * n
    assert not bool(geometry.occluded((verts, faces), start, eyes - start, 0.0, 1.0).any())


def test_a_dent_is_occluded(dented):
    from arah_release_amd import geometry
    verts, faces = dented
    ao = geometry.ambient_occlusion(verts, faces)
    antipode = int(((verts + verts[100] * 3.0).norm(dim=1)).argmin())
    print("AO in the dent %.3f, at the antipode %.3f, smallest %.3f" % (float(ao[100]), float(ao[antipode]), float(ao.min())))
    assert float(ao[100]) < 1.0 and float(ao[antipode]) == 1.0
    assert bool(((ao >= 0) & (ao <= 1)).all())
    assert torch.equal(ao * 64, (ao * 64).round())                     # a count over 64
    assert bool((geometry.ambient_occlusion(verts, faces, radius=0.05) >= ao).all())     # a shorter reach hides no more
    assert bool((geometry.ambient_occlusion(verts, faces, radius=1e-6) == 1.0).all())    # the rays start 1e-4 off the surface
    assert torch.equal(geometry.ambient_occlusion(verts, faces, adjacency=geometry.mesh_adjacency(verts, faces)), ao)
    few = geometry.ambient_occlusion(verts, faces, n_rays=7, seed=5)
    assert torch.equal(few * 7, (few * 7).round()) and float(few[100]) < 1.0
    # from straight above the dent its bottom is seen, from the side it is not
    out = verts[100] * 3.0
    assert bool(geometry.vertex_visibility(verts, faces, out * 3.0)[100])
    side = torch.linalg.cross(out, T([0.3, 0.5, 0.8]))
    assert not bool(geometry.vertex_visibility(verts, faces, out + 3.0 * side / side.norm())[100])


# Measured here (host): the distance of `points` -- re-evaluated from bary and the corners in float64 -- from origin + t dir, for the
# 5 402 x 2 + 9 rays of sphere 0 (|t dir| about 1): at most 5.24e-16.
ON_RAY_TOL = 4 * 5.24e-16


def test_cast_rays_points_lie_on_the_rays_and_attributes_follow_the_rule(sphere):
    from arah_release_amd import geometry, meshing
    verts, faces, o, d = sphere_rays(0)
    colour = torch.rand(verts.shape[0], 5, generator=torch.Generator().manual_seed(3))
    res = geometry.cast_rays((verts, faces), o, d, attributes={"colour": colour, "vertex_normal": True})
    assert set(res) == {"hit", "t", "face", "bary", "points", "normal", "colour", "vertex_normal"}
    assert bool(res["hit"].all())
    spec = meshing.mesh_raycast(verts[faces], o, d)
    assert_same((res["t"], res["face"], res["bary"]), spec)
    tri = verts[faces].double()[res["face"].long()]
    again = (res["bary"][:, 0:1] * tri[:, 0] + res["bary"][:, 1:2] * tri[:, 1]) + res["bary"][:, 2:3] * tri[:, 2]
    assert torch.equal(again, res["points"])
    off = (again - (o.double() + res["t"][:, None] * d.double())).norm(dim=1).max()
    print("points off their rays by at most %.3g" % float(off))
    assert float(off) <= ON_RAY_TOL
    # the normal is the face's, and the ray leaves through it
    assert torch.equal(res["normal"], geometry.face_normals(verts, faces)[res["face"].long()])
    assert bool(((res["normal"].double() * d.double()).sum(1) > 0).all())
    # attributes: the rule of interpolate_attributes on the float32 barycentrics
    R = o.shape[0]
    for name, a in (("colour", colour), ("vertex_normal", geometry.vertex_normals(verts, faces))):
        want = meshing.interpolate_attributes(res["face"].reshape(1, R), res["bary"].float().reshape(1, R, 3), faces, a)[0]
        assert torch.equal(res[name], want)
    # a soup gives the same hits; misses are zero
    soup = geometry.cast_rays(verts[faces], o, d, t_max=0.5)
    assert not bool(soup["hit"].any()) and bool((soup["points"] == 0).all()) and bool((soup["normal"] == 0).all())
    culled = geometry.cast_rays(verts[faces], o, d, cull="front")           # from inside every hit is on a back
    assert_same((culled["t"], culled["face"], culled["bary"]), spec)
    assert not bool(geometry.cast_rays(verts[faces], o, d, cull="back")["hit"].any())
    assert torch.equal(geometry.occluded((verts, faces), o, d, 0.0, INF), res["hit"])


# Measured here (host): |depth - t| over the agreeing pixels of the three cameras at 48 x 64 -- the rasteriser's float32 depth
# against the ray's float64 t along a direction of view depth 1 -- is at most 2.17e-6 (opencv), 7.66e-6 (lookat), 1.51e-6
# (lookat_at) at depths of 2 to 3: the rasteriser works on corners projected to float32 pixels and interpolates 1/z in float32.
DEPTH_TOL = 4 * 7.66e-6


def raster_against_rays(raster, cast, H, W):
    """The conditions under which the rasteriser and the ray caster see one mesh alike: -> (disagreeing interior pixels, largest
    |depth - t| where both name the same face, number of such pixels)."""
    m_r, m_c = raster["mask"].reshape(H, W), cast["hit"].reshape(H, W)

    def no_background_neighbour(m):   # the image's border counts as background
        p = torch.nn.functional.pad(m, (1, 1, 1, 1))
        return p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:]
    both = no_background_neighbour(m_r) & no_background_neighbour(m_c)
    bad = int((both & (m_r != m_c)).sum())
    same = (raster["pix_to_face"].reshape(-1) == cast["face"]) & cast["hit"]
    err = (raster["depth"].reshape(-1).double() - cast["t"])[same].abs()
    return bad, (float(err.max()) if err.numel() else 0.0), int(same.sum()), int(both.sum())


@pytest.mark.parametrize("name,make", CAMERAS)
def test_render_mesh_and_cast_rays_see_the_same_sphere(sphere, name, make):
    from arah_release_amd import geometry
    verts, faces = sphere
    H, W = 48, 64
    cam = make(H, W)
    raster = geometry.render_mesh(verts, faces, H, W, camera=cam)
    o, d = geometry.camera_rays(cam, H, W)
    cast = geometry.cast_rays((verts, faces), o, d)
    bad, err, n_same, n_both = raster_against_rays(raster, cast, H, W)
    print("%s: %d interior pixels, %d with the same face, largest |depth - t| %.3g, %d disagree" % (name, n_both, n_same, err, bad))
    assert n_both > 200 and n_same > 0.9 * n_both
    assert bad == 0
    assert err <= DEPTH_TOL
