"""Geometry scores of a predicted mesh against a ground-truth mesh, on the device (DESIGN.md "Geometry metrics on the
device"): Chamfer distance, accuracy / completeness, normal consistency and the two Hausdorff distances from area-weighted
surface samples and their EXACT point-to-surface distances (hip.mesh_index / hip.mesh_closest / hip.surface_metrics).

The reference publishes such numbers but its tree holds no code for them (its README points to a script in its issue
tracker): PARITY UNPINNED, the definitions are this project's.  Also here: `load_mesh` for the two formats ground-truth meshes
come in (.npz with `vertices` / `faces`, PLY with triangle faces), and `save_mesh`, which writes an indexed mesh in either;
`mesh_components` / `clean_mesh`: the connected components of an indexed mesh and the removal of its floaters (DESIGN.md "Mesh
components on the device"); `simplify_mesh`: fewer vertices and faces by vertex clustering on a grid (DESIGN.md "Simplifying meshes
on the device") and `decimate_mesh`: fewer by edge collapse, which keeps a closed surface closed (DESIGN.md "Edge-collapse
decimation on the device"); `mesh_adjacency` / `mesh_topology` / `vertex_normals` / `smooth_mesh`: who is adjacent to whom, whether a mesh is
watertight, the mesh's own normals, and Laplacian / Taubin smoothing (DESIGN.md "Adjacency, normals and smoothing on the device");
`mesh_laplacian` / `laplacian_matrix` / `apply_laplacian` / `mesh_curvature`: the cotangent Laplacian with its lumped mass, and mean,
Gaussian and principal curvatures (DESIGN.md "Cotangent operator and curvature on the device"); `solve_laplacian` /
`harmonic_extend` / `smooth_mesh(method="implicit")`: systems solved with that operator (DESIGN.md "Solving with the cotangent
operator on the device").
Ground truth that is a SCAN -- a point cloud, with or without normals -- is scored through the exact
nearest-point query hip.point_index / hip.point_nearest (DESIGN.md "Scoring against point clouds"): `PointCloud`, `nearest_points`,
`load_points` / `save_points` / `load_geometry`, and F-scores at distance thresholds (`thresholds=` of `mesh_metrics`).
Rays against a mesh -- `cast_rays`, `occluded`, `vertex_visibility`, `camera_rays`, `ambient_occlusion` -- go through hip.mesh_raycast
on the same index (DESIGN.md "Casting rays against meshes on the device").  Whether points lie INSIDE a mesh -- `mesh_contains`,
`voxelize`, `mesh_iou` -- is the reference's crossing-parity rule over its two-dimensional triangle hash, hip.contains_index /
hip.mesh_contains / hip.mesh_contains_grid (DESIGN.md "Containment, occupancy grids and IoU on the device")."""
import collections
import math
import warnings

import numpy as np
import torch

METRIC_KEYS = ("accuracy", "completeness", "chamfer_l1", "chamfer_l2", "normal_consistency", "hausdorff_ab", "hausdorff_ba")


def _as_soup(mesh, what):
    """(F,3,3) triangles or a (verts (V,3), faces (F,3)) pair -> ((F,3,3) float32 soup on the mesh's device, 0-dim bool tensor:
    every face index is in range).  Indices are clamped into range before the gather, so a bad face never reaches the device as
    an out-of-bounds read; the flag turns the scores into NaN without a host round trip."""
    if isinstance(mesh, (tuple, list)):
        if len(mesh) != 2:
            raise ValueError("%s: a mesh is an (F, 3, 3) tensor or a (verts, faces) pair" % what)
        verts, faces = torch.as_tensor(mesh[0]), torch.as_tensor(mesh[1])
        if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
            raise ValueError("%s: verts must be (V, 3) and faces (F, 3)" % what)
        if faces.dtype.is_floating_point or faces.dtype == torch.bool:
            raise ValueError("%s: faces must hold integer vertex indices" % what)
        if faces.shape[0] < 1 or verts.shape[0] < 1:
            raise ValueError("%s is empty" % what)
        faces = faces.to(verts.device).long()
        valid = ((faces >= 0) & (faces < verts.shape[0])).all()
        tris = verts.to(torch.float32)[faces.clamp(0, verts.shape[0] - 1)]
    else:
        tris = torch.as_tensor(mesh)
        if tris.dim() != 3 or tuple(tris.shape[1:]) != (3, 3):
            raise ValueError("%s: a mesh is an (F, 3, 3) tensor or a (verts, faces) pair, got shape %s" % (what, tuple(tris.shape)))
        if tris.shape[0] < 1:
            raise ValueError("%s is empty" % what)
        tris = tris.to(torch.float32)
        valid = torch.ones((), dtype=torch.bool, device=tris.device)
    return tris.detach().contiguous(), valid


def drop_degenerate(tris):
    """Faces whose float64 cross product is exactly the zero vector leave the soup WITHOUT a host round trip: the kept faces
    move to the front in their order and the tail is filled with copies of the last kept face (a copy never wins a tie: the
    lowest index does, and its normal is the original's anyway).  -> (soup (F,3,3), n_kept 0-dim int64 on the device,
    sampling faces (F,3) int64 into soup.reshape(-1, 3): the tail's are degenerate, area-weighted sampling never draws them)."""
    F = tris.shape[0]
    t64 = tris.double()
    cross = torch.linalg.cross(t64[:, 1] - t64[:, 0], t64[:, 2] - t64[:, 0])
    keep = (cross != 0).any(-1)
    order = torch.argsort((~keep).to(torch.uint8), stable=True)
    n_kept = keep.sum()
    idx = torch.arange(F, device=tris.device)
    src = torch.where(idx < n_kept, idx, (n_kept - 1).clamp(min=0))
    soup = tris[order][src].contiguous()
    corners = (idx * 3)[:, None] + torch.arange(3, device=tris.device)[None]
    return soup, n_kept, torch.where((idx < n_kept)[:, None], corners, torch.zeros_like(corners))


class PointCloud:
    """A point cloud: points (P,3) float32 and optional unit normals (P,3) float32, tensors on one device.  ValueError for other
    shapes, an empty cloud, or normals of another length or on another device."""

    def __init__(self, points, normals=None):
        points = torch.as_tensor(points)
        if points.dim() != 2 or points.shape[1] != 3 or not points.dtype.is_floating_point:
            raise ValueError("a point cloud is a (P, 3) floating-point tensor, got shape %s" % (tuple(points.shape),))
        if points.shape[0] < 1:
            raise ValueError("the point cloud is empty")
        self.points = points.detach().to(torch.float32).contiguous()
        self.normals = None
        if normals is not None:
            normals = torch.as_tensor(normals)
            if tuple(normals.shape) != tuple(points.shape) or not normals.dtype.is_floating_point:
                raise ValueError("normals must be (P, 3) = %s, got %s" % (tuple(points.shape), tuple(normals.shape)))
            if normals.device != points.device:
                raise ValueError("points live on %s, normals on %s" % (points.device, normals.device))
            self.normals = normals.detach().to(torch.float32).contiguous()

    @property
    def device(self):
        return self.points.device

    def tensors(self):
        return (self.points,) if self.normals is None else (self.points, self.normals)

    def to(self, device):
        return PointCloud(self.points.to(device), None if self.normals is None else self.normals.to(device))

    def __len__(self):
        return int(self.points.shape[0])


def _is_cloud(x):
    """A PointCloud, or a bare (P,3) tensor / array (a triangle soup is (F,3,3), a mesh pair a tuple)."""
    if isinstance(x, PointCloud):
        return True
    if isinstance(x, (tuple, list)):
        return False
    return (torch.is_tensor(x) or isinstance(x, np.ndarray)) and x.ndim == 2 and x.shape[-1] == 3


def _as_cloud(x):
    return x if isinstance(x, PointCloud) else PointCloud(x)


def nearest_points(cloud_points, pts):
    """Nearest point of a cloud for every query: cloud_points (P,3) (or a PointCloud), pts (Q,3), both float32 on one device ->
    (d2 (Q,) float64 = dx dx + dy dy + dz dz of the float64 differences of the float32 coordinates, index (Q,) int64, the
    LOWEST index on ties).  On the GPU: hip.point_index / hip.point_nearest.  On the host: the float64 brute force below, which
    is the specification.  A cloud point with a non-finite coordinate is nobody's neighbour; a query with one answers
    (NaN, -1); a cloud without a finite point (+inf, -1)."""
    cloud = _as_cloud(cloud_points).points
    pts = torch.as_tensor(pts)
    if pts.dim() != 2 or pts.shape[1] != 3 or not pts.dtype.is_floating_point:
        raise ValueError("pts must be (Q, 3) floating point, got %s" % (tuple(pts.shape),))
    pts = pts.detach().to(torch.float32).contiguous()
    if pts.device != cloud.device:
        raise ValueError("the cloud lives on %s, pts on %s" % (cloud.device, pts.device))
    if cloud.is_cuda:
        from . import hip
        d2, idx, _ = hip.point_nearest(hip.point_index(cloud), pts)
        return d2, idx.long()
    c, q = cloud.double(), pts.double()
    usable = torch.isfinite(c).all(1)
    d2 = torch.empty(q.shape[0], dtype=torch.float64)
    idx = torch.empty(q.shape[0], dtype=torch.int64)
    order = torch.arange(c.shape[0])
    for s0 in range(0, q.shape[0], 1024):                         # chunks of queries: the (Q, P) matrix never exists whole
        d = q[s0:s0 + 1024, None, :] - c[None, :, :]
        m = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        m = torch.where(usable[None, :], m, torch.full_like(m, float("inf")))
        best = m.min(1).values
        first = torch.where(m == best[:, None], order[None, :], c.shape[0]).min(1).values   # the lowest index at the minimum
        d2[s0:s0 + 1024], idx[s0:s0 + 1024] = best, first
    none = ~usable.any()
    idx = torch.where(none | (idx >= c.shape[0]), torch.full_like(idx, -1), idx)
    bad = ~torch.isfinite(q).all(1)
    d2 = torch.where(bad, torch.full_like(d2, float("nan")), d2)
    idx = torch.where(bad, torch.full_like(idx, -1), idx)
    return d2, idx


def check_thresholds(thresholds):
    """None, or a sequence of 1 .. 16 positive finite distances in metres -> tuple of floats.  ValueError otherwise."""
    import math
    if thresholds is None:
        return None
    if isinstance(thresholds, (str, bytes)) or not isinstance(thresholds, (tuple, list, np.ndarray)) or np.ndim(thresholds) != 1:
        raise ValueError("thresholds must be a sequence of distances, got %r" % (thresholds,))
    out = []
    for t in thresholds:
        if isinstance(t, (bool, str)) or not isinstance(t, (int, float, np.integer, np.floating)):
            raise ValueError("thresholds must be numbers, got %r" % (t,))
        t = float(t)
        if not math.isfinite(t) or t <= 0.0:
            raise ValueError("thresholds must be positive and finite, got %r" % (t,))
        out.append(t)
    if not 1 <= len(out) <= 16:
        raise ValueError("between 1 and 16 thresholds are taken, got %d" % len(out))
    return tuple(out)


def within_thresholds(d2, thresholds):
    """The threshold rule on the host, the specification of the device count: for every distance t of `thresholds` the number of
    entries of d2 (float64 squared distances) with d2 <= t t, the product taken in float64 -- an entry exactly at t t is within,
    a NaN is not.  -> (T,) int64 tensor."""
    d2 = torch.as_tensor(d2, dtype=torch.float64)
    return torch.stack([(d2 <= t * t).sum() for t in check_thresholds(thresholds)]).long()


def fscore(precision, recall):
    """2 P R / (P + R), and 0 where P + R = 0 (elementwise, float64)."""
    total = precision + recall
    return torch.where(total > 0, 2.0 * precision * recall / torch.where(total > 0, total, torch.ones_like(total)),
                       torch.zeros_like(total))


def _face_normals(soup):
    """Unit normals (F,3) float64 of a soup: the float64 cross product on the float32 vertices, normalised (NaN for a face without
    one)."""
    t = soup.double()
    n = torch.linalg.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    return n / torch.sqrt((n * n).sum(-1))[:, None]


def mesh_metrics(tris_a, tris_b, n_samples=100000, seed=0, return_samples=False, thresholds=None):
    """Scores of A (the prediction) against B (the ground truth), both in world metres on one GPU.  Each is a MESH -- an (F,3,3)
    triangle soup or a (verts, faces) pair -- or a CLOUD -- a PointCloud or a bare (P,3) tensor.  From a mesh n_samples points
    are drawn area-weighted (data.sample_surface on hip.face_area_cumsum's cumulative areas) from a torch.Generator seeded with
    `seed`: A's first, then B's.  A cloud contributes all its points as its samples and draws nothing.  A sample's distance to a
    mesh is the exact point-to-surface distance (hip.mesh_closest), to a cloud the distance to its nearest point
    (hip.point_nearest).  -> dict of 0-dimensional float64 DEVICE tensors

        accuracy / completeness   mean distance of A's samples to B / of B's samples to A
        chamfer_l1, chamfer_l2    half the sum of the two mean distances / of the two mean squared distances
        normal_consistency        half the sum of the two means of |n_sample . n_nearest|: the sample's normal is its face's (mesh)
                                  or its own (cloud), the other the closest face's or the nearest point's.  NaN when a cloud
                                  without normals is involved.
        hausdorff_ab / _ba        the largest of those distances, each way

    plus n_a, n_b (the sample counts, Python ints).  thresholds = (t1, ...), up to 16 positive finite distances in metres, adds
    (T,) float64 device tensors "precision" (the share of A's samples with d2 <= t t, the product in float64, from an exact
    integer count), "recall" (the same for B's samples), "fscore" = 2 P R / (P + R) (0 when P + R = 0), and "thresholds" (the
    tuple of floats); the seven scores above keep their bits.  Nothing is copied to the host and the stream is never waited
    for; the same inputs and seed give the same bits.  A mesh all of whose faces are degenerate, a (verts, faces) pair with a face
    index out of range, or a cloud holding a non-finite point scores NaN (checked on the device: `load_mesh` / `load_points` raise
    for such a file).  return_samples=True adds "samples": the points and their faces (indices into the soups "tris_a" /
    "tris_b" given beside them, degenerate faces dropped; for a cloud side the points are the cloud's, faces and soup None), for
    tests."""
    from . import data, hip
    if int(n_samples) != n_samples or n_samples < 1:
        raise ValueError("n_samples must be a positive integer, got %r" % (n_samples,))
    n = int(n_samples)
    thresholds = check_thresholds(thresholds)
    cloud_a, cloud_b = _is_cloud(tris_a), _is_cloud(tris_b)
    if cloud_a or cloud_b:
        return _mixed_metrics(tris_a, tris_b, cloud_a, cloud_b, n, seed, return_samples, thresholds)
    (a, valid_a), (b, valid_b) = _as_soup(tris_a, "tris_a"), _as_soup(tris_b, "tris_b")
    if not a.is_cuda or not b.is_cuda or a.device != b.device:
        raise ValueError("mesh_metrics runs on the HIP kernels: both meshes must live on one GPU")
    dev = a.device
    gen = torch.Generator(device=dev).manual_seed(int(seed))
    with torch.no_grad():
        sides = []
        for soup in (a, b):
            soup, n_kept, sample_faces = drop_degenerate(soup)
            # the cumulative areas in one fixed order (torch.cumsum on the device is not run-to-run reproducible at this size),
            # forced monotone; the tail's faces are degenerate here, so they are never drawn
            corners = soup.reshape(-1, 3)
            cum = torch.cummax(hip.face_area_cumsum(corners[sample_faces]), 0).values
            pts, fi = data.sample_surface(corners, sample_faces, n, generator=gen, cum=cum)
            sides.append((soup, n_kept, pts.contiguous(), fi.to(torch.int32)))
        (sa, ka, pa, fa), (sb, kb, pb, fb) = sides
        index_a, index_b = hip.mesh_index(sa), hip.mesh_index(sb)
        d2_ab, g_ab, _, _ = hip.mesh_closest(index_b, pa, want_closest=False)
        d2_ba, g_ba, _, _ = hip.mesh_closest(index_a, pb, want_closest=False)
        out = hip.surface_metrics(sa, fa, d2_ab, g_ab, sb, fb, d2_ba, g_ba)
        nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
        ok = (ka > 0) & (kb > 0) & valid_a & valid_b
        res = {k: torch.where(ok, out[i], nan) for i, k in enumerate(METRIC_KEYS)}
        if thresholds is not None:
            thr2 = _thr2(thresholds, dev)
            _, within_a = hip.sample_scores(d2_ab, thr2=thr2)
            _, within_b = hip.sample_scores(d2_ba, thr2=thr2)
            _add_fscores(res, thresholds, within_a, n, within_b, n, ok)
    res["n_a"], res["n_b"] = n, n
    if return_samples:
        res["samples"] = {"tris_a": sa, "n_faces_a": ka, "points_a": pa, "face_a": fa, "d2_ab": d2_ab, "closest_face_ab": g_ab,
                          "tris_b": sb, "n_faces_b": kb, "points_b": pb, "face_b": fb, "d2_ba": d2_ba, "closest_face_ba": g_ba}
    return res


def _thr2(thresholds, dev):
    """(T,) float64 device tensor of t t, the product in float64 on the host, written by fill kernels (a copy from the host would
    wait for the stream)."""
    return torch.cat([torch.full((1,), t * t, dtype=torch.float64, device=dev) for t in thresholds])


def _add_fscores(res, thresholds, within_a, n_a, within_b, n_b, ok):
    nan = torch.full_like(within_a, float("nan"), dtype=torch.float64)
    # a tensor divisor: count / n correctly rounded (a Python scalar would be turned into a multiplication by 1 / n)
    p = within_a.double() / torch.full_like(nan, float(n_a))
    r = within_b.double() / torch.full_like(nan, float(n_b))
    res["precision"], res["recall"], res["fscore"] = torch.where(ok, p, nan), torch.where(ok, r, nan), torch.where(ok, fscore(p, r), nan)
    res["thresholds"] = thresholds


def _mixed_metrics(in_a, in_b, cloud_a, cloud_b, n, seed, return_samples, thresholds):
    """mesh_metrics with a cloud on at least one side: hip.sample_scores per direction, the means on the device."""
    from . import data, hip
    sides, dev = [], None
    for x, is_cloud, what in ((in_a, cloud_a, "tris_a"), (in_b, cloud_b, "tris_b")):
        if is_cloud:
            cloud = _as_cloud(x)
            t = cloud.points
            sides.append({"cloud": cloud})
        else:
            t, valid = _as_soup(x, what)
            sides.append({"soup": t, "valid": valid})
        if not t.is_cuda or (dev is not None and t.device != dev):
            raise ValueError("mesh_metrics runs on the HIP kernels: both sides must live on one GPU")
        dev = t.device
    gen = torch.Generator(device=dev).manual_seed(int(seed))
    with torch.no_grad():
        for s in sides:                                            # A's samples first, then B's; a cloud draws nothing
            if "cloud" in s:
                c = s["cloud"]
                s.update(pts=c.points, normals=None if c.normals is None else c.normals.double(), index=hip.point_index(c.points),
                         tris=None, n_kept=None, face=None)
                s["sample_normals"], s["ok"], s["n"] = s["normals"], s["index"].n_bad == 0, len(c)
            else:
                soup, n_kept, sample_faces = drop_degenerate(s["soup"])
                corners = soup.reshape(-1, 3)
                cum = torch.cummax(hip.face_area_cumsum(corners[sample_faces]), 0).values
                pts, fi = data.sample_surface(corners, sample_faces, n, generator=gen, cum=cum)
                normals = _face_normals(soup)
                s.update(pts=pts.contiguous(), normals=normals, index=hip.mesh_index(soup), tris=soup, n_kept=n_kept,
                         face=fi.to(torch.int32), sample_normals=normals[fi.long()], ok=(n_kept > 0) & s["valid"], n=n)
        thr2 = _thr2(thresholds, dev) if thresholds is not None else None
        sums, within, queried = [], [], []
        for x, y in ((sides[0], sides[1]), (sides[1], sides[0])):
            if "cloud" in y:
                d2, g, _ = hip.point_nearest(y["index"], x["pts"])
            else:
                d2, g, _, _ = hip.mesh_closest(y["index"], x["pts"], want_closest=False)
            if x["sample_normals"] is not None and y["normals"] is not None:
                su, wi = hip.sample_scores(d2, x["sample_normals"], y["normals"], g, thr2=thr2)
            else:
                su, wi = hip.sample_scores(d2, thr2=thr2)
            sums.append(su), within.append(wi), queried.append((d2, g))
        (sa, sb), (xa, xb) = sums, sides
        acc, comp = sa[0] / sa[4], sb[0] / sb[4]
        out = {"accuracy": acc, "completeness": comp, "chamfer_l1": 0.5 * (acc + comp),
               "chamfer_l2": 0.5 * (sa[1] / sa[4] + sb[1] / sb[4]), "normal_consistency": 0.5 * (sa[2] / sa[5] + sb[2] / sb[5]),
               "hausdorff_ab": sa[3], "hausdorff_ba": sb[3]}
        nan = torch.full((), float("nan"), dtype=torch.float64, device=dev)
        ok = xa["ok"] & xb["ok"]
        res = {k: torch.where(ok, out[k], nan) for k in METRIC_KEYS}
        if thresholds is not None:
            _add_fscores(res, thresholds, within[0], xa["n"], within[1], xb["n"], ok)
    res["n_a"], res["n_b"] = xa["n"], xb["n"]
    if return_samples:
        res["samples"] = {"tris_a": xa["tris"], "n_faces_a": xa["n_kept"], "points_a": xa["pts"], "face_a": xa["face"],
                          "d2_ab": queried[0][0], "closest_face_ab": queried[0][1],
                          "tris_b": xb["tris"], "n_faces_b": xb["n_kept"], "points_b": xb["pts"], "face_b": xb["face"],
                          "d2_ba": queried[1][0], "closest_face_ba": queried[1][1]}
    return res


# ---- connected components, floater removal -----------------------------------------------------------------------------------
def check_keep(keep):
    """Validate a `keep` / `clean` policy of `clean_mesh` and return it in canonical form: ("largest",), ("referenced",),
    ("faces", k) or ("share", m, e) with the float share = m / 2^e exactly.  ValueError for anything else."""
    import math
    if isinstance(keep, str):
        if keep in ("largest", "referenced"):
            return (keep,)
    elif isinstance(keep, bool):
        pass
    elif isinstance(keep, (int, np.integer)):
        if 0 <= int(keep) <= 2 ** 31 - 1:
            return ("faces", int(keep))
    elif isinstance(keep, (float, np.floating)):
        if math.isfinite(float(keep)) and 0.0 < float(keep) <= 1.0:
            m, q = float(keep).as_integer_ratio()          # q is a power of two, m < 2^53
            return ("share", m, q.bit_length() - 1)
    raise ValueError("keep must be 'largest', 'referenced', an int >= 0 (faces) or a float in (0, 1] (share of the largest "
                     "component's faces), got %r" % (keep,))


def ceil_share(most, m, e):
    """ceil(most m / 2^e) in int64 tensor operations, exactly: most a 0-dim int64 tensor in [0, 2^31), 0 < m < 2^53, m <= 2^e.
    most m can need 84 bits, so m is split at bit 26: most m = (most mh) 2^26 + most ml, both products below 2^58."""
    if e <= 26:                                        # m <= 2^26: the product fits
        return (most * m + ((1 << e) - 1)) >> e
    mh, ml = m >> 26, m & ((1 << 26) - 1)
    low = most * ml
    high = most * mh + (low >> 26)                     # floor(most m / 2^26)
    rest = (low & ((1 << 26) - 1)) != 0                # ... and whether bits were dropped
    s = e - 26
    if s >= 62:                                        # high < 2^59: the quotient is below 1
        return ((high != 0) | rest).long()
    return (high >> s) + (((high & ((1 << s) - 1)) != 0) | rest).long()


def keep_components(policy, comp_faces, counts):
    """The policy of `check_keep` as a few elementwise operations on the device: comp_faces (V,) and counts (3,) of
    mesh_components -> keep (V,) int32 indexed by component id (entries beyond the component count are never looked at).

        ("largest",)      the component with the most faces (ties: the lowest id)
        ("faces", k)      every component with at least k faces
        ("share", m, e)   every component with at least ceil(share largest) faces, share = m / 2^e being the float exactly; the
                          threshold is computed in integers (ceil_share)
        ("referenced",)   every component with a face: only the vertices no valid face names go"""
    V = comp_faces.shape[0]
    if policy[0] == "largest":
        keep = torch.arange(V, device=comp_faces.device) == counts[2]
    elif policy[0] == "faces":
        keep = comp_faces >= policy[1]
    elif policy[0] == "share":
        most = comp_faces.max().long() if V else torch.zeros((), dtype=torch.int64, device=comp_faces.device)
        keep = comp_faces.long() >= ceil_share(most, policy[1], policy[2])
    else:
        keep = comp_faces > 0
    return keep.to(torch.int32)


def _mesh_args(verts_or_n_verts, faces, what):
    if isinstance(verts_or_n_verts, torch.Tensor) and verts_or_n_verts.dim() > 0:
        if verts_or_n_verts.dim() != 2 or verts_or_n_verts.shape[1] != 3:
            raise ValueError("%s: verts must be (V, 3), got %s" % (what, tuple(verts_or_n_verts.shape)))
        n_verts = int(verts_or_n_verts.shape[0])
    else:
        n_verts = verts_or_n_verts
        if isinstance(n_verts, (bool, float)) or isinstance(n_verts, torch.Tensor) or int(n_verts) != n_verts or int(n_verts) < 0:
            raise ValueError("%s: the vertex count must be an integer >= 0 or verts (V, 3), got %r" % (what, n_verts))
        n_verts = int(n_verts)
    if not isinstance(faces, torch.Tensor):
        raise ValueError("%s: faces must be an (F, 3) tensor" % what)
    return n_verts, faces      # shape and dtype of the faces: the backend's own checks


def _check_mesh_verts(verts, faces, what):
    """The vertices of a mesh whose faces _mesh_args has checked: a floating-point (V, 3) tensor on the faces' device."""
    if not isinstance(verts, torch.Tensor) or verts.dim() != 2 or not verts.dtype.is_floating_point:
        raise ValueError("%s: verts must be a floating-point (V, 3) tensor" % what)
    if verts.device != faces.device:
        raise ValueError("%s: verts live on %s, faces on %s" % (what, verts.device, faces.device))


def _cc_backend(faces):
    """The two kernels for a mesh on the GPU, their tensor specification for one on the host."""
    if faces.is_cuda:
        from . import hip
        return hip
    from . import meshing
    return meshing


def mesh_components(verts_or_n_verts, faces):
    """Connected components of an indexed mesh by shared vertex ids (hip.mesh_components on the GPU, meshing.mesh_components on the
    host): faces (F,3) integer ids, and the vertices (V,3) or just their number.  A face with an id out of range is skipped, a
    vertex no valid face names is a component of its own.  -> dict of labels (V,) int32 component of every vertex, n_components C,
    comp_verts / comp_faces (C,) int32 sizes, n_valid_faces and largest (the component with the most faces, ties to the lowest id;
    -1 for an empty mesh).  Components are numbered in ascending order of their smallest vertex id.  One host synchronisation
    (the counts)."""
    n_verts, faces = _mesh_args(verts_or_n_verts, faces, "mesh_components")
    labels, comp_verts, comp_faces, counts = _cc_backend(faces).mesh_components(faces, n_verts)
    C, n_valid, largest = counts.tolist()
    return {"labels": labels, "n_components": C, "comp_verts": comp_verts[:C], "comp_faces": comp_faces[:C],
            "n_valid_faces": n_valid, "largest": largest}


def clean_mesh(verts, faces, keep="largest", attributes=None):
    """Drop floaters: the indexed mesh (verts (V,3), faces (F,3) integer ids) restricted to the connected components `keep` names,
    vertices and faces in their original order.

        keep = "largest"      the component with the most faces (ties: the lowest-numbered one)
               int k          every component with at least k faces
               float in (0,1] every component with at least ceil(share largest) faces, largest being the largest component's
               "referenced"   every component with a face: only unreferenced vertices go

    Faces with an id out of range are dropped whatever `keep` says.  -> dict of verts (V',3), faces (F',3) in the dtype of
    `faces`, n_verts, n_tris, vert_src (V',) int64 (the old id of every new vertex: verts_out = verts[vert_src]), removed = dict
    of the components / vertices / faces dropped, and every tensor of the dict `attributes` (first dimension V) gathered by
    vert_src.  On the GPU the labelling and the compaction are arah_mesh_components / arah_mesh_select, the policy a few
    elementwise operations between them, and ONE host synchronisation reads the kept sizes; on the host the same through their
    tensor specification."""
    policy = check_keep(keep)
    n_verts, faces = _mesh_args(verts, faces, "clean_mesh")
    if not isinstance(verts, torch.Tensor) or verts.dim() != 2:
        raise ValueError("clean_mesh: verts must be a (V, 3) tensor")
    if verts.device != faces.device:
        raise ValueError("clean_mesh: verts live on %s, faces on %s" % (verts.device, faces.device))
    attributes = dict(attributes or {})
    reserved = ("verts", "faces", "n_verts", "n_tris", "vert_src", "removed")
    for name, t in attributes.items():
        if name in reserved:
            raise ValueError("clean_mesh: an attribute cannot be called %r" % (name,))
        if not isinstance(t, torch.Tensor) or t.dim() < 1 or t.shape[0] != n_verts or t.device != verts.device:
            raise ValueError("clean_mesh: attribute %r must be a tensor with %d rows on %s" % (name, n_verts, verts.device))
    backend = _cc_backend(faces)
    with torch.no_grad():
        labels, _, comp_faces, counts = backend.mesh_components(faces, n_verts)
        keep_c = keep_components(policy, comp_faces, counts)
        vert_src, _, faces_out, _, kept = backend.mesh_select(faces, n_verts, labels, keep_c)
        in_use = torch.arange(n_verts, device=faces.device) < counts[0]
        kept_comps = (keep_c.bool() & in_use).sum().to(torch.int32).reshape(1)
        nv, nf, C, nc = torch.cat([kept, counts[:1], kept_comps]).tolist()      # the host synchronisation
        vert_src = vert_src[:nv].long()
        res = {"verts": verts.index_select(0, vert_src), "faces": faces_out[:nf].to(faces.dtype), "n_verts": nv, "n_tris": nf,
               "vert_src": vert_src,
               "removed": {"components": C - nc, "vertices": n_verts - nv, "faces": int(faces.shape[0]) - nf}}
        for name, t in attributes.items():
            res[name] = t.index_select(0, vert_src)
    return res


# ---- simplification by vertex clustering ------------------------------------------------------------------------------------------
_SIMPLIFY_KEYS = ("cell", "resolution", "bounds", "position", "dedup", "drop_unreferenced", "quadric_reg", "target_faces")
SIMPLIFY_TARGET_MAX_RESOLUTION = 400     # the face-count search ends here: 401^3 cells stay below the grid's 2^27


def check_simplify(simplify):
    """Validate a `simplify` option of the model's mesh entries and return the keywords of `simplify_mesh` it stands for: a cell
    length (a number > 0), or a dict of cell / resolution / target_faces (exactly one of the three) / bounds / position /
    quadric_reg / dedup / drop_unreferenced.  A dict with "method": "collapse" stands for `decimate_mesh` instead: target_faces /
    ratio / max_error / quadric_reg / max_rounds, and comes back with its "method" (`apply_simplify` routes it); "method": "cluster"
    is the dict without it.  ValueError for anything else."""
    import math
    if isinstance(simplify, dict) and "method" in simplify:
        kw = dict(simplify)
        method = kw.pop("method")
        if method == "collapse":
            bad = set(kw) - set(_DECIMATE_KEYS)
            if bad:
                raise ValueError("simplify: unknown keys %s for method 'collapse' (known: %s)"
                                 % (sorted(bad, key=str), ", ".join(_DECIMATE_KEYS)))
            check_decimate(**kw)
            return dict(kw, method="collapse")
        if method != "cluster":
            raise ValueError("simplify: method must be 'cluster' or 'collapse', got %r" % (method,))
        return check_simplify(kw)
    if isinstance(simplify, dict):
        kw = dict(simplify)
        bad = set(kw) - set(_SIMPLIFY_KEYS)
        if bad:
            raise ValueError("simplify: unknown keys %s (known: %s)" % (sorted(bad, key=str), ", ".join(_SIMPLIFY_KEYS)))
    elif isinstance(simplify, (int, float, np.integer, np.floating)) and not isinstance(simplify, bool):
        kw = {"cell": float(simplify)}
    else:
        raise ValueError("simplify must be a cell length or a dict of simplify_mesh keywords, got %r" % (simplify,))
    cell, resolution, target = kw.get("cell"), kw.get("resolution"), kw.get("target_faces")
    if (cell is not None) + (resolution is not None) + (target is not None) != 1:
        raise ValueError("simplify: exactly one of cell, resolution and target_faces is given, got cell=%r resolution=%r "
                         "target_faces=%r" % (cell, resolution, target))
    if cell is not None and (isinstance(cell, bool) or not isinstance(cell, (int, float, np.integer, np.floating))
                             or not math.isfinite(float(cell)) or not float(cell) > 0.0):
        raise ValueError("simplify: cell must be a finite length > 0, got %r" % (cell,))
    if resolution is not None and (isinstance(resolution, bool) or not isinstance(resolution, (int, np.integer)) or int(resolution) < 1):
        raise ValueError("simplify: resolution must be an integer >= 1, got %r" % (resolution,))
    if target is not None and (isinstance(target, bool) or not isinstance(target, (int, np.integer)) or int(target) < 1):
        raise ValueError("simplify: target_faces must be an integer >= 1, got %r" % (target,))
    if kw.get("position", "mean") not in ("mean", "member", "quadric"):
        raise ValueError("simplify: position must be 'mean', 'member' or 'quadric', got %r" % (kw["position"],))
    reg = kw.get("quadric_reg", 1e-3)
    if (isinstance(reg, bool) or not isinstance(reg, (int, float, np.integer, np.floating)) or not math.isfinite(float(reg))
            or float(reg) < 0.0):
        raise ValueError("simplify: quadric_reg must be a finite number >= 0, got %r" % (reg,))
    return kw


def simplify_grid_of(lo, hi, cell):
    """The grid rule of `simplify_mesh`, in float32: origin = floor(lo / cell) cell, dims = floor((hi - origin) / cell) + 1.
    -> (origin (3,) float32 array, dims list of ints).  ValueError when the quotients are not finite (a cell so small that they
    overflow float32): such bounds and cell make no grid."""
    lo, hi, c = np.asarray(lo, np.float32), np.asarray(hi, np.float32), np.float32(cell)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        origin = (np.floor(lo / c) * c).astype(np.float32)
        dims = np.floor((hi - origin) / c).astype(np.float64) + 1.0
    if not np.isfinite(origin).all() or not np.isfinite(dims).all():
        raise ValueError("simplify_mesh: the bounds %r .. %r with cell %r make no grid" % (lo.tolist(), hi.tolist(), float(c)))
    return origin, [int(x) for x in dims]


def simplify_mesh(verts, faces, cell=None, resolution=None, bounds=None, position="mean", dedup=True, attributes=None,
                  drop_unreferenced=True, quadric_reg=1e-3, target_faces=None):
    """Simplify an indexed mesh (verts (V,3), faces (F,3) integer ids) by vertex clustering: the vertices inside one cell of a
    regular grid become one vertex, faces are renamed to cells, and the faces that collapse (two corners in one cell) or repeat
    (dedup: the same three cells as an earlier face, in any orientation) go.  Decimation and welding by position in one step.

        cell          the side of a cell, a length in the units of verts; or
        resolution    the number of cells along the longest side of the bounds; or
        target_faces  a face count N (exactly one of the three is given): the largest resolution r in [1, 400] that
                      `search_resolution` finds with at most N kept faces -- up to eleven clusterings, each with one host
                      synchronisation; the result gains resolution, probes (the (r, faces) asked) and reached (False when even
                      r = 1 keeps more than N)
        bounds        (lo, hi), three numbers each; default: the box of the vertices with finite coordinates
        position      "mean": a cluster sits at the exact mean of its members; "member": at the member nearest to that mean -- a
                      subset of the input, still on the extracted level set; "quadric": at the minimiser of the plane quadric
                      of the faces that touch it (mesh_quadric_place: arah_mesh_quadric_place on the GPU, its specification on
                      the host), regularised towards the mean by quadric_reg and never further than a cell from it -- a mean of
                      points on a convex surface lies inside it, the minimiser keeps the volume; the result gains quadric =
                      dict of fallbacks (clusters left at their mean) and longest (the most faces at one cluster), and
                      vert_src names the member nearest to the NEW position.  ValueError when a cluster has more than 2^15
                      faces: choose a smaller cell or position='mean'
        drop_unreferenced   clusters that lost all their faces are removed (mesh_select with the "referenced" policy of clean_mesh)

    The grid, in float32: origin = floor(lo / cell) cell, dims = floor((hi - origin) / cell) + 1; at most 2^27 cells.  A vertex
    outside the bounds counts for the nearest cell; a vertex with a non-finite coordinate is invalid and takes its faces along.
    -> dict of verts (V',3) float32, faces (F',3) in the dtype of `faces`, n_verts, n_tris, vert_src (V',) int64 (the member
    that represents every new vertex, in the input's ids), removed = dict of vertices / faces_collapsed / faces_duplicate /
    faces_invalid, cell (float), dims (tuple), and every tensor of the dict `attributes` (first dimension V) gathered by vert_src
    -- never averaged.  On the GPU the clustering is arah_mesh_simplify and the removal arah_mesh_select; on the host their
    tensor specifications.  Every decision is an integer's: the result does not depend on the order in which the device's
    threads arrive, and the host's and the device's are equal bit for bit; the numbering of the vertices matters through the tie
    rule alone (of members equally near the mean the lowest id represents the cluster, so "member" positions can differ there).  Host synchronisations: ONE (the sizes of the result), and one more
    when `bounds` is left to the vertices' box.  ValueError when dedup meets more than 2^21 clusters: choose a larger cell, or
    dedup=False."""
    check_simplify({"cell": cell, "resolution": resolution, "position": position, "quadric_reg": quadric_reg,
                    "target_faces": target_faces})
    n_verts, faces = _mesh_args(verts, faces, "simplify_mesh")
    _check_mesh_verts(verts, faces, "simplify_mesh")
    attributes = dict(attributes or {})
    reserved = ("verts", "faces", "n_verts", "n_tris", "vert_src", "removed", "cell", "dims")
    reserved += ("quadric",) if position == "quadric" else ()                  # the keys a mode adds are reserved in that mode
    reserved += ("resolution", "probes", "reached") if target_faces is not None else ()
    for name, t in attributes.items():
        if name in reserved:
            raise ValueError("simplify_mesh: an attribute cannot be called %r" % (name,))
        if not isinstance(t, torch.Tensor) or t.dim() < 1 or t.shape[0] != n_verts or t.device != verts.device:
            raise ValueError("simplify_mesh: attribute %r must be a tensor with %d rows on %s" % (name, n_verts, verts.device))
    backend, dev = _cc_backend(faces), verts.device
    with torch.no_grad():
        v32 = verts.detach().to(torch.float32).contiguous()
        if bounds is None:
            finite = torch.isfinite(v32).all(1, keepdim=True)
            inf = torch.full_like(v32, float("inf"))
            box = torch.stack([torch.where(finite, v32, inf).amin(0), torch.where(finite, v32, -inf).amax(0)]) if n_verts else None
            lo, hi = box.tolist() if n_verts else ([0.0] * 3, [0.0] * 3)      # a host synchronisation
            if lo[0] > hi[0]:                                                     # no finite vertex
                lo, hi = [0.0] * 3, [0.0] * 3
        else:
            try:
                lo, hi = ([float(x) for x in (b.tolist() if isinstance(b, torch.Tensor) else b)] for b in bounds)
            except (TypeError, ValueError):
                raise ValueError("simplify_mesh: bounds must be (lo, hi), three numbers each, got %r" % (bounds,))
            if len(lo) != 3 or len(hi) != 3 or not all(np.isfinite(lo + hi)) or any(h < l for l, h in zip(lo, hi)):
                raise ValueError("simplify_mesh: bounds must be finite with lo <= hi, got %r" % (bounds,))
        lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)

        def cell_of(resolution):
            side = np.float32((hi - lo).max())
            return float(side / np.float32(int(resolution))) if side > 0 else 1.0      # a mesh without extent: one cell

        def grid_of(cell):
            cell = float(np.float32(cell))
            if not np.isfinite(lo).all() or not np.isfinite(hi).all() or not cell > 0.0:
                raise ValueError("simplify_mesh: the bounds %r .. %r with cell %r make no grid" % (lo.tolist(), hi.tolist(), cell))
            origin, dims = simplify_grid_of(lo, hi, cell)
            return cell, origin, dims

        found = None
        if target_faces is not None:
            def kept_faces(r):
                c, o, d = grid_of(cell_of(r))
                sizes = backend.mesh_simplify(v32, faces, o.tolist(), c, d, position="mean", dedup=dedup)[5].tolist()   # a host synchronisation
                return sizes[1], bool(sizes[5])
            resolution, probes, reached = search_resolution(kept_faces, int(target_faces))
            found = {"resolution": resolution, "probes": probes, "reached": reached}
        if cell is None:
            cell = cell_of(resolution)
        cell, origin, dims = grid_of(cell)
        quadric = position == "quadric"
        verts_out, vert_src, vert_map, faces_out, _, counts = backend.mesh_simplify(v32, faces, origin.tolist(), cell, dims,
                                                                                    position="mean" if quadric else position,
                                                                                    dedup=dedup)
        if quadric:
            verts_out, vert_src, qcounts = backend.mesh_quadric_place(v32, faces, vert_map, verts_out, counts, cell, float(quadric_reg))
        else:
            qcounts = counts[:0]                                                 # its sizes are read with the others
        F = int(faces.shape[0])
        if drop_unreferenced:
            # the guard rows of faces_out name vertex 0: they become invalid faces; a vertex is its own component here, kept
            # when a kept face names it -- so every kept face stays
            live = torch.arange(F, device=dev)[:, None] < counts[1]
            named = torch.where(live, faces_out, torch.full_like(faces_out, -1))
            keep = torch.zeros(n_verts + 1, dtype=torch.int32, device=dev)
            keep[(named.reshape(-1) + 1).long()] = 1
            own = torch.arange(n_verts, dtype=torch.int32, device=dev)
            sel_src, _, faces_out, _, kept = backend.mesh_select(named, n_verts, own, keep[1:].contiguous())
            sizes = torch.cat([counts, kept, qcounts]).tolist()                  # the host synchronisation
            nv, nf = sizes[6:8]
            pick = sel_src[:nv].long()
            verts_out, vert_src = verts_out.index_select(0, pick), vert_src.long().index_select(0, pick)
        else:
            sizes = torch.cat([counts, counts[:2], qcounts]).tolist()            # the host synchronisation
            nv, nf = sizes[:2]
            verts_out, vert_src = verts_out[:nv], vert_src[:nv].long()
        if sizes[5]:
            raise ValueError("simplify_mesh: dedup holds three 21-bit cluster ids in a face's key, and this grid has %d occupied "
                             "cells; choose a larger cell or dedup=False" % sizes[0])
        res = {"verts": verts_out, "faces": faces_out[:nf].to(faces.dtype), "n_verts": nv, "n_tris": nf, "vert_src": vert_src,
               "removed": {"vertices": n_verts - nv, "faces_collapsed": sizes[3], "faces_duplicate": sizes[4],
                           "faces_invalid": sizes[2]},
               "cell": cell, "dims": tuple(dims)}
        if quadric:
            if sizes[11] == 2:
                raise ValueError("simplify_mesh: a cell holds more than 2^15 faces (%d), too many to place by their quadric; "
                                 "choose a smaller cell or position='mean'" % sizes[10])
            res["quadric"] = {"fallbacks": sizes[8], "longest": sizes[10]}
        if found is not None:
            res.update(found)
        for name, t in attributes.items():
            res[name] = t.index_select(0, vert_src)
    return res


def search_resolution(kept_faces, target, r_max=SIMPLIFY_TARGET_MAX_RESOLUTION):
    """The face-count search of `simplify_mesh(target_faces=N)` over the integer resolution r in [1, r_max].  kept_faces(r) ->
    (the faces the clustering keeps on r's grid, its status); count(r) is that number, and a probe with a status counts as
    above N.  count(1) > N: r = 1, not reached.  count(r_max) <= N: r = r_max.  Otherwise bisect with count(lo) <= N < count(hi),
    mid = (lo + hi) // 2, until hi - lo = 1: r = lo.  -> (r, probes = the list of (r, count) in the order asked, reached)."""
    probes = []

    def above(r):
        n, status = kept_faces(r)
        probes.append((r, n))
        return bool(status) or n > target

    if above(1):
        return 1, probes, False
    if not above(r_max):
        return r_max, probes, True
    lo, hi = 1, r_max
    while hi - lo > 1:              # terminates: lo < mid < hi, so hi - lo strictly decreases
        mid = (lo + hi) // 2
        if above(mid):
            hi = mid
        else:
            lo = mid
    return lo, probes, True


# ---- decimation by edge collapse ----------------------------------------------------------------------------------------------------
_DECIMATE_KEYS = ("target_faces", "ratio", "max_error", "quadric_reg", "max_rounds")
_DECIMATE_SUMS = ("pinned", "link", "long_edges", "nonfinite", "over_error", "flips", "fallbacks")


def check_decimate(target_faces=None, ratio=None, max_error=None, quadric_reg=1e-3, max_rounds=200):
    """Validate the scalars of `decimate_mesh`; ValueError for anything else.  At most one of target_faces (an integer >= 0) and
    ratio (in [0, 1]) is given, and at least one of them and max_error (a number >= 0)."""
    import math

    def number(x):
        return isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, bool) and not math.isnan(float(x))
    if target_faces is not None and ratio is not None:
        raise ValueError("decimate_mesh: at most one of target_faces and ratio is given, got %r and %r" % (target_faces, ratio))
    if target_faces is None and ratio is None and max_error is None:
        raise ValueError("decimate_mesh: one of target_faces, ratio and max_error is needed")
    if target_faces is not None and (isinstance(target_faces, bool) or not isinstance(target_faces, (int, np.integer))
                                     or int(target_faces) < 0):
        raise ValueError("decimate_mesh: target_faces must be an integer >= 0, got %r" % (target_faces,))
    if ratio is not None and (not number(ratio) or not 0.0 <= float(ratio) <= 1.0):
        raise ValueError("decimate_mesh: ratio must lie in [0, 1], got %r" % (ratio,))
    if max_error is not None and (not number(max_error) or float(max_error) < 0.0):
        raise ValueError("decimate_mesh: max_error must be a number >= 0, got %r" % (max_error,))
    if not number(quadric_reg) or not math.isfinite(float(quadric_reg)) or float(quadric_reg) < 0.0:
        raise ValueError("decimate_mesh: quadric_reg must be a finite number >= 0, got %r" % (quadric_reg,))
    if isinstance(max_rounds, bool) or not isinstance(max_rounds, (int, np.integer)) or int(max_rounds) < 0:
        raise ValueError("decimate_mesh: max_rounds must be an integer >= 0, got %r" % (max_rounds,))


def decimate_mesh(verts, faces, target_faces=None, ratio=None, max_error=None, quadric_reg=1e-3, max_rounds=200, attributes=None):
    """Decimate an indexed mesh (verts (V,3), faces (F,3) integer ids) by edge collapse: rounds of `mesh_collapse_round`
    (arah_mesh_collapse_round on the GPU, meshing.mesh_collapse_round on the host, equal bit for bit).  Unlike `simplify_mesh` the
    surface stays a surface: an edge collapses only between two vertices interior to a consistently oriented manifold
    neighbourhood, under the link condition, and when no face around it turns over -- a closed embedded mesh stays manifold and
    watertight with its Euler characteristic and its components, and faces go where the surface is flat.

        target_faces  the face count to reach; or
        ratio         the share of the input's faces to reach: target = floor(ratio F)
        max_error     the largest cost of an edge that may collapse: the quadric's value at the new vertex, the sum over the
                      faces around the edge of (2 area x distance of the vertex to the face's plane)^2 -- a length to the SIXTH
                      power, not a distance; alone it decimates as far as that bound allows
        quadric_reg   the regulariser of the position solve, as in simplify_mesh(position="quadric")
        max_rounds    the most rounds

    A round collapses at most need = ceil((F - target) / 2) independent edges, two faces each, so the count ends at the target, or
    one below it when F - target is odd; the last round takes the first `need` selected edges in ascending id, not the cheapest.
    The loop ends when F <= target, when a round selects no edge (every remaining one is pinned, fails the link or flip test,
    is surrounded by more than 32 faces or costs more than max_error), or after max_rounds.  Boundary vertices and vertices on
    non-manifold or misoriented edges never move and never merge.  ONE host synchronisation per round (its counts).

    -> dict of verts (V',3) float32, faces (F',3) in the dtype of `faces`, n_verts, n_tris, vert_src (V',) int64 (the input
    vertex nearest to every output vertex among those it absorbed in its last collapse), face_src (F',) int64 (every output face
    is that input face, renamed), every tensor of the dict `attributes` (first dimension V) gathered by vert_src -- never averaged
    -- and report = dict of target, rounds, reached, faces (the count before every round and at the end) and the rounds' summed
    counts pinned, link, long_edges, nonfinite, over_error, flips (edges that were no candidates, by their first reason) and
    fallbacks (position solves that fell back to the midpoint)."""
    import math
    check_decimate(target_faces, ratio, max_error, quadric_reg, max_rounds)
    n_verts, faces = _mesh_args(verts, faces, "decimate_mesh")
    _check_mesh_verts(verts, faces, "decimate_mesh")
    attributes = dict(attributes or {})
    reserved = ("verts", "faces", "n_verts", "n_tris", "vert_src", "face_src", "report")
    for name, t in attributes.items():
        if name in reserved:
            raise ValueError("decimate_mesh: an attribute cannot be called %r" % (name,))
        if not isinstance(t, torch.Tensor) or t.dim() < 1 or t.shape[0] != n_verts or t.device != verts.device:
            raise ValueError("decimate_mesh: attribute %r must be a tensor with %d rows on %s" % (name, n_verts, verts.device))
    backend, dev = _cc_backend(faces), verts.device
    from . import meshing
    names = meshing.COLLAPSE_COUNTS
    n_faces = int(faces.shape[0])
    target = int(target_faces) if target_faces is not None else int(math.floor(float(ratio) * n_faces)) if ratio is not None else 0
    max_cost = float("inf") if max_error is None else float(max_error)
    with torch.no_grad():
        v, f = verts.detach().to(torch.float32).contiguous(), faces
        vert_src, face_src = torch.arange(n_verts, device=dev), torch.arange(n_faces, device=dev)
        history, sums, rounds = [n_faces], dict.fromkeys(_DECIMATE_SUMS, 0), 0
        while rounds < int(max_rounds) and history[-1] > target:
            need = (history[-1] - target + 1) // 2
            out = backend.mesh_collapse_round(v, f, need, float(quadric_reg), max_cost)
            c = dict(zip(names, out[4].tolist()))                                 # the host synchronisation
            rounds += 1
            for k in _DECIMATE_SUMS:
                sums[k] += c[k]
            if c["applied"] == 0:
                break
            nv, nf = c["n_verts"], c["n_faces"]
            v, f = out[0][:nv], out[1][:nf]
            vert_src, face_src = vert_src[out[2][:nv].long()], face_src[out[3][:nf].long()]
            history.append(nf)
        res = {"verts": v, "faces": f.to(faces.dtype), "n_verts": int(v.shape[0]), "n_tris": int(f.shape[0]), "vert_src": vert_src,
               "face_src": face_src,
               "report": dict(sums, target=target, rounds=rounds, reached=history[-1] <= target, faces=history)}
        for name, t in attributes.items():
            res[name] = t.index_select(0, vert_src)
    return res


def apply_simplify(verts, faces, simplify):
    """The mesh entries' `simplify` option, as `check_simplify` returned it: `decimate_mesh` for method="collapse",
    `simplify_mesh` otherwise."""
    if simplify.get("method") == "collapse":
        return decimate_mesh(verts, faces, **{k: x for k, x in simplify.items() if k != "method"})
    return simplify_mesh(verts, faces, **simplify)


# ---- subdivision ----------------------------------------------------------------------------------------------------------------------
_SUBDIVIDE_KEYS = ("levels", "method", "max_edge", "max_rounds", "max_faces")


def check_subdivide(subdivide):
    """The mesh entries' `subdivide` option, validated: None stays None, an integer is a number of uniform midpoint levels, a dict
    holds keywords of `subdivide_mesh` (levels, method, max_edge, max_rounds, max_faces).  -> the dict of keywords; ValueError for
    anything else."""
    import math
    if subdivide is None:
        return None
    if isinstance(subdivide, (int, np.integer)) and not isinstance(subdivide, bool):
        subdivide = {"levels": int(subdivide)}
    if not isinstance(subdivide, dict):
        raise ValueError("subdivide must be None, a number of levels or a dict of subdivide_mesh keywords, got %r" % (subdivide,))
    bad = set(subdivide) - set(_SUBDIVIDE_KEYS)
    if bad:
        raise ValueError("subdivide: unknown keys %s (known: %s)" % (sorted(bad), ", ".join(_SUBDIVIDE_KEYS)))
    kw = dict(subdivide)
    levels, method, max_edge = kw.get("levels", 1), kw.get("method", "midpoint"), kw.get("max_edge")
    if isinstance(levels, bool) or not isinstance(levels, (int, np.integer)) or int(levels) < 0:
        raise ValueError("subdivide_mesh: levels must be an integer >= 0, got %r" % (levels,))
    if method not in ("midpoint", "loop"):
        raise ValueError("subdivide_mesh: method must be 'midpoint' or 'loop', got %r" % (method,))
    if max_edge is not None:
        if isinstance(max_edge, bool) or not isinstance(max_edge, (int, float, np.integer, np.floating)) \
                or not math.isfinite(float(max_edge)) or float(max_edge) <= 0.0:
            raise ValueError("subdivide_mesh: max_edge must be a finite length > 0, got %r" % (max_edge,))
        if method == "loop":
            raise ValueError("subdivide_mesh: method='loop' refines every edge: it takes no max_edge")
    for name in ("max_rounds", "max_faces"):
        x = kw.get(name, 0)
        if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or int(x) < 0:
            raise ValueError("subdivide_mesh: %s must be an integer >= 0, got %r" % (name, x))
    return kw


def _weights_step(rows, cols, vals, n_rows, n_cols, lo, hi):
    """The (n_rows x n_cols) weights as sorted COO triples with rows lo and hi averaged appended: -> the triples of the taller matrix."""
    from . import meshing
    cnt = torch.bincount(rows, minlength=n_rows)
    start = torch.cumsum(cnt, 0) - cnt
    parts = [(rows, cols, vals)]
    for ids in (lo, hi):
        k, r = meshing._ragged(start[ids], cnt[ids])
        parts.append((n_rows + k, cols[r], vals[r] * 0.5))
    idx = torch.stack([torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])])
    w = torch.sparse_coo_tensor(idx, torch.cat([p[2] for p in parts]), (n_rows + int(lo.shape[0]), n_cols)).coalesce()
    return w.indices()[0], w.indices()[1], w.values()


def subdivide_mesh(verts, faces, levels=1, method="midpoint", max_edge=None, max_rounds=16, max_faces=1 << 24, attributes=None):
    """Refine an indexed mesh (verts (V,3), faces (F,3) integer ids): rounds of `mesh_subdivide_round` (arah_mesh_subdivide_round on
    the GPU, meshing.mesh_subdivide_round on the host, equal bit for bit).  Old vertices keep their ids, new ones follow; faces
    keep their orientation and their order; marks belong to edges, so a closed manifold mesh stays closed and manifold.

        levels      without max_edge: the number of uniform rounds -- every edge is split, every face becomes four
        method      "midpoint": new vertices at the midpoints, old ones stay -- the surface does not move; "loop": Loop's scheme
                    with Warren's weights -- old vertices move too, a coarse cage converges to a smooth limit surface; boundary,
                    non-manifold and misoriented edges and non-finite vertices fall back to the midpoint
        max_edge    midpoint only, levels is ignored: rounds that split only the edges longer than max_edge (squared length >
                    float(max_edge)^2) until a round marks nothing (report["reached"]) or max_rounds rounds have run
        max_faces   a ValueError before a round whose worst case, four times its faces, exceeds it -- for uniform rounds before
                    the first one runs

    ONE host synchronisation per round (its counts).  -> dict of verts (V',3) float32, faces (F',3) in the dtype of `faces`,
    n_verts, n_tris, vert_src (V',2) int64 -- (v, v) for an input vertex and (lo, hi), the ends of the edge it split, for a new
    one, as ids of the OUTPUT (an id below V is an input vertex: following the pairs ends there) --, vert_weights, the same
    composed down to the input: a sparse COO float64 (V' x V) matrix whose row is the midpoint rule's weights over the input
    vertices (after two rounds up to four of them; vert_weights @ verts is the midpoint position before rounding), face_src (F',)
    int64 (the input face every output face lies in), and report = dict of rounds, reached, verts / faces / marked (per round; the
    first two start with the input's) and counts (the last round's, by meshing.SUBDIVIDE_COUNTS).  attributes = {name: (V, ...)
    tensor}: pushed through the midpoint rule round by round whatever the method -- a new vertex gets ((A_lo + A_hi) 0.5) in
    float64 rounded to the attribute's dtype when that is floating, A_lo otherwise; old vertices keep theirs."""
    from . import meshing
    kw = check_subdivide({"levels": levels, "method": method, "max_edge": max_edge, "max_rounds": max_rounds, "max_faces": max_faces})
    n_verts, faces = _mesh_args(verts, faces, "subdivide_mesh")
    _check_mesh_verts(verts, faces, "subdivide_mesh")
    reserved = ("verts", "faces", "n_verts", "n_tris", "vert_src", "vert_weights", "face_src", "report")
    attributes = _repair_attributes(attributes, n_verts, verts.device, reserved, "subdivide_mesh")
    backend, dev, names = _cc_backend(faces), verts.device, meshing.SUBDIVIDE_COUNTS
    n_faces, max_faces = int(faces.shape[0]), int(kw["max_faces"])
    adaptive = max_edge is not None
    max_len2 = float(max_edge) ** 2 if adaptive else None
    n_rounds = int(max_rounds) if adaptive else int(levels)
    if not adaptive and n_rounds > 0 and n_faces * 4 ** n_rounds > max_faces:
        raise ValueError("subdivide_mesh: %d levels of %d faces give up to %d faces, more than max_faces = %d"
                         % (n_rounds, n_faces, n_faces * 4 ** n_rounds, max_faces))
    with torch.no_grad():
        v, f = verts.detach().to(torch.float32).contiguous(), faces
        ids = torch.arange(n_verts, device=dev)
        vert_src, face_src = torch.stack([ids, ids], 1), torch.arange(n_faces, device=dev)
        w_rows, w_cols, w_vals = ids, ids, torch.ones(n_verts, dtype=torch.float64, device=dev)
        attrs = dict(attributes)
        hist_v, hist_f, hist_m, last, rounds, reached = [n_verts], [n_faces], [], None, 0, not adaptive
        while rounds < n_rounds:
            if 4 * hist_f[-1] > max_faces:
                raise ValueError("subdivide_mesh: a round of %d faces gives up to %d faces, more than max_faces = %d"
                                 % (hist_f[-1], 4 * hist_f[-1], max_faces))
            out = backend.mesh_subdivide_round(v, f, method, max_len2)
            last = dict(zip(names, out[4].tolist()))                              # the host synchronisation
            rounds += 1
            hist_m.append(last["marked"])
            if adaptive and last["marked"] == 0:
                reached = True
                break
            nv, nf, n_old = last["n_verts"], last["n_faces"], hist_v[-1]
            v, f = out[0][:nv], out[1][:nf]
            src = out[2][n_old:nv].long()
            lo, hi = src[:, 0], src[:, 1]
            vert_src, face_src = torch.cat([vert_src, src]), face_src[out[3][:nf].long()]
            w_rows, w_cols, w_vals = _weights_step(w_rows, w_cols, w_vals, n_old, n_verts, lo, hi)
            for name, t in attrs.items():
                new = ((t[lo].double() + t[hi].double()) * 0.5).to(t.dtype) if t.dtype.is_floating_point else t[lo]
                attrs[name] = torch.cat([t, new])
            hist_v.append(nv)
            hist_f.append(nf)
        weights = torch.sparse_coo_tensor(torch.stack([w_rows, w_cols]), w_vals, (hist_v[-1], n_verts)).coalesce()
        res = {"verts": v, "faces": f.to(faces.dtype), "n_verts": int(v.shape[0]), "n_tris": int(f.shape[0]), "vert_src": vert_src,
               "vert_weights": weights, "face_src": face_src,
               "report": {"rounds": rounds, "reached": reached, "verts": hist_v, "faces": hist_f, "marked": hist_m, "counts": last}}
        res.update(attrs)
    return res


def apply_subdivide(verts, faces, subdivide):
    """The mesh entries' `subdivide` option, as `check_subdivide` returned it: -> the refined verts, faces, n_verts and n_tris of
    `subdivide_mesh`, and under "subdivide" its vert_src, vert_weights, face_src and report -- the entries' own vert_src and
    report (clean's, simplify's) stay what they are."""
    res = subdivide_mesh(verts, faces, **subdivide)
    out = {k: res[k] for k in ("verts", "faces", "n_verts", "n_tris")}
    out["subdivide"] = {k: res[k] for k in ("vert_src", "vert_weights", "face_src", "report")}
    return out


# ---- edge flips -------------------------------------------------------------------------------------------------------------------------
_FLIP_SUMS = ("not_interior", "same_corner", "exists", "nonfinite", "criterion", "normals")


def flip_edges(verts, faces, criterion="delaunay", max_rounds=64):
    """Flip edges of an indexed mesh (verts (V,3), faces (F,3) integer ids) until none asks for it: rounds of `mesh_flip_round`
    (arah_mesh_flip_round on the GPU, meshing.mesh_flip_round on the host, equal bit for bit).  A flip replaces the edge {u, v}
    between the faces (u, v, a) and (v, u, b) by {a, b} between (a, u, b) and (b, v, a): vertices, the face count, the faces'
    order and the topology stay.  Only an edge with one face each way whose flipped edge is not there yet and whose new faces
    look the way the old ones did can flip, so boundary, non-manifold and misoriented edges and edges at a non-finite vertex
    never do.

        criterion   "delaunay": an edge flips when the two angles opposite to it sum to more than pi (cot + cot < 0, decided
                    without a square root) -- on a planar triangulation the loop ends at the Delaunay triangulation;
                    "valence": when it lowers the sum of |valence - target| over the four vertices around it, target 6, or 4
                    on a boundary
        max_rounds  the most rounds

    Round r runs with salt = r: a round flips the candidates that hold the least hashed key at all four of their vertices, and
    the hash changes with the round.  The loop ends after a round WITHOUT A CANDIDATE (converged), or after max_rounds.  ONE
    host synchronisation per round (its counts).

    -> dict of faces (F,3) in the dtype of `faces`, rounds (the rounds run, the last, empty one included), converged, flips (the
    flips applied), candidates (per round) and the rounds' summed counts not_interior, same_corner, exists, nonfinite, criterion
    and normals (edges that were no candidates, by their first reason)."""
    from . import meshing
    meshing.flip_args(criterion, 0, "flip_edges")
    if isinstance(max_rounds, bool) or not isinstance(max_rounds, (int, np.integer)) or int(max_rounds) < 0:
        raise ValueError("flip_edges: max_rounds must be an integer >= 0, got %r" % (max_rounds,))
    n_verts, faces = _mesh_args(verts, faces, "flip_edges")
    _check_mesh_verts(verts, faces, "flip_edges")
    backend, names = _cc_backend(faces), meshing.FLIP_COUNTS
    with torch.no_grad():
        v, f = verts.detach().to(torch.float32).contiguous(), faces
        sums, history, flips, rounds, converged = dict.fromkeys(_FLIP_SUMS, 0), [], 0, 0, False
        while rounds < int(max_rounds) and not converged:
            out = backend.mesh_flip_round(v, f, criterion, rounds)
            c = dict(zip(names, out[2].tolist()))                                 # the host synchronisation
            rounds += 1
            history.append(c["candidates"])
            for k in _FLIP_SUMS:
                sums[k] += c[k]
            flips += c["selected"]
            converged = c["candidates"] == 0
            if not converged:
                f = out[0]
    return dict(sums, faces=f.to(faces.dtype), rounds=rounds, converged=converged, flips=flips, candidates=history)


# ---- isotropic remeshing and its yardstick --------------------------------------------------------------------------------------
_ISOTROPIC_KEYS = ("edge_length", "iterations", "lamb", "project", "max_rounds", "max_faces")


def _valid_faces(verts, faces):
    """The faces with three different ids in [0, V), as int64 on the host, and the vertices as float64 on the host."""
    f = faces.detach().cpu().long().reshape(-1, 3)
    V = int(verts.shape[0])
    ok = ((f >= 0) & (f < V)).all(1) & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    return verts.detach().cpu().double(), f[ok]


def _edge_lengths(p, f):
    """The lengths of the undirected edges of the valid faces f over the float64 positions p, on the host, in ascending (lo, hi)."""
    V = max(int(p.shape[0]), 1)
    e = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key = torch.unique(e.min(1).values * V + e.max(1).values)
    d = p[key // V] - p[key % V]
    return torch.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def mesh_quality(verts, faces, edge_length=None):
    """How regular the triangles of an indexed mesh are: verts (V,3) floating point, faces (F,3) integer ids, edge_length the
    target length (None: the mesh's own mean edge length).  Plain float64 tensor code ON THE HOST whatever the mesh's device (one
    copy; the same mesh gives the same numbers from both), over the faces with three different ids in range and the finite
    edges.  -> dict of Python numbers: n_verts, n_faces (the valid ones), n_edges, edge_length, edge_min / edge_mean / edge_max,
    edges_in_range (the share of edges with a length in [4/5, 4/3] of edge_length), min_angle_min / min_angle_mean (degrees, of the
    smallest angle of every face), small_angle_share (the share of faces with an angle below 30 degrees), valence6_share and
    valence5to7_share (of the vertices that have a neighbour and lie on no boundary or non-manifold edge)."""
    import math
    n_verts, faces = _mesh_args(verts, faces, "mesh_quality")
    if not isinstance(verts, torch.Tensor) or verts.dim() != 2 or not verts.dtype.is_floating_point:
        raise ValueError("mesh_quality: verts must be a floating-point (V, 3) tensor")
    if edge_length is not None and (isinstance(edge_length, bool) or not isinstance(edge_length, (int, float, np.integer, np.floating))
                                    or not math.isfinite(float(edge_length)) or float(edge_length) <= 0.0):
        raise ValueError("mesh_quality: edge_length must be a finite length > 0, got %r" % (edge_length,))
    nan = float("nan")
    with torch.no_grad():
        p, f = _valid_faces(verts, faces)
        length = _edge_lengths(p, f)
        length = length[torch.isfinite(length)]
        n_edges = int(length.shape[0])
        L = float(edge_length) if edge_length is not None else (float(length.mean()) if n_edges else nan)
        out = {"n_verts": n_verts, "n_faces": int(f.shape[0]), "n_edges": n_edges, "edge_length": L,
               "edge_min": float(length.min()) if n_edges else nan, "edge_mean": float(length.mean()) if n_edges else nan,
               "edge_max": float(length.max()) if n_edges else nan,
               "edges_in_range": float(((length >= 0.8 * L) & (length <= 4.0 / 3.0 * L)).double().mean()) if n_edges else nan}
        t = p[f]                                                                  # (F,3,3)
        angles = []
        for k in range(3):
            a, b = t[:, (k + 1) % 3] - t[:, k], t[:, (k + 2) % 3] - t[:, k]
            angles.append(torch.atan2(torch.linalg.cross(a, b).norm(dim=1), (a * b).sum(1)))
        least = torch.stack(angles, 1).min(1).values * (180.0 / math.pi) if f.shape[0] else torch.zeros(0, dtype=torch.float64)
        least = least[torch.isfinite(least)]
        some = int(least.shape[0]) > 0
        out.update({"min_angle_min": float(least.min()) if some else nan, "min_angle_mean": float(least.mean()) if some else nan,
                    "small_angle_share": float((least < 30.0).double().mean()) if some else nan})
        from . import meshing
        adj = meshing.mesh_adjacency(f, n_verts)
        deg = (adj[2][1:] - adj[2][:-1]).long()
        inner = deg[(deg > 0) & ((adj[6] & 3) == 0)]
        some = int(inner.shape[0]) > 0
        out.update({"valence6_share": float((inner == 6).double().mean()) if some else nan,
                    "valence5to7_share": float(((inner >= 5) & (inner <= 7)).double().mean()) if some else nan})
    return out


def check_isotropic(isotropic):
    """The mesh entries' `isotropic` option, validated: None stays None, a number is the target edge length, a dict holds
    keywords of `isotropic_remesh` (edge_length, iterations, lamb, project, max_rounds, max_faces).  -> the dict of keywords;
    ValueError for anything else."""
    import math
    from . import meshing
    if isotropic is None:
        return None
    if isinstance(isotropic, (int, float, np.integer, np.floating)) and not isinstance(isotropic, bool):
        isotropic = {"edge_length": float(isotropic)}
    if not isinstance(isotropic, dict):
        raise ValueError("isotropic must be None, an edge length or a dict of isotropic_remesh keywords, got %r" % (isotropic,))
    bad = set(isotropic) - set(_ISOTROPIC_KEYS)
    if bad:
        raise ValueError("isotropic: unknown keys %s (known: %s)" % (sorted(bad), ", ".join(_ISOTROPIC_KEYS)))
    kw = dict(isotropic)
    L = kw.get("edge_length")
    if L is not None and (isinstance(L, bool) or not isinstance(L, (int, float, np.integer, np.floating)) or not math.isfinite(float(L))
                          or float(L) <= 0.0):
        raise ValueError("isotropic_remesh: edge_length must be a finite length > 0, got %r" % (L,))
    for name, least in (("iterations", 0), ("max_rounds", 1), ("max_faces", 0)):
        x = kw.get(name, least)
        if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or int(x) < least:
            raise ValueError("isotropic_remesh: %s must be an integer >= %d, got %r" % (name, least, x))
    meshing.check_tangential_lamb(kw.get("lamb", 0.5), "isotropic_remesh")
    if not isinstance(kw.get("project", True), bool):
        raise ValueError("isotropic_remesh: project must be True or False, got %r" % (kw["project"],))
    return kw


def _closest_on_input(tris, index, pts):
    """d2, face, closest of the float32 points against the input's soup: hip.mesh_closest on the GPU, its rule on the host."""
    from . import meshing
    if tris.is_cuda and int(tris.shape[0]) > 0:
        from . import hip
        return hip.mesh_closest(index, pts)[:3]
    return meshing.soup_closest(tris, pts)


def isotropic_remesh(verts, faces, edge_length=None, iterations=5, lamb=0.5, project=True, max_rounds=32, max_faces=1 << 24,
                     attributes=None):
    """Remesh an indexed mesh (verts (V,3), faces (F,3) integer ids) towards triangles of one size and vertices of valence six, after
    Botsch and Kobbelt, "A remeshing approach to multiresolution modeling" (2004).  With L = edge_length (None: the input's mean
    edge length), every one of the `iterations` does

        1  split     rounds of `mesh_subdivide_round` on the edges longer than 4/3 L until a round marks none
        2  collapse  rounds of `mesh_collapse_round` on the edges shorter than 4/5 L, refusing a collapse that would leave an edge
                     longer than 4/3 L at the new vertex, until a round applies none
        3  flip      `flip_edges(criterion="valence")` until no candidate is left
        4  relax     one `mesh_tangential_step` with `lamb`, the normals taken from the mesh at hand
        5  project   (project=True) every vertex moves to the closest point of the INPUT mesh, rounded once to float32; the index
                     of the input is built once

    each loop also ending after max_rounds rounds; a split round whose worst case, four times its faces, exceeds max_faces
    raises.  Every step runs its kernels for a mesh on the GPU and its tensor specification for one on the host, equal bit for
    bit, so the whole call is; one host synchronisation per round.  Boundary, non-manifold and misoriented edges are split but
    never collapsed or flipped and their vertices are not relaxed: a closed manifold surface stays one.

    -> dict of verts (V',3) float32, faces (F',3) in the dtype of `faces`, n_verts, n_tris, src_face (V',) int64 and src_bary
    (V',3) float64 -- the closest input face of every output vertex and the barycentric weights of the closest point in it (-1
    and NaN for a vertex that is not finite) --, every tensor of the dict `attributes` (first dimension V) carried over through
    them: (w0 A0 + w1 A1) + w2 A2 in float64 rounded to the attribute's dtype when that is floating, the attribute of the corner
    with the largest weight (the first of them) otherwise; and report = dict of edge_length, iterations (a list of dicts of
    faces, splits, collapses and flips, one per iteration), and before / after, the `mesh_quality` of the input and of the
    output against L."""
    from . import meshing
    kw = check_isotropic({"edge_length": edge_length, "iterations": iterations, "lamb": lamb, "project": project,
                          "max_rounds": max_rounds, "max_faces": max_faces})
    n_verts, faces = _mesh_args(verts, faces, "isotropic_remesh")
    _check_mesh_verts(verts, faces, "isotropic_remesh")
    reserved = ("verts", "faces", "n_verts", "n_tris", "src_face", "src_bary", "report")
    attributes = _repair_attributes(attributes, n_verts, verts.device, reserved, "isotropic_remesh")
    backend, dev = _cc_backend(faces), verts.device
    with torch.no_grad():
        v0 = verts.detach().to(torch.float32).contiguous()
        p64, valid = _valid_faces(v0, faces)
        if edge_length is None:
            length = _edge_lengths(p64, valid)
            length = length[torch.isfinite(length)]
            if int(length.shape[0]) == 0:
                raise ValueError("isotropic_remesh: the mesh has no finite edge to take the target length from")
            L = float(length.mean())
        else:
            L = float(edge_length)
        long2, short2 = (4.0 / 3.0 * L) ** 2, (0.8 * L) ** 2
        corners = valid.to(dev)
        tris = v0[corners] if int(corners.shape[0]) else v0.new_zeros((0, 3, 3))
        index = None
        if tris.is_cuda and int(tris.shape[0]) > 0:
            from . import hip
            index = hip.mesh_index(tris)
        before = mesh_quality(v0, faces, L)
        v, f, steps = v0, faces, []
        for _ in range(int(iterations)):
            splits = collapses = 0
            for _r in range(int(max_rounds)):
                if 4 * int(f.shape[0]) > int(max_faces):
                    raise ValueError("isotropic_remesh: a split round of %d faces gives up to %d faces, more than max_faces = %d"
                                     % (int(f.shape[0]), 4 * int(f.shape[0]), int(max_faces)))
                out = backend.mesh_subdivide_round(v, f, "midpoint", long2)
                c = dict(zip(meshing.SUBDIVIDE_COUNTS, out[4].tolist()))              # the host synchronisation
                if c["marked"] == 0:
                    break
                v, f, splits = out[0][:c["n_verts"]], out[1][:c["n_faces"]], splits + c["marked"]
            for _r in range(int(max_rounds)):
                out = backend.mesh_collapse_round(v, f, 2 ** 31 - 1, short_len2=short2, long_len2=long2)
                c = dict(zip(meshing.COLLAPSE_BOUNDED_COUNTS, out[4].tolist()))       # the host synchronisation
                if c["applied"] == 0:
                    break
                v, f, collapses = out[0][:c["n_verts"]], out[1][:c["n_faces"]], collapses + c["applied"]
            flipped = flip_edges(v, f, "valence", int(max_rounds))
            f = flipped["faces"]
            adj = backend.mesh_adjacency(f, int(v.shape[0]))
            v = backend.mesh_tangential_step(v, f, backend.vertex_normals(v, f, adjacency=adj)[0], lamb, adjacency=adj)
            if project:
                _, face, closest = _closest_on_input(tris, index, v)
                v = torch.where((face >= 0)[:, None], closest.float(), v)
            steps.append({"faces": int(f.shape[0]), "splits": splits, "collapses": collapses, "flips": flipped["flips"]})
        _, face, closest = _closest_on_input(tris, index, v)
        found = face >= 0
        at = corners[face.long().clamp(min=0)] if int(corners.shape[0]) else torch.zeros(int(v.shape[0]), 3, dtype=torch.long, device=dev)
        if int(corners.shape[0]):
            a, b, c3 = (v0.double()[at[:, k]] for k in range(3))
            bary = torch.stack(meshing.closest_on_triangles(v.double(), a, b, c3), 1)
        else:
            bary = torch.full((int(v.shape[0]), 3), float("nan"), dtype=torch.float64, device=dev)
        bary = torch.where(found[:, None], bary, torch.full_like(bary, float("nan")))
        # src_face counts the INPUT's rows, skipped faces included
        rows = torch.nonzero(_valid_rows(faces, n_verts))[:, 0]
        src_face = torch.where(found, rows[face.long().clamp(min=0)] if int(rows.shape[0]) else face.long(), torch.full_like(face.long(), -1))
        res = {"verts": v, "faces": f.to(faces.dtype), "n_verts": int(v.shape[0]), "n_tris": int(f.shape[0]), "src_face": src_face,
               "src_bary": bary,
               "report": {"edge_length": L, "iterations": steps, "before": before, "after": mesh_quality(v, f, L)}}
        for name, t in attributes.items():
            A = t[at]                                                             # (V',3,...)
            if t.dtype.is_floating_point:
                w = bary.reshape(bary.shape + (1,) * (t.dim() - 1))
                res[name] = ((w[:, 0] * A[:, 0].double() + w[:, 1] * A[:, 1].double()) + w[:, 2] * A[:, 2].double()).to(t.dtype)
            else:
                best = torch.where(found[:, None], bary, torch.zeros_like(bary)).argmax(1)
                res[name] = A[torch.arange(int(v.shape[0]), device=dev), best]
    return res


def _valid_rows(faces, n_verts):
    """(F,) bool on the faces' device: the rows with three different ids in [0, V)."""
    f = faces.detach().long().reshape(-1, 3)
    return ((f >= 0) & (f < n_verts)).all(1) & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])


def apply_isotropic(verts, faces, isotropic):
    """The mesh entries' `isotropic` option, as `check_isotropic` returned it: -> the remeshed verts, faces, n_verts and n_tris of
    `isotropic_remesh`, and under "isotropic" its src_face, src_bary and report -- the entries' own vert_src and report (clean's,
    simplify's) stay what they are."""
    res = isotropic_remesh(verts, faces, **isotropic)
    out = {k: res[k] for k in ("verts", "faces", "n_verts", "n_tris")}
    out["isotropic"] = {k: res[k] for k in ("src_face", "src_bary", "report")}
    return out


# ---- adjacency, topology, per-vertex normals, smoothing -------------------------------------------------------------------------
MeshAdjacency =collections.namedtuple("MeshAdjacency", ("vf_start", "vf", "nbr_start", "nbr", "nbr_out", "nbr_in", "vert_flags",
                                                         "counts"))
MeshAdjacency.__doc__ = """The arrays of `mesh_adjacency`, on the mesh's device: vf_start (V+1,) / vf (3F,) the CSR of the valid
faces incident to every vertex (ids ascending); nbr_start (V+1,) / nbr (6F,) the CSR of its unique neighbours (ids ascending) with
nbr_out / nbr_in (6F,) the faces traversing v->n / n->v; vert_flags (V,) uint8 (1 boundary, 2 non-manifold, 4 no neighbour); counts
(8,) int32 (valid faces, edges, boundary, non-manifold and misoriented edges, the largest valence, isolated vertices, Euler)."""

_SMOOTH_KEYS = ("iterations", "lamb", "mu", "method", "boundary", "weights", "time")


def mesh_adjacency(verts_or_n_verts, faces):
    """Who is adjacent to whom in an indexed mesh (hip.mesh_adjacency on the GPU, meshing.mesh_adjacency on the host): faces (F,3)
    integer ids, and the vertices (V,3) or just their number.  A face with an id out of range or a repeated id is skipped.  -> a
    MeshAdjacency of arrays that stay on the mesh's device; no host synchronisation on the GPU.  Build it once and hand it to
    `vertex_normals` and `smooth_mesh` of the same mesh."""
    n_verts, faces = _mesh_args(verts_or_n_verts, faces, "mesh_adjacency")
    with torch.no_grad():
        return MeshAdjacency(*_cc_backend(faces).mesh_adjacency(faces, n_verts))


def mesh_topology(verts_or_n_verts, faces):
    """The topology of an indexed mesh from `mesh_adjacency`, as Python numbers: -> dict of faces (the valid ones), edges,
    boundary_edges (one face), nonmanifold_edges (three or more), misoriented_edges (two faces that traverse the edge in the same
    direction), isolated_vertices (no neighbour), max_valence, euler = (V - isolated_vertices) - edges + faces, skipped_faces (an
    id out of range or repeated), manifold (no non-manifold edge) and watertight (at least one face and no boundary, non-manifold or
    misoriented edge).  One host synchronisation (the counts)."""
    adj = mesh_adjacency(verts_or_n_verts, faces)
    c = adj.counts.tolist()                                                     # the host synchronisation
    return {"faces": c[0], "edges": c[1], "boundary_edges": c[2], "nonmanifold_edges": c[3], "misoriented_edges": c[4],
            "isolated_vertices": c[6], "max_valence": c[5], "euler": c[7], "skipped_faces": int(faces.shape[0]) - c[0],
            "manifold": c[3] == 0, "watertight": c[0] > 0 and c[2] == 0 and c[3] == 0 and c[4] == 0}


def _smooth_args(verts, faces, adjacency, what):
    n_verts, faces = _mesh_args(verts, faces, what)
    _check_mesh_verts(verts, faces, what)
    return verts.detach().to(torch.float32).contiguous(), faces, (None if adjacency is None else tuple(adjacency))


def vertex_normals(verts, faces, adjacency=None):
    """Unit per-vertex normals (V,3) float32 of an indexed mesh from the mesh itself, pytorch3d's verts_normals_packed: the sum of
    the incident faces' cross products (area-weighted face normals), normalised; (0, 0, 0) for a vertex without a valid face or
    with a sum of length 0.  Good for any mesh -- a loaded scan, a simplified or smoothed one --, unlike the SDF gradient
    canonical_mesh(attributes=("normal",)) gives.  adjacency: a `mesh_adjacency` of the same mesh built earlier, or None.
    hip.vertex_normals on the GPU, meshing.vertex_normals on the host, equal bit for bit."""
    v32, faces, adjacency = _smooth_args(verts, faces, adjacency, "vertex_normals")
    with torch.no_grad():
        return _cc_backend(faces).vertex_normals(v32, faces, adjacency=adjacency)[1]


def _check_smooth_call(iterations, lamb, mu, method, boundary, what, weights="uniform", time=None):
    """meshing.check_smooth_args, and method="tangential": iterations and lamb as for "laplacian"; mu is not used, and boundary
    must be "pin" (a tangential step never moves a vertex of a boundary or non-manifold edge).  -> True for "tangential".
    method="implicit": iterations, time and boundary (meshing.check_implicit_args); lamb, mu and weights are not used.  -> False."""
    from . import meshing
    if method == "implicit":
        meshing.check_implicit_args(iterations, time, boundary, what)
        return False
    if time is not None:
        raise ValueError("%s: time belongs to method='implicit', got it with method=%r" % (what, method))
    meshing.check_smooth_weights(weights, what)
    if method == "tangential" and weights != "uniform":
        raise ValueError("%s: method='tangential' has uniform weights only, got weights=%r" % (what, weights))
    if method != "tangential":
        meshing.check_smooth_args(iterations, lamb, mu, method, boundary, what)
        return False
    meshing.check_smooth_args(iterations, lamb, -0.53, "laplacian", "pin", what)
    if boundary != "pin":
        raise ValueError("%s: method='tangential' keeps boundary vertices where they are: boundary must be 'pin', got %r" % (what, boundary))
    return True


def smooth_mesh(verts, faces, iterations=10, lamb=0.5, mu=-0.53, method="taubin", boundary="pin", adjacency=None, weights="uniform",
                time=None):
    """Smooth an indexed mesh with the umbrella operator: every step moves a vertex towards (lamb > 0) or away from (mu < 0) the
    mean of its neighbours, p + f (mean - p), uniform weights.  method="taubin" (Taubin 1995, "A signal processing approach to
    fair surface design"): an iteration is a lamb step and a mu step, a low-pass filter that does not shrink the mesh the way
    method="laplacian" (lamb steps only) does.  boundary="pin" keeps the vertices of boundary and non-manifold edges where they
    are, "free" moves them like the others.  lamb in (0, 1], mu in [-1.1, 0), iterations >= 0.  -> verts (V,3) float32; faces,
    the vertex count and the order stay, so every per-vertex attribute stays valid.  Vertices with a non-finite coordinate stay
    and are left out of their neighbours' means.  adjacency: a `mesh_adjacency` of the same mesh built earlier, or None.
    hip.mesh_smooth on the GPU (no host synchronisation), meshing.mesh_smooth on the host, equal bit for bit.

    method="tangential": every iteration is one `mesh_tangential_step` with lamb -- the umbrella step without its part along the
    vertex normal, which is taken from the mesh at hand (`vertex_normals`' unnormalised sum, recomputed every iteration).  Vertices
    slide along the surface: the triangles even out and the shape neither shrinks nor loses detail the way it does along the
    normal.  Vertices of boundary and non-manifold edges stay (boundary must be "pin"); mu is not used.  hip.mesh_tangential_step
    on the GPU, meshing.mesh_tangential_step on the host, equal bit for bit.

    weights="cotangent" (with "taubin" or "laplacian"): every step takes the cotangent weights of the positions it reads
    (`mesh_laplacian`) instead of uniform ones: p + f (sum w (q - p)) / (sum |w|), the explicit mean-curvature flow.  On a flat
    patch it does not move a vertex at all, whatever the sampling, where the uniform mean drags vertices along
    the surface towards their denser side: the choice for decimated, adaptively subdivided and marching-cubes meshes.  It costs
    the operator once per step.  hip.mesh_smooth on the GPU, meshing.mesh_smooth on the host, equal bit for bit.

    method="implicit", time=t: implicit fairing (Desbrun, Meyer, Schroeder, Barr 1999): every iteration solves (M + t S) p' = M p
    with the cotangent operator S and the mixed-cell mass M of the positions it reads (`solve_laplacian`, tol 1e-10), and rounds
    the result once to float32.  time is a length squared, required and > 0: one iteration removes detail below about sqrt(t) for
    ANY t, where the explicit steps above are stable only for small ones -- a bump ten edges wide goes in one solve instead of
    hundreds of steps.  boundary="pin" holds the vertices of boundary and non-manifold edges, "free" none; held vertices (and
    those with a non-finite coordinate or without area) stay bit for bit.  lamb, mu and weights are not used.  A solve that does
    not converge raises RuntimeError with its status and residual.  meshing.mesh_smooth_implicit is the rule, over
    hip.laplacian_solve on the GPU and meshing.laplacian_solve on the host, equal bit for bit."""
    tangential = _check_smooth_call(iterations, lamb, mu, method, boundary, "smooth_mesh", weights, time)
    v32, faces, adjacency = _smooth_args(verts, faces, adjacency, "smooth_mesh")
    if method == "implicit":
        from . import meshing
        backend = _cc_backend(faces)
        with torch.no_grad():
            if adjacency is None:
                adjacency = backend.mesh_adjacency(faces, int(v32.shape[0]))
            return meshing.mesh_smooth_implicit(v32, faces, iterations, time, boundary, adjacency,
                                                backend=None if backend is meshing else backend)
    if tangential:
        backend = _cc_backend(faces)
        with torch.no_grad():
            if adjacency is None:
                adjacency = backend.mesh_adjacency(faces, int(v32.shape[0]))
            for _ in range(int(iterations)):
                normal_sum = backend.vertex_normals(v32, faces, adjacency=adjacency)[0]
                v32 = backend.mesh_tangential_step(v32, faces, normal_sum, lamb, adjacency=adjacency)
        return v32
    with torch.no_grad():
        if weights == "uniform":                                                  # the call as it always was
            return _cc_backend(faces).mesh_smooth(v32, faces, iterations, lamb=lamb, mu=mu, method=method, boundary=boundary,
                                                  adjacency=adjacency)
        return _cc_backend(faces).mesh_smooth(v32, faces, iterations, lamb=lamb, mu=mu, method=method, boundary=boundary,
                                              adjacency=adjacency, weights=weights)


# ---- the cotangent Laplacian and curvatures ---------------------------------------------------------------------------------------
def mesh_laplacian(verts, faces, mass="mixed", adjacency=None):
    """The cotangent Laplacian of an indexed mesh with its lumped mass (hip.mesh_cotangent on the GPU, meshing.mesh_cotangent --
    which states the rule -- on the host): verts (V,3), faces (F,3) integer ids, mass "mixed" (Meyer et al.'s Voronoi cells, safe
    with obtuse triangles) or "barycentric" (a third of the incident faces), adjacency a `mesh_adjacency` built earlier or None.
    -> dict of weight (6F,) float64 -- for the entry (v, n) of adjacency.nbr half the sum of the cotangents opposite to the edge,
    the same bits from both ends --, diag (V,) the row sums, area (V,) the lumped mass, angle_sum (V,) the sum of the angles at the
    vertex, adjacency (the MeshAdjacency used) and report: the counts by name (meshing.COTANGENT_COUNTS: faces, degenerate,
    nonfinite, obtuse, negative_edges, bad_area) as Python numbers, one host synchronisation.  negative_edges are the edges that are
    not locally Delaunay: `flip_edges`("delaunay") removes them where the surface allows it.  Everything stays on the mesh's
    device; hand the dict to `laplacian_matrix`, `apply_laplacian` and `mesh_curvature`."""
    from . import meshing
    v32, faces, adjacency = _smooth_args(verts, faces, adjacency, "mesh_laplacian")
    backend = _cc_backend(faces)
    with torch.no_grad():
        if adjacency is None:
            adjacency = backend.mesh_adjacency(faces, int(v32.shape[0]))
        weight, diag, area, angle_sum, counts = backend.mesh_cotangent(v32, faces, mass, adjacency=adjacency)
    return {"weight": weight, "diag": diag, "area": area, "angle_sum": angle_sum, "adjacency": MeshAdjacency(*adjacency),
            "report": dict(zip(meshing.COTANGENT_COUNTS, counts.tolist())), "mass": mass}


def _check_laplacian(lap, what):
    if not isinstance(lap, dict) or any(k not in lap for k in ("weight", "diag", "area", "angle_sum", "adjacency")):
        raise ValueError("%s: lap must be the dict of mesh_laplacian" % what)
    return lap


def laplacian_matrix(lap, kind="stiffness"):
    """The operator of `mesh_laplacian` as a torch sparse CSR matrix (V, V) float64 on the mesh's device: off-diagonals weight,
    diagonal -diag, so that L x = `apply_laplacian`(lap, x) up to the order of the sums; kind="normalized": every row divided by
    the vertex's area (rows of vertices whose area is not > 0 are not finite).  "stiffness" is symmetric, negative semi-definite,
    with zero row sums.  Built from the neighbour CSR that is already there -- the diagonal is merged into each sorted row by its
    position, no sort."""
    lap = _check_laplacian(lap, "laplacian_matrix")
    if kind not in ("stiffness", "normalized"):
        raise ValueError("laplacian_matrix: kind must be 'stiffness' or 'normalized', got %r" % (kind,))
    adj = lap["adjacency"]
    start, nbr = adj.nbr_start.long(), adj.nbr.long()
    V, dev = int(start.shape[0]) - 1, start.device
    E = int(start[-1]) if V else 0
    ids = torch.arange(V, device=dev)
    deg = start[1:] - start[:-1]
    row = torch.repeat_interleave(ids, deg)
    col_off, val_off = nbr[:E], lap["weight"][:E]
    below = torch.zeros(V, dtype=torch.int64, device=dev).index_add_(0, row, (col_off < row).long())   # neighbours in front of v
    # row v holds deg[v] + 1 entries: its neighbours below v, v itself, the neighbours above
    crow = torch.zeros(V + 1, dtype=torch.int64, device=dev)
    crow[1:] = torch.cumsum(deg + 1, 0)
    k = torch.arange(E, device=dev) - start[:-1][row]                             # position inside the neighbour row
    at_off = crow[:-1][row] + k + (k >= below[row]).long()
    at_diag = crow[:-1] + below
    cols = torch.empty(E + V, dtype=torch.int64, device=dev)
    vals = torch.empty(E + V, dtype=torch.float64, device=dev)
    cols[at_off], vals[at_off] = col_off, val_off
    cols[at_diag], vals[at_diag] = ids, -lap["diag"]
    if kind == "normalized":
        vals = vals / lap["area"][torch.repeat_interleave(ids, deg + 1)]
    with warnings.catch_warnings():                                              # torch announces its CSR support as beta, once
        warnings.filterwarnings("ignore", message="Sparse CSR tensor support is in beta state")
        return torch.sparse_csr_tensor(crow, cols, vals, size=(V, V), dtype=torch.float64, device=dev)


def apply_laplacian(lap, x):
    """L x for the dict of `mesh_laplacian`: x (V,) or (V,C) float32 or float64 with C <= 32, on the mesh's device.  -> float64 of
    the same shape: y[v] = sum over the neighbours in ascending id of weight (x[n] - x[v]); neighbours whose x is not finite are
    skipped.  Divide by lap["area"] for the pointwise Laplace-Beltrami operator.  hip.laplacian_apply on the GPU,
    meshing.laplacian_apply on the host, equal bit for bit."""
    lap = _check_laplacian(lap, "apply_laplacian")
    if not isinstance(x, torch.Tensor) or x.dim() not in (1, 2):
        raise ValueError("apply_laplacian: x must be a (V,) or (V, C) tensor")
    x2 = x.detach()[:, None] if x.dim() == 1 else x.detach()
    with torch.no_grad():
        y = _cc_backend(lap["weight"]).laplacian_apply(lap["weight"], tuple(lap["adjacency"]), x2.contiguous())
    return y[:, 0] if x.dim() == 1 else y


def mesh_curvature(verts, faces, mass="mixed", adjacency=None, laplacian=None):
    """Mean, Gaussian and principal curvatures at the vertices of an indexed mesh (Meyer, Desbrun, Schroeder, Barr 2002, "Discrete
    differential-geometry operators for triangulated 2-manifolds"; meshing.mesh_curvature states the rule): verts (V,3), faces
    (F,3) integer ids, mass as in `mesh_laplacian`, adjacency a `mesh_adjacency` built earlier or None, laplacian the dict of
    `mesh_laplacian` of this mesh or None.  -> dict of mean, mean_abs, gaussian, k1 >= k2 (V,) float64, mean_normal (V,3) float64
    (the mean-curvature normal, half of the Laplacian of the positions over the area), area (V,), valid (V,) bool and report (the
    operator's counts and invalid_vertices; one host synchronisation).  mean_abs = |mean_normal| carries no sign; mean takes its sign
    from the mesh's own orientation: > 0 on a convex part of a mesh with counter-clockwise faces seen from outside, and < 0 THERE
    ON THE PROJECT'S OWN LEVEL SETS, whose marching-cubes faces are clockwise seen from outside.  gaussian is the angle defect over
    the area (pi instead of 2 pi on a boundary).  Vertices on non-manifold edges, without a face, with a non-finite coordinate or
    without area are invalid: NaN, valid False.  hip.mesh_curvature on the GPU, meshing.mesh_curvature on the host: equal bit for
    bit but for the last bits of the angles' atan2."""
    v32, faces, adjacency = _smooth_args(verts, faces, adjacency, "mesh_curvature")
    backend = _cc_backend(faces)
    with torch.no_grad():
        if laplacian is None:
            laplacian = mesh_laplacian(v32, faces, mass, adjacency)
        lap = _check_laplacian(laplacian, "mesh_curvature")
        adj = tuple(lap["adjacency"])
        curv, mean_normal, valid, counts = backend.mesh_curvature(
            v32, faces, mass, adjacency=adj, laplacian=(lap["weight"], lap["diag"], lap["area"], lap["angle_sum"]))
    out = {name: curv[:, i].contiguous() for i, name in enumerate(("mean", "mean_abs", "gaussian", "k1", "k2"))}
    out.update(mean_normal=mean_normal, area=lap["area"], valid=valid.bool(),
               report=dict(lap["report"], invalid_vertices=int(counts[0])))
    return out


# ---- solving with the cotangent operator ------------------------------------------------------------------------------------------
def solve_laplacian(lap, rhs, mass_coef=0.0, stiff_coef=1.0, pinned=None, x0=None, tol=1e-10, max_iter=10000, check_every=32):
    """Solve (mass_coef M + stiff_coef S) x = rhs with the dict of `mesh_laplacian` -- M its lumped mass (area), S = -L its
    stiffness, positive semi-definite -- by Jacobi-preconditioned conjugate gradients in float64 (hip.laplacian_solve on the GPU,
    meshing.laplacian_solve -- which states the rule -- on the host, equal bit for bit).  rhs (V,) or (V,C) float32 or float64, C <=
    32 independent columns; mass_coef >= 0, stiff_coef > 0; pinned (V,) bool or None: vertices held at x0; x0 like rhs, zeros when
    None: the start, and the value of every held vertex.  Besides the pinned, vertices with a non-finite x0 or rhs row, without
    area (when mass_coef > 0) or without a positive diagonal are held; a held vertex is a Dirichlet value for its neighbours where
    its x0 is finite and is left out of their sums where it is not.  With mass_coef = 0 every connected component needs a held
    vertex, or its column of rhs must sum to 0.  tol: the relative residual |r| / |r0| at which a column stops; check_every: steps
    per batch on the GPU, between two looks at the statuses (the result does not depend on it).

    -> dict of x (float64, of rhs's shape), iterations and status ("converged" | "max_iter" | "breakdown") per column -- numbers
    and strings for a (V,C) rhs, one of each for a (V,) one --, converged (all of them), residual = sqrt(rr / r0) of the
    recurrence, true_residual = |rhs - A x| over the solved rows / sqrt(r0) from one more application of the operator (0 where r0
    is 0), and report: the vertices by class (meshing.SOLVE_COUNTS).  "breakdown": p.Ap was not positive or not finite -- the
    operator is indefinite (weights spoiled from outside) or the numbers overflowed; x is the last iterate.  Both residuals are
    relative to the start's: where x0 already solves the system to rounding, r0 is rounding noise and true_residual stays near 1."""
    from . import meshing
    what = "solve_laplacian"
    lap = _check_laplacian(lap, what)
    if not isinstance(rhs, torch.Tensor) or rhs.dim() not in (1, 2) or rhs.dtype not in (torch.float32, torch.float64):
        raise ValueError("%s: rhs must be a (V,) or (V, C) float32 or float64 tensor" % what)
    if x0 is not None and (not isinstance(x0, torch.Tensor) or x0.shape != rhs.shape or x0.dtype not in (torch.float32, torch.float64)):
        raise ValueError("%s: x0 must be a float32 or float64 tensor of rhs's shape %s, or None" % (what, tuple(rhs.shape)))
    weight, area, adj = lap["weight"], lap["area"], tuple(lap["adjacency"])
    one = rhs.dim() == 1
    b = (rhs.detach()[:, None] if one else rhs.detach()).to(torch.float64).contiguous()
    start = torch.zeros_like(b) if x0 is None else (x0.detach()[:, None] if one else x0.detach()).to(torch.float64).contiguous()
    backend = _cc_backend(weight)
    extra = {"check_every": check_every} if backend is not meshing else {}
    with torch.no_grad():
        x, iters, status, rr, r0, counts, classes = backend.laplacian_solve(weight, area, adj, b, start, pinned=pinned, mass_coef=mass_coef,
                                                                            stiff_coef=stiff_coef, tol=tol, max_iter=max_iter, **extra)
        # one more application of the operator: rows that are not live are hidden from their neighbours as the solver hides them
        solved = (classes == 0)[:, None]
        live = torch.isfinite(start).all(1, keepdim=True)
        y = backend.laplacian_apply(weight, adj, torch.where(live, x, torch.full_like(x, float("nan"))))
        ax = -float(stiff_coef) * y if float(mass_coef) == 0.0 else float(mass_coef) * (area[:, None] * x) - float(stiff_coef) * y
        res = torch.where(solved, b - ax, torch.zeros_like(b))
        scale = torch.where(r0 > 0, r0, torch.ones_like(r0))
        true = torch.where(r0 > 0, torch.sqrt((res * res).sum(0) / scale), torch.zeros_like(r0))
        rel = torch.where(r0 > 0, torch.sqrt(rr / scale), torch.zeros_like(r0))
        host = torch.stack([rel, true]).cpu()                                      # with the next three: the call's last synchronisations
    names = [meshing.SOLVE_STATUS[s] for s in status.tolist()]
    out = {"x": x[:, 0] if one else x, "iterations": iters.tolist(), "status": names, "converged": all(s == "converged" for s in names),
           "residual": host[0].tolist(), "true_residual": host[1].tolist(), "report": dict(zip(meshing.SOLVE_COUNTS, counts.tolist()))}
    if one:
        out.update({k: out[k][0] for k in ("iterations", "status", "residual", "true_residual")})
    return out


def harmonic_extend(verts, faces, known, values, laplacian=None, adjacency=None, tol=1e-10, max_iter=10000):
    """The harmonic extension of per-vertex values from the vertices where they are known to all others: S x = 0 with x = values at
    `known` -- the smoothest fill-in (it minimises the Dirichlet energy), for the attributes (skinning weights, colours) of
    vertices that `fill_holes`, `subdivide_mesh` or a remesh created.  verts (V,3), faces (F,3); known (V,) bool; values (V,) or
    (V,C) float32 or float64, C <= 32, read at the known vertices only; laplacian: the dict of `mesh_laplacian` of this mesh or
    None; adjacency as there.  It is `solve_laplacian` with mass_coef 0, rhs 0, pinned = known and x0 = values where known, 0
    elsewhere.  -> dict of values (float64, of values' shape: the input at the known vertices, the extension elsewhere) and the
    solver's iterations, status, converged, residual, true_residual and report.  A connected component without a known vertex
    keeps 0 and converges at once (its right-hand side is 0).  With cotangent weights the extension of a linear function over a
    planar mesh is that function; negative weights (edges that are not Delaunay) can take it outside the known values' range."""
    what = "harmonic_extend"
    if laplacian is None:
        laplacian = mesh_laplacian(verts, faces, adjacency=adjacency)
    lap = _check_laplacian(laplacian, what)
    V, dev = int(lap["area"].shape[0]), lap["area"].device
    if not isinstance(known, torch.Tensor) or tuple(known.shape) != (V,) or known.dtype != torch.bool or known.device != dev:
        raise ValueError("%s: known must be a (V,) bool tensor on %s" % (what, dev))
    if not isinstance(values, torch.Tensor) or values.dim() not in (1, 2) or int(values.shape[0]) != V \
            or values.dtype not in (torch.float32, torch.float64) or values.device != dev:
        raise ValueError("%s: values must be a (V,) or (V, C) float32 or float64 tensor on %s" % (what, dev))
    vals = values.detach().to(torch.float64)
    x0 = torch.where(known if vals.dim() == 1 else known[:, None], vals, torch.zeros_like(vals))
    out = solve_laplacian(lap, torch.zeros_like(vals), 0.0, 1.0, pinned=known, x0=x0, tol=tol, max_iter=max_iter)
    out["values"] = out.pop("x")
    return out


# ---- orientation, boundary loops, hole filling -----------------------------------------------------------------------------------
def _repair_attributes(attributes, n_verts, dev, reserved, what):
    attributes = dict(attributes or {})
    for name, t in attributes.items():
        if name in reserved:
            raise ValueError("%s: an attribute cannot be called %r" % (what, name))
        if not isinstance(t, torch.Tensor) or t.dim() < 1 or t.shape[0] != n_verts or t.device != dev:
            raise ValueError("%s: attribute %r must be a tensor with %d rows on %s" % (what, name, n_verts, dev))
    return attributes


def orient_mesh(verts, faces, policy="majority", adjacency=None):
    """Orient the faces of an indexed mesh consistently (hip.mesh_orient on the GPU, meshing.mesh_orient on the host, equal bit for
    bit; the rules are stated in meshing.mesh_orient).  Faces that share an edge with exactly one other face are made to traverse
    it in opposite directions, component by component; edges with one face or with three or more carry no constraint, so a
    non-manifold edge separates components.  A non-orientable component (a Moebius strip) is left as it is and counted.

        policy = "seed"        the lowest face of every component keeps its orientation
                 "majority"    the orientation held by more faces of the component wins, ties go to "seed"
                 "negative" /  the component's signed volume gets that sign -- the project's own meshes are negative
                 "positive"    (winding_orient gives -1); a zero volume falls back to "majority"

    verts (V,3), or just the vertex count under "seed" and "majority"; adjacency: a `mesh_adjacency` of the same mesh built
    earlier, or None.  -> dict of faces (F,3) in the dtype of the input: row order and vertices never change, a flipped row (a, b,
    c) becomes (a, c, b); flip (F,) uint8; face_component (F,) int32, -1 for a skipped face; n_components, n_nonorientable,
    n_flipped; component_faces (C,) int32; component_nonorientable (C,) bool.  One host synchronisation (the counts), and one more
    for the vertices' bounds under the two volume policies."""
    from . import meshing
    meshing.check_orient_policy(policy, "orient_mesh")
    n_verts, faces = _mesh_args(verts, faces, "orient_mesh")
    by_volume = policy in ("negative", "positive")
    if isinstance(verts, torch.Tensor) and verts.dim() > 0:
        if not verts.dtype.is_floating_point:
            raise ValueError("orient_mesh: verts must be a floating-point (V, 3) tensor")
        if verts.device != faces.device:
            raise ValueError("orient_mesh: verts live on %s, faces on %s" % (verts.device, faces.device))
    elif by_volume:
        raise ValueError("orient_mesh: policy %r needs the vertices, not their number" % (policy,))
    with torch.no_grad():
        v = verts.detach().to(torch.float32).contiguous() if by_volume else n_verts
        flip, face_comp, _, comp_faces, comp_flags, _, _, counts = _cc_backend(faces).mesh_orient(
            v, faces, policy=policy, adjacency=None if adjacency is None else tuple(adjacency))
        c = counts.tolist()                                                     # the host synchronisation
        out = torch.where(flip.bool()[:, None], faces[:, [0, 2, 1]], faces)
    return {"faces": out, "flip": flip, "face_component": face_comp, "n_components": c[1], "n_nonorientable": c[2],
            "n_flipped": c[5], "component_faces": comp_faces[:c[1]], "component_nonorientable": (comp_flags[:c[1]] & 1).bool()}


def boundary_loops(verts_or_n_verts, faces, adjacency=None):
    """The boundary of an indexed mesh (hip.mesh_boundary_loops on the GPU, meshing.mesh_boundary_loops on the host): the directed
    edges a->b of valid faces whose undirected edge carries exactly one face, in ascending (face, corner) order, and their loops:
    the connected components through shared vertices, numbered in ascending order of their smallest vertex.  A loop is simple when
    every vertex on it has one outgoing and one incoming boundary edge: one closed polygon.  -> dict of edges (B,2) int32,
    edge_face (B,) int32, edge_loop (B,) int32, n_edges, n_loops, n_simple, loop_edges (L,) int32, loop_simple (L,) bool, loop_vert
    (L,) int32 (the loop's smallest vertex).  One host synchronisation (the counts)."""
    n_verts, faces = _mesh_args(verts_or_n_verts, faces, "boundary_loops")
    with torch.no_grad():
        edges, edge_face, edge_loop, loop_edges, loop_simple, loop_vert, counts = _cc_backend(faces).mesh_boundary_loops(
            faces, n_verts, adjacency=None if adjacency is None else tuple(adjacency))
        B, L, n_simple = counts.tolist()                                        # the host synchronisation
    return {"edges": edges[:B], "edge_face": edge_face[:B], "edge_loop": edge_loop[:B], "n_edges": B, "n_loops": L,
            "n_simple": n_simple, "loop_edges": loop_edges[:L], "loop_simple": loop_simple[:L].bool(), "loop_vert": loop_vert[:L]}


def fill_holes(verts, faces, max_edges=64, attributes=None, adjacency=None):
    """Close the small holes of an indexed mesh (hip.mesh_fill_holes on the GPU, meshing.mesh_fill_holes on the host, equal bit for
    bit).  A boundary loop is filled when it is simple and has between 3 and max_edges edges: one new vertex at the exact mean of
    the loop's vertices, appended after the existing ones, and one face (b, a, new) per boundary edge a->b, appended after the
    existing ones, consistent with the face that owns the edge.  Nothing existing is renumbered.  Larger loops, loops that are not
    simple (two holes touching at a vertex, a hole in a misoriented neighbourhood: run `orient_mesh` first) and loops with a
    non-finite vertex are left alone and counted.  -> dict of verts (V',3) float32, faces (F',3) in the dtype of `faces`,
    n_verts, n_tris, vert_src (V',) int64 (an old vertex: itself; a new one: the smallest vertex of its loop), filled = dict of
    loops / faces / skipped_loops, and every tensor of the dict `attributes` (first dimension V) gathered by vert_src -- never
    averaged.  Host synchronisations: the vertices' bounds and the sizes of the result."""
    from . import meshing
    meshing.check_max_edges(max_edges, "fill_holes")
    n_verts, faces = _mesh_args(verts, faces, "fill_holes")
    _check_mesh_verts(verts, faces, "fill_holes")
    attributes = _repair_attributes(attributes, n_verts, verts.device, ("verts", "faces", "n_verts", "n_tris", "vert_src", "filled"),
                                    "fill_holes")
    with torch.no_grad():
        v32 = verts.detach().to(torch.float32).contiguous()
        verts_out, vert_src, faces_out, _, counts = _cc_backend(faces).mesh_fill_holes(
            v32, faces, max_edges=max_edges, adjacency=None if adjacency is None else tuple(adjacency))
        _, L, _, Lf, Bf = counts.tolist()                                       # the host synchronisation
        F = int(faces.shape[0])
        vert_src = vert_src[:n_verts + Lf].long()
        res = {"verts": verts_out[:n_verts + Lf], "faces": torch.cat([faces, faces_out[F:F + Bf].to(faces.dtype)]),
               "n_verts": n_verts + Lf, "n_tris": F + Bf, "vert_src": vert_src,
               "filled": {"loops": Lf, "faces": Bf, "skipped_loops": L - Lf}}
        for name, t in attributes.items():
            res[name] = t.index_select(0, vert_src)
    return res


def repair_mesh(verts, faces, policy="majority", max_edges=64, attributes=None):
    """`orient_mesh`, then `fill_holes` of the oriented mesh: -> the dict of `fill_holes` plus topology (`mesh_topology` of the
    result) and oriented (the report of `orient_mesh` without its faces).  The adjacency is built once for the orientation and
    once for the filling: the flips change the directions it counts."""
    if attributes and ("topology" in attributes or "oriented" in attributes):
        raise ValueError("repair_mesh: an attribute cannot be called 'topology' or 'oriented'")
    oriented = orient_mesh(verts, faces, policy=policy)
    res = fill_holes(verts, oriented.pop("faces"), max_edges=max_edges, attributes=attributes)
    res["topology"] = mesh_topology(res["verts"], res["faces"])
    res["oriented"] = oriented
    return res


def _intersections(verts, faces, group, between, max_pairs, what):
    """The backend's `mesh_intersections` and the counts on the host: -> (hits, vert_hit, pairs (n,2), the five counts)."""
    from . import meshing
    meshing.check_max_pairs(max_pairs, what)
    _mesh_args(verts, faces, what)
    _check_mesh_verts(verts, faces, what)
    with torch.no_grad():
        v32 = verts.detach().to(torch.float32).contiguous()
        if faces.is_cuda:
            from . import hip
            hits, vert_hit, _, pairs, counts = hip.mesh_intersections(v32, faces, group=group, between=between, max_pairs=max_pairs, trim=False)
        else:
            hits, vert_hit, _, pairs, counts = meshing.mesh_intersections(v32, faces, group=group, between=between, max_pairs=max_pairs)
        c = counts.tolist()                                                     # the host synchronisation
        if c[0] < 0:
            raise ValueError("%s: more than 2^31 - 1 pairs do not fit an int32 count" % what)
    return hits, vert_hit, pairs[:c[4]], c


def self_intersections(verts, faces, max_pairs=1 << 20, return_pairs=True):
    """Is the indexed mesh EMBEDDED -- or do some of its faces cut through each other?  (hip.mesh_intersections on the GPU,
    meshing.mesh_intersections on the host, equal bit for bit; the rule is stated in meshing.mesh_intersections.)  Exact in
    integers on a 2^18 lattice over the vertices' bounds: two faces intersect when an edge of one properly crosses the other.  Faces
    that share a vertex or an edge are reported only when they fold through each other; duplicates, touching contact and coplanar
    overlap are not intersections; a degenerate face can cut and cannot be cut; a face with an id out of range or a non-finite
    vertex is void.  `mesh_topology` says whether a mesh is manifold and watertight; this says whether it bounds a solid without
    passing through itself, which the parity rule of `mesh_contains`, `voxelize`, `mesh_iou` and `mesh_sdf` assumes -- `remesh`
    repairs a mesh that is not.  -> dict of count (the pairs), faces_hit, verts_hit, void_faces, hits (F,) int32 (the faces each face
    intersects), vert_hit (V,) uint8 (1 on the corners of the faces hit: an attribute for `render_mesh`), pairs (n,2) int32 (f < g,
    ordered by f then g; the first max_pairs of them; None without return_pairs), truncated (count > n) and embedded (count == 0).
    Host synchronisations: the vertices' bounds and the counts."""
    if not isinstance(return_pairs, bool):
        raise ValueError("self_intersections: return_pairs must be True or False, got %r" % (return_pairs,))
    hits, vert_hit, pairs, c = _intersections(verts, faces, None, False, max_pairs if return_pairs else 0, "self_intersections")
    return {"count": c[0], "faces_hit": c[1], "verts_hit": c[2], "void_faces": c[3], "hits": hits, "vert_hit": vert_hit,
            "pairs": pairs if return_pairs else None, "truncated": bool(return_pairs and c[0] > c[4]), "embedded": c[0] == 0}


def mesh_intersections(mesh_a, mesh_b, max_pairs=1 << 20, return_pairs=True):
    """Which faces of mesh_a cut through faces of mesh_b: a posed body against a scan or a prop, frame t against frame t + 1.  Both
    are (verts (V,3), faces (F,3)) on one device.  The two meshes are concatenated, labelled 0 / 1 and quantised over their joint
    bounds, and only pairs from different meshes count (the rule of `self_intersections`; a mesh's own folds are not reported).  ->
    dict of count, faces_hit_a / faces_hit_b, void_faces, hits_a (F_a,) / hits_b (F_b,) int32, vert_hit_a (V_a,) / vert_hit_b (V_b,)
    uint8, pairs (n,2) int32 (face of a, face of b; ordered by the face of a, then of b; None without return_pairs), truncated and
    disjoint (count == 0: the SURFACES do not meet; one mesh may still lie inside the other)."""
    what = "mesh_intersections"
    if not isinstance(return_pairs, bool):
        raise ValueError("%s: return_pairs must be True or False, got %r" % (what, return_pairs))
    for m in (mesh_a, mesh_b):
        if not isinstance(m, (tuple, list)) or len(m) != 2 or not all(isinstance(t, torch.Tensor) for t in m):
            raise ValueError("%s: a mesh is (verts (V, 3), faces (F, 3))" % what)
        _mesh_args(m[0], m[1], what)
        if m[0].dim() != 2 or not m[0].dtype.is_floating_point:
            raise ValueError("%s: verts must be a floating-point (V, 3) tensor" % what)
        if m[1].dim() != 2 or m[1].shape[1] != 3 or m[1].dtype.is_floating_point or m[1].dtype == torch.bool:
            raise ValueError("%s: faces must be an (F, 3) tensor of integer ids" % what)
    (va, fa), (vb, fb) = mesh_a, mesh_b
    if len({va.device, fa.device, vb.device, fb.device}) != 1:
        raise ValueError("%s: both meshes must live on one device" % what)
    Va, Fa, Vb = int(va.shape[0]), int(fa.shape[0]), int(vb.shape[0])
    with torch.no_grad():
        fa64, fb64 = fa.long(), fb.long()
        # an id out of its own mesh's range must stay out of range in the joint mesh
        fb64 = torch.where((fb64 >= 0) & (fb64 < Vb), fb64 + Va, torch.full_like(fb64, -1))
        fa64 = torch.where((fa64 >= 0) & (fa64 < Va), fa64, torch.full_like(fa64, -1))
        verts = torch.cat([va.detach().to(torch.float32), vb.detach().to(torch.float32)])
        faces = torch.cat([fa64, fb64])
        group = torch.cat([torch.zeros(Fa, dtype=torch.uint8, device=fa.device), torch.ones(int(fb.shape[0]), dtype=torch.uint8, device=fa.device)])
    hits, vert_hit, pairs, c = _intersections(verts, faces, group, True, max_pairs if return_pairs else 0, what)
    if return_pairs:
        pairs = torch.stack([pairs[:, 0], pairs[:, 1] - Fa], 1)                   # f < g and different groups: f in a, g in b
    return {"count": c[0], "faces_hit_a": int((hits[:Fa] > 0).sum()), "faces_hit_b": int((hits[Fa:] > 0).sum()), "void_faces": c[3],
            "hits_a": hits[:Fa], "hits_b": hits[Fa:], "vert_hit_a": vert_hit[:Va], "vert_hit_b": vert_hit[Va:],
            "pairs": pairs if return_pairs else None, "truncated": bool(return_pairs and c[0] > c[4]), "disjoint": c[0] == 0}


def check_smooth(smooth):
    """Validate a `smooth` option of the model's mesh entries and return the keywords of `smooth_mesh` it stands for: None
    (nothing), a number of iterations (an integer >= 0), or a dict of iterations / lamb / mu / method / boundary / weights / time
    ({"method": "implicit", "time": t} is implicit fairing).  ValueError for anything else."""
    from . import meshing
    if smooth is None:
        return None
    if isinstance(smooth, dict):
        kw = dict(smooth)
        bad = set(kw) - set(_SMOOTH_KEYS)
        if bad:
            raise ValueError("smooth: unknown keys %s (known: %s)" % (sorted(bad, key=str), ", ".join(_SMOOTH_KEYS)))
    elif isinstance(smooth, (int, np.integer)) and not isinstance(smooth, bool):
        kw = {"iterations": int(smooth)}
    else:
        raise ValueError("smooth must be None, a number of iterations or a dict of smooth_mesh keywords, got %r" % (smooth,))
    _check_smooth_call(kw.get("iterations", 10), kw.get("lamb", 0.5), kw.get("mu", -0.53), kw.get("method", "taubin"),
                       kw.get("boundary", "pin"), "smooth", kw.get("weights", "uniform"), kw.get("time"))
    return kw


# ---- drawing indexed meshes ---------------------------------------------------------------------------------------------
_CAMERA_OPENCV = ("cam_rot", "cam_trans", "K")
_CAMERA_LOOKAT = ("azim", "dist", "fov", "at")
_BUILTIN_ATTRIBUTES = ("vertex_normal", "face_normal")


def check_camera(camera, what="render_mesh"):
    """The `camera` of `render_mesh`: -> "opencv" for {"cam_rot" (3,3), "cam_trans" (3,), "K" (3,3)} (all three), "lookat" for
    {"azim" degrees[, "dist" 2.0, "fov" 60 degrees, "at" the point looked at: three numbers or a tensor of three, default the
    origin]}.  ValueError for anything else, keys of both kinds included."""
    if not isinstance(camera, dict) or not camera:
        raise ValueError("%s: camera must be a dict of cam_rot / cam_trans / K or of azim [/ dist / fov], got %r" % (what, camera))
    keys = set(camera)
    if keys == set(_CAMERA_OPENCV):
        for k, n in (("cam_rot", 9), ("cam_trans", 3), ("K", 9)):
            t = camera[k]
            if not isinstance(t, torch.Tensor) or not t.dtype.is_floating_point or t.numel() != n:
                raise ValueError("%s: camera[%r] must be a floating-point tensor of %d elements" % (what, k, n))
        return "opencv"
    if "azim" in keys and keys <= set(_CAMERA_LOOKAT):
        at = camera.get("at")
        if at is not None and not (isinstance(at, torch.Tensor) and at.dtype.is_floating_point and at.numel() == 3):
            if not isinstance(at, (tuple, list)) or len(at) != 3 or any(
                    isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or not np.isfinite(float(x)) for x in at):
                raise ValueError("%s: camera['at'] must be three finite numbers or a floating-point tensor of three, got %r" % (what, at))
        for k in keys - {"at"}:
            x = camera[k]
            if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or not np.isfinite(float(x)):
                raise ValueError("%s: camera[%r] must be a finite number, got %r" % (what, k, x))
        if not float(camera.get("dist", 2.0)) > 0.0 or not 0.0 < float(camera.get("fov", 60.0)) < 180.0:
            raise ValueError("%s: camera dist must be > 0 and fov in (0, 180) degrees" % what)
        return "lookat"
    raise ValueError("%s: camera must hold exactly cam_rot, cam_trans and K, or azim with optional dist, fov and at; got the keys %s"
                     % (what, sorted(keys, key=str)))


def _rows_times(pts, M):
    """pts (V,3) @ M (3,3) with the sum written out, (x m0 + y m1) + z m2 per column, every operation rounded on its own: the same
    bits on the host and on the device, which a matrix product does not promise."""
    x, y, z = pts[:, 0:1], pts[:, 1:2], pts[:, 2:3]
    return (x * M[0][None, :] + y * M[1][None, :]) + z * M[2][None, :]


def project_mesh(verts, camera, height, width):
    """verts (V,3) float32 through `camera` (check_camera) -> (V,3) (u, v, view depth) in the pixels of a height x width image: the
    formulas of meshing.project_opencv / project_lookat with the products summed in a fixed order (host and device agree bit for
    bit).  A look-at view of an image that is not square fits the shorter side, like pytorch3d."""
    from . import meshing
    kind = check_camera(camera)
    dev = verts.device
    if kind == "opencv":
        R = camera["cam_rot"].detach().to(dev, torch.float32).reshape(3, 3)
        t = camera["cam_trans"].detach().to(dev, torch.float32).reshape(3)
        K = camera["K"].detach().to(dev, torch.float32).reshape(3, 3)
        xc = _rows_times(verts, R.t()) + t[None, :]
        z = xc[:, 2]
        return torch.stack([K[0, 0] * xc[:, 0] / z + K[0, 2], K[1, 1] * xc[:, 1] / z + K[1, 2], z], dim=1)
    cam, R = meshing._lookat(dev, float(camera["azim"]), float(camera.get("dist", 2.0)))
    at = camera.get("at")
    if at is not None:   # the camera keeps its offset and its axes, and moves with the point it looks at
        at = at.detach().to(dev, torch.float32).reshape(3) if isinstance(at, torch.Tensor) else \
            torch.tensor([float(x) for x in at], dtype=torch.float32, device=dev)
        cam = cam + at
    xv = _rows_times(verts - cam[None, :], R)
    f = 1.0 / math.tan(math.radians(float(camera.get("fov", 60.0))) / 2.0)
    z, side = xv[:, 2], min(height, width)
    u = (1.0 - f * xv[:, 0] / z) * side / 2.0 + (width - side) / 2.0
    v = (1.0 - f * xv[:, 1] / z) * side / 2.0 + (height - side) / 2.0
    return torch.stack([u, v, z], dim=1)


def face_normals(verts, faces):
    """Unit right-hand normals (F,3) float32 of the faces of an indexed mesh, (p1 - p0) x (p2 - p0) normalised in float64 with every
    operation rounded on its own; (0, 0, 0) for a face with an id out of range, a non-finite corner or no area."""
    V, f64 = int(verts.shape[0]), torch.float64
    faces = faces.long()
    if V == 0 or faces.shape[0] == 0:
        return torch.zeros(faces.shape[0], 3, dtype=torch.float32, device=verts.device)
    p = verts.to(f64)[faces.clamp(0, V - 1)]
    a, b = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    n = torch.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], dim=1)
    length = torch.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    ok = ((faces >= 0) & (faces < V)).all(1) & torch.isfinite(length) & (length > 0)
    unit = n / torch.where(ok, length, torch.ones_like(length))[:, None]
    return torch.where(ok[:, None], unit, torch.zeros_like(unit)).float()


def surface_centroid(verts, faces):
    """The centroid (3,) float32 of the SURFACE of an indexed mesh: the faces' centres weighted with their areas, in float64; faces
    with an id out of range or a non-finite corner are left out, and a mesh without area gives the origin.  Unlike the mean of the
    vertices it does not depend on how finely a part is tessellated, and unlike the centre of the bounding box it is where the bulk
    of the surface is.  On the mesh's device, no host synchronisation."""
    V, f64 = int(verts.shape[0]), torch.float64
    faces = faces.long()
    if V == 0 or faces.shape[0] == 0:
        return torch.zeros(3, dtype=torch.float32, device=verts.device)
    p = verts.to(f64)[faces.clamp(0, V - 1)]
    area = torch.linalg.vector_norm(torch.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], dim=1), dim=1)
    ok = ((faces >= 0) & (faces < V)).all(1) & torch.isfinite(area)
    area = torch.where(ok, area, torch.zeros_like(area))
    centre = torch.where(ok[:, None], p.mean(1), torch.zeros_like(p[:, 0]))
    c = (area[:, None] * centre).sum(0) / area.sum()
    return torch.where(torch.isfinite(c), c, torch.zeros_like(c)).float()


def render_mesh(verts, faces, height, width, camera=None, attributes=None, cull="none", z_near=1e-4, background=0.0):
    """Draw an indexed mesh: verts (V,3) world (or canonical) coordinates, faces (F,3) integer ids, through `camera` --
    {"cam_rot" (3,3), "cam_trans" (3,), "K" (3,3)}, an OpenCV camera as the frames carry it (meshing.project_opencv), or {"azim"
    degrees[, "dist" 2.0, "fov" 60, "at" the point looked at, default the origin]}, pytorch3d's look-at view of the canonical maps
    (meshing.project_lookat) -- into a height x
    width image, one face per pixel, the nearest.  The rule is meshing.mesh_rasterize: watertight along shared edges,
    perspective-correct depth and barycentrics, faces at or behind z_near dropped whole; cull="back" / "front" drops the faces
    whose projected area2 is negative / positive.

    attributes: a dict name -> (V,C) float tensor, 1 <= C <= 32, of per-vertex values to interpolate.  The names "vertex_normal"
    and "face_normal" may be given as True: the mesh's own normals (geometry.vertex_normals, interpolated -- NOT renormalised; and
    the faces' unit cross products, flat: gathered by pix_to_face).  -> a dict of tensors on the mesh's device: pix_to_face (H,W)
    int32 (-1: nothing), depth (H,W) float32 view depth (-1), bary (H,W,3) float32 (-1), mask (H,W) bool, and one (H,W,C) float32
    image per attribute with `background` where nothing is drawn.  hip.mesh_rasterize / hip.mesh_interpolate for a mesh on the GPU
    (no host synchronisation), their specification in meshing for one on the host, equal bit for bit."""
    from . import meshing
    if not isinstance(verts, torch.Tensor) or verts.dim() != 2 or verts.shape[1] != 3 or not verts.dtype.is_floating_point:
        raise ValueError("render_mesh: verts must be a floating-point (V, 3) tensor")
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError("render_mesh: faces must be an (F, 3) tensor")
    if faces.dtype.is_floating_point or faces.dtype.is_complex or faces.dtype == torch.bool:
        raise ValueError("render_mesh: faces must hold integer vertex ids")
    if verts.device != faces.device:
        raise ValueError("render_mesh: verts live on %s, faces on %s" % (verts.device, faces.device))
    for name, x in (("height", height), ("width", width)):
        if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or int(x) < 1:
            raise ValueError("render_mesh: %s must be an integer >= 1, got %r" % (name, x))
    if cull not in meshing.RASTER_CULL:
        raise ValueError("render_mesh: cull must be 'none', 'back' or 'front', got %r" % (cull,))
    check_camera(camera)
    V, dev = int(verts.shape[0]), verts.device
    attributes = dict(attributes or {})
    for name, a in attributes.items():
        if a is True and name in _BUILTIN_ATTRIBUTES:
            continue
        if name in ("pix_to_face", "depth", "bary", "mask"):
            raise ValueError("render_mesh: an attribute cannot be called %r" % name)
        if not isinstance(a, torch.Tensor) or a.dim() != 2 or not a.dtype.is_floating_point or not 1 <= int(a.shape[1]) <= 32:
            raise ValueError("render_mesh: attribute %r must be a floating-point (V, C) tensor with 1 <= C <= 32%s"
                             % (name, " (True only for %s)" % " / ".join(_BUILTIN_ATTRIBUTES) if a is True else ""))
        if int(a.shape[0]) != V:
            raise ValueError("render_mesh: attribute %r has %d rows, the mesh %d vertices" % (name, int(a.shape[0]), V))
        if a.device != dev:
            raise ValueError("render_mesh: attribute %r lives on %s, the mesh on %s" % (name, a.device, dev))
    height, width = int(height), int(width)
    backend = _cc_backend(faces)
    rasterize = backend.mesh_rasterize
    interpolate = backend.mesh_interpolate if faces.is_cuda else backend.interpolate_attributes
    with torch.no_grad():
        v32 = verts.detach().to(torch.float32).contiguous()
        uvz = project_mesh(v32, camera, height, width)
        p2f, depth, bary = rasterize(uvz, faces, height, width, z_near=z_near, cull=cull)
        res = {"pix_to_face": p2f, "depth": depth, "bary": bary, "mask": p2f >= 0}
        for name, a in attributes.items():
            if a is True and name == "face_normal":
                n = face_normals(v32, faces)
                fill = torch.full((), float(background), dtype=torch.float32, device=dev)
                res[name] = torch.where(res["mask"][..., None], n[p2f.long().clamp_min(0)], fill) if n.shape[0] else \
                    fill.expand(height, width, 3).clone()
                continue
            if a is True:
                a = vertex_normals(v32, faces)
            res[name] = interpolate(p2f, bary, faces, a.detach().to(torch.float32).contiguous(), background=background)
    return res


# ---- casting rays against meshes (DESIGN.md "Casting rays against meshes on the device") ---------------------------------
def _ray_args(origins, dirs, dev, what):
    for name, x in (("origins", origins), ("dirs", dirs)):
        if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[1] != 3 or not x.dtype.is_floating_point:
            raise ValueError("%s: %s must be a floating-point (R, 3) tensor" % (what, name))
        if x.device != dev:
            raise ValueError("%s: %s live on %s, the mesh on %s" % (what, name, x.device, dev))
    if origins.shape[0] != dirs.shape[0]:
        raise ValueError("%s: %d origins but %d directions" % (what, origins.shape[0], dirs.shape[0]))
    return origins.detach().to(torch.float32).contiguous(), dirs.detach().to(torch.float32).contiguous()


def _ray_soup(mesh, what):
    """The soup rays are cast against: `_as_soup`, with every face of a (verts, faces) pair that names a vertex out of range
    replaced by three corners at 0 -- a face without area, which no ray hits (its det is exactly 0) --, as mesh_components,
    face_normals and the interpolation skip such a face.  No host synchronisation."""
    tris, _ = _as_soup(mesh, what)
    if isinstance(mesh, (tuple, list)):
        faces = torch.as_tensor(mesh[1]).to(tris.device).long()
        ok = ((faces >= 0) & (faces < int(torch.as_tensor(mesh[0]).shape[0]))).all(1)
        tris = torch.where(ok[:, None, None], tris, torch.zeros_like(tris)).contiguous()
    return tris


def _ray_index(tris, index, what):
    from . import hip
    if index is None:
        return hip.mesh_index(tris)
    if not isinstance(index, hip.MeshIndex) or index.tris.shape != tris.shape or index.tris.device != tris.device:
        raise ValueError("%s: index must be the hip.mesh_index of this mesh's soup" % what)
    return index


def cast_rays(mesh, origins, dirs, t_min=0.0, t_max=float("inf"), cull="none", attributes=None, index=None):
    """What the rays origins + t dirs ((R,3) each; dirs need not be unit, t is in units of |dirs|) see first of a mesh -- an (F,3,3)
    soup or a (verts, faces) pair as in `mesh_metrics`.  The rule is meshing.mesh_raycast: watertight (a ray through a shared edge
    or vertex hits one of the faces), float64 on the float32 inputs, the nearest hit with t_min <= t <= t_max, the lowest face id on
    a tie; cull="back" drops the hits a ray makes running ALONG a face's normal (b-a)x(c-a), "front" those against it.
    -> a dict of tensors on the mesh's device: hit (R,) bool, t (R,) float64 (+inf on a miss), face (R,) int32 (-1), bary (R,3)
    float64 (0), points (R,3) float64 the barycentric combination of the face's corners (0), normal (R,3) float32 the face's unit
    normal (0), and one (R,C) float32 tensor per attribute (0 on a miss).  attributes: as in `render_mesh`, a dict name -> (V,C)
    per-vertex tensor, "vertex_normal": True for the mesh's own normals; interpolated by the rule of meshing.interpolate_attributes
    with the rays as a 1 x R image and the barycentrics rounded to float32; they need the (verts, faces) form.  A face that names
    a vertex out of range is never hit.  index: the
    hip.mesh_index of the mesh's soup built earlier, or None.  hip.mesh_raycast for a mesh on the GPU (no host synchronisation),
    the specification for one on the host; equal bit for bit."""
    from . import meshing
    tris = _ray_soup(mesh, "cast_rays")
    dev = tris.device
    o, d = _ray_args(origins, dirs, dev, "cast_rays")
    t_min, t_max, _ = meshing.check_raycast_args(tris, o, d, t_min, t_max, cull, "cast_rays")
    indexed = isinstance(mesh, (tuple, list))
    attributes = dict(attributes or {})
    if attributes and not indexed:
        raise ValueError("cast_rays: attributes are per vertex and need the (verts, faces) form of the mesh")
    if indexed:
        verts, faces = torch.as_tensor(mesh[0]).detach().to(torch.float32).contiguous(), torch.as_tensor(mesh[1]).to(dev)
        V = int(verts.shape[0])
    for name, a in attributes.items():
        if a is True and name == "vertex_normal":
            continue
        if name in ("hit", "t", "face", "bary", "points", "normal"):
            raise ValueError("cast_rays: an attribute cannot be called %r" % name)
        if not isinstance(a, torch.Tensor) or a.dim() != 2 or not a.dtype.is_floating_point or not 1 <= int(a.shape[1]) <= 32:
            raise ValueError("cast_rays: attribute %r must be a floating-point (V, C) tensor with 1 <= C <= 32%s"
                             % (name, " (True only for vertex_normal)" if a is True else ""))
        if int(a.shape[0]) != V or a.device != dev:
            raise ValueError("cast_rays: attribute %r must have one row per vertex (%d) on the mesh's device" % (name, V))
    with torch.no_grad():
        if tris.is_cuda:
            from . import hip
            t, face, bary, _ = hip.mesh_raycast(_ray_index(tris, index, "cast_rays"), o, d, t_min, t_max, cull)
        else:
            if index is not None:
                raise ValueError("cast_rays: an index belongs to a mesh on the GPU")
            t, face, bary = meshing.mesh_raycast(tris, o, d, t_min, t_max, cull)
        hit = face >= 0
        corners = tris.double()[face.long().clamp_min(0)]                                        # (R,3,3)
        points = (bary[:, 0:1] * corners[:, 0] + bary[:, 1:2] * corners[:, 1]) + bary[:, 2:3] * corners[:, 2]
        points = torch.where(hit[:, None], points, torch.zeros_like(points))
        soup_faces = torch.arange(3 * tris.shape[0], device=dev).reshape(-1, 3)
        normal = face_normals(tris.reshape(-1, 3), soup_faces)[face.long().clamp_min(0)]
        normal = torch.where(hit[:, None], normal, torch.zeros_like(normal))
        res = {"hit": hit, "t": t, "face": face, "bary": bary, "points": points, "normal": normal}
        if attributes:
            interpolate = _cc_backend(faces).mesh_interpolate if tris.is_cuda else meshing.interpolate_attributes
            R = int(o.shape[0])
            for name, a in attributes.items():
                if a is True:
                    a = vertex_normals(verts, faces)
                a = a.detach().to(torch.float32).contiguous()
                if R == 0:
                    res[name] = torch.zeros(0, a.shape[1], dtype=torch.float32, device=dev)
                    continue
                res[name] = interpolate(face.reshape(1, R), bary.to(torch.float32).reshape(1, R, 3), faces, a, background=0.0)[0]
    return res


def occluded(mesh, origins, dirs, t_min, t_max, index=None):
    """(R,) bool: whether anything of the mesh (as in `cast_rays`) meets the ray origins + t dirs within t_min <= t <= t_max -- for a
    segment from p to q: origins p, dirs q - p, t in [0, 1].  hip.mesh_raycast(mode="any") on the GPU, which stops at the first
    accepted face; the specification's face >= 0 on the host; the same answer."""
    from . import meshing
    tris = _ray_soup(mesh, "occluded")
    o, d = _ray_args(origins, dirs, tris.device, "occluded")
    t_min, t_max, _ = meshing.check_raycast_args(tris, o, d, t_min, t_max, "none", "occluded")
    with torch.no_grad():
        if tris.is_cuda:
            from . import hip
            return hip.mesh_raycast(_ray_index(tris, index, "occluded"), o, d, t_min, t_max, mode="any")[0]
        if index is not None:
            raise ValueError("occluded: an index belongs to a mesh on the GPU")
        return meshing.mesh_raycast(tris, o, d, t_min, t_max)[1] >= 0


def vertex_visibility(verts, faces, eye, eps=1e-4):
    """(V,) bool: which vertices of the indexed mesh a point `eye` (three numbers or a tensor of three) sees.  A vertex is visible
    when the segment from the vertex, moved by eps along its own vertex normal (`vertex_normals`) so that its own faces do not
    hide it, to the eye meets no face.  The normals must point OUT of the body: the level sets of `posed_mesh` / `canonical_mesh` are
    wound the other way ("Normals") -- pass faces.flip(1) for them."""
    v32, faces, _ = _smooth_args(verts, faces, None, "vertex_visibility")
    eye = eye.detach().to(v32.device, torch.float32).reshape(-1) if isinstance(eye, torch.Tensor) else \
        torch.tensor([float(x) for x in eye], dtype=torch.float32, device=v32.device)
    if eye.numel() != 3:
        raise ValueError("vertex_visibility: eye must be a point, three numbers")
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not eps >= 0.0:
        raise ValueError("vertex_visibility: eps must be a number >= 0, got %r" % (eps,))
    with torch.no_grad():
        start = v32 + float(eps) * vertex_normals(v32, faces)
        return ~occluded((v32, faces), start, eye[None, :] - start, 0.0, 1.0)


def camera_rays(camera, height, width):
    """The rays through the pixel centres (j + 0.5, i + 0.5) of a height x width image of `camera` (check_camera), row by row: ->
    origins, dirs (H W, 3) float32 on the camera tensors' device (the host for a look-at camera of numbers).  A direction has
    view depth 1 -- it is NOT unit --, so the t of `cast_rays` along it is the view depth `render_mesh` draws, and
    project_mesh(origin + dir) is the pixel centre."""
    from . import meshing
    kind = check_camera(camera, "camera_rays")
    for name, x in (("height", height), ("width", width)):
        if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or int(x) < 1:
            raise ValueError("camera_rays: %s must be an integer >= 1, got %r" % (name, x))
    H, W = int(height), int(width)
    f64 = torch.float64
    if kind == "opencv":
        dev = camera["K"].device
        R = camera["cam_rot"].detach().to(dev, f64).reshape(3, 3)
        t = camera["cam_trans"].detach().to(dev, f64).reshape(3)
        K = camera["K"].detach().to(dev, f64).reshape(3, 3)
    else:
        at = camera.get("at")
        dev = at.device if isinstance(at, torch.Tensor) else torch.device("cpu")
    u = (torch.arange(W, dtype=f64, device=dev) + 0.5)[None, :].expand(H, W).reshape(-1)
    v = (torch.arange(H, dtype=f64, device=dev) + 0.5)[:, None].expand(H, W).reshape(-1)
    if kind == "opencv":
        x_cam = torch.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], torch.ones_like(u)], dim=1)
        dirs = x_cam @ R                     # R^T x_cam per row
        origin = -(R.t() @ t)
    else:
        cam, R = meshing._lookat(dev, float(camera["azim"]), float(camera.get("dist", 2.0)))
        cam, R = cam.to(f64), R.to(f64)
        if at is not None:
            cam = cam + (at.detach().to(dev, torch.float32).reshape(3) if isinstance(at, torch.Tensor) else
                         torch.tensor([float(x) for x in at], dtype=torch.float32, device=dev)).to(f64)
        f = 1.0 / math.tan(math.radians(float(camera.get("fov", 60.0))) / 2.0)
        side = min(H, W)
        xv = torch.stack([(1.0 - (u - (W - side) / 2.0) * 2.0 / side) / f, (1.0 - (v - (H - side) / 2.0) * 2.0 / side) / f,
                          torch.ones_like(u)], dim=1)
        dirs = xv @ R.t()                    # the columns of R are the view axes
        origin = cam
    return origin.to(torch.float32)[None, :].expand(H * W, 3).contiguous(), dirs.to(torch.float32).contiguous()


_AO_TABLES = {}


def ao_directions(n_rays, seed):
    """The fixed table of `ambient_occlusion`: (n_rays, 3) float64 on the host, unit directions about +z with a density
    proportional to the cosine (Malley: a uniform disc lifted onto the hemisphere), from torch's CPU generator seeded with `seed`."""
    key = (int(n_rays), int(seed))
    if key not in _AO_TABLES:
        g = torch.Generator().manual_seed(int(seed))
        u = torch.rand(int(n_rays), 2, generator=g, dtype=torch.float64)
        r, phi = torch.sqrt(u[:, 0]), 2.0 * math.pi * u[:, 1]
        _AO_TABLES[key] = torch.stack([r * torch.cos(phi), r * torch.sin(phi), torch.sqrt(1.0 - u[:, 0])], dim=1)
    return _AO_TABLES[key]


def ambient_occlusion(verts, faces, n_rays=64, seed=0, radius=float("inf"), eps=1e-4, adjacency=None):
    """(V,) float32 in [0, 1]: the share of n_rays directions about every vertex's normal in which the mesh does not hide the sky
    within `radius` -- 1 on a convex body, less in folds and armpits.  The directions are those of `ao_directions(n_rays, seed)`
    turned into the frame of the vertex's normal (`vertex_normals`; adjacency as there), the rays start eps along the normal, and
    ONE any-hit query (`occluded`) answers all V n_rays of them.  The frame is built in float64 from operations that round the
    same way on the host and on the device, and the count of open directions is an integer: host and device agree exactly.  A
    vertex without a normal gets 1.  The normals must point OUT of the body: for the level sets of `posed_mesh` / `canonical_mesh`,
    which are wound the other way ("Normals"), pass faces.flip(1), as model.render_mesh does."""
    v32, faces, adjacency = _smooth_args(verts, faces, adjacency, "ambient_occlusion")
    if isinstance(n_rays, bool) or not isinstance(n_rays, (int, np.integer)) or not 1 <= int(n_rays) <= 4096:
        raise ValueError("ambient_occlusion: n_rays must be an integer in [1, 4096], got %r" % (n_rays,))
    if isinstance(radius, bool) or not isinstance(radius, (int, float)) or not radius > 0.0:
        raise ValueError("ambient_occlusion: radius must be a number > 0, got %r" % (radius,))
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not eps >= 0.0:
        raise ValueError("ambient_occlusion: eps must be a number >= 0, got %r" % (eps,))
    V, dev, n_rays = int(v32.shape[0]), v32.device, int(n_rays)
    if V * n_rays > 2 ** 31 - 1:
        raise ValueError("ambient_occlusion: at most 2^31 - 1 rays")
    if V == 0 or faces.shape[0] == 0:
        return torch.ones(V, dtype=torch.float32, device=dev)
    with torch.no_grad():
        start, dirs = ao_rays(v32, faces, n_rays, seed, float(eps), adjacency)
        hidden = occluded((v32, faces), start, dirs, 0.0, float(radius))
        open_count = n_rays - hidden.reshape(V, n_rays).sum(1)
        return open_count.to(torch.float32) / float(n_rays)


def ao_rays(v32, faces, n_rays, seed, eps, adjacency=None):
    """The rays of `ambient_occlusion`: -> origins, dirs (V n_rays, 3) float32, vertex by vertex."""
    V, dev = int(v32.shape[0]), v32.device
    n32 = vertex_normals(v32, faces, adjacency=adjacency)
    n = n32.double()
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    # a tangent: e x n with e the axis the normal is least along, normalised; the other: n x tangent
    use_x = (nx.abs() <= ny.abs()) & (nx.abs() <= nz.abs())
    use_y = ~use_x & (ny.abs() <= nz.abs())
    zero = torch.zeros_like(nx)
    tx = torch.where(use_x, zero, torch.where(use_y, nz, -ny))
    ty = torch.where(use_x, -nz, torch.where(use_y, zero, nx))
    tz = torch.where(use_x, ny, torch.where(use_y, -nx, zero))
    length = torch.sqrt((tx * tx + ty * ty) + tz * tz)
    tx, ty, tz = tx / length, ty / length, tz / length
    bx, by, bz = ny * tz - nz * ty, nz * tx - nx * tz, nx * ty - ny * tx
    tab = ao_directions(n_rays, seed).to(dev)
    dx, dy, dz = tab[None, :, 0], tab[None, :, 1], tab[None, :, 2]
    dirs = torch.stack([(dx * tx[:, None] + dy * bx[:, None]) + dz * nx[:, None],
                        (dx * ty[:, None] + dy * by[:, None]) + dz * ny[:, None],
                        (dx * tz[:, None] + dy * bz[:, None]) + dz * nz[:, None]], dim=2).to(torch.float32)   # (V,n,3)
    start = (v32 + float(eps) * n32)[:, None, :].expand(V, n_rays, 3)
    return start.reshape(-1, 3), dirs.reshape(-1, 3)


# ---- containment, occupancy grids and IoU (DESIGN.md "Containment, occupancy grids and IoU on the device") -----------------
IOU_KEYS = ("iou", "n_a", "n_b", "n_both", "n_either", "ambiguous_a", "ambiguous_b", "volume_a", "volume_b")


def _contains_mesh(mesh, what):
    """A soup (F,3,3) or a (verts, faces) pair -> (verts (V,3) float32, faces (F,3) int32) on the mesh's device, the soup as three
    vertices per face.  Face ids are not checked here: a face naming a vertex out of range makes the mesh degenerate for
    meshing.mesh_contains (every point outside), on the device without a host round trip."""
    if isinstance(mesh, (tuple, list)):
        if len(mesh) != 2:
            raise ValueError("%s: a mesh is an (F, 3, 3) tensor or a (verts, faces) pair" % what)
        verts, faces = torch.as_tensor(mesh[0]), torch.as_tensor(mesh[1])
        if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
            raise ValueError("%s: verts must be (V, 3) and faces (F, 3)" % what)
        if faces.dtype.is_floating_point or faces.dtype == torch.bool:
            raise ValueError("%s: faces must hold integer vertex indices" % what)
        V = max(int(verts.shape[0]), 1)
        faces = faces.to(verts.device).long().clamp(-1, V).to(torch.int32)      # out of range stays out of range in an int32
        return verts.detach().to(torch.float32).contiguous(), faces.contiguous()
    tris = torch.as_tensor(mesh)
    if tris.dim() != 3 or tuple(tris.shape[1:]) != (3, 3):
        raise ValueError("%s: a mesh is an (F, 3, 3) tensor or a (verts, faces) pair, got shape %s" % (what, tuple(tris.shape)))
    verts = tris.detach().to(torch.float32).reshape(-1, 3).contiguous()
    return verts, torch.arange(verts.shape[0], dtype=torch.int32, device=verts.device).reshape(-1, 3)


def _contains_index(verts, faces, resolution, index, what):
    from . import hip
    if index is None:
        return hip.contains_index(verts, faces, resolution)
    if (not isinstance(index, hip.ContainsIndex) or index.n_faces != int(faces.shape[0]) or index.resolution != int(resolution)
            or index.device != verts.device):
        raise ValueError("%s: index must be the hip.contains_index of this mesh at this resolution" % what)
    return index


def _is_winding_index_of(index, verts, faces, depth):
    """Whether `index` can be the hip.winding_index of this mesh: its kind, device, numbers of vertices and faces, and its depth where
    one is asked for.  The coordinates are NOT compared (that would be a host synchronisation per call): an index of another mesh
    with the same two counts on the same device is accepted and answers for that other mesh."""
    from . import hip
    return (isinstance(index, hip.WindingIndex) and index.device == verts.device and index.n_faces == int(faces.shape[0])
            and index.n_verts == int(verts.shape[0]) and (depth is None or index.depth == depth))


def _winding(verts, faces, points, accuracy, what, index=None, depth=None):
    """The winding number of float32 points against a mesh whose face ids were checked -> w (P,) float64, inside (P,) bool, n_exact,
    n_far (P,) int32, on the mesh's device: the kernels for a mesh on the GPU, the specification on the host."""
    from . import meshing
    acc = meshing.check_accuracy(accuracy, what)
    if (not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3
            or points.dtype not in (torch.float32, torch.float64)):
        raise ValueError("%s: points must be (P, 3) float32 or float64" % what)
    if points.device != verts.device:
        raise ValueError("%s: points live on %s, the mesh on %s" % (what, points.device, verts.device))
    pts = points.detach().to(torch.float32).contiguous()
    with torch.no_grad():
        if verts.is_cuda:
            from . import hip
            if index is None:
                index = hip.winding_index(verts, faces, depth)
            elif not _is_winding_index_of(index, verts, faces, depth):
                raise ValueError("%s: index must be the hip.winding_index of this mesh%s" % (
                    what, "" if depth is None else " at depth %r" % (depth,)))
            return hip.mesh_winding(index, pts, acc, want_counts=True)
        if index is not None:
            raise ValueError("%s: an index belongs to a mesh on the GPU" % what)
        tree = meshing.winding_tree(verts, faces, depth)
        w, n_exact, n_far = meshing.mesh_winding(tree, pts, acc)
        return w, meshing.winding_inside(w, tree.orient), n_exact, n_far


def winding_number(mesh, points, accuracy=3.0, depth=None, index=None, return_counts=False):
    """The generalized winding number w (P,) float64 of points (P,3) (rounded to float32) around a mesh -- an (F,3,3) soup or a
    (verts, faces) pair as in `mesh_contains`, every face id checked as in `mesh_sdf` --, on the mesh's device.  Defined for meshes
    that are NOT watertight: open sheets, holes, flipped or duplicated patches; |w| is near 1 inside, near 0 outside, and the sign
    follows the faces' orientation (meshing.winding_orient; `rule="winding"` of `mesh_contains` takes it into account).  The rule is
    meshing.winding_tree / meshing.mesh_winding: exact solid angles for near triangles, one dipole for a cluster farther than
    `accuracy` times its radius; accuracy=inf is the exact sum, depth the tree's (None: meshing.winding_depth).  index: the
    hip.winding_index of the mesh built earlier, or None (then one host synchronisation); an index is checked by its device, its
    numbers of vertices and faces and, where depth is given, its depth -- not by its coordinates.  return_counts=True -> (w, n_exact, n_far),
    the triangles summed exactly and the dipoles taken per point.  The kernels for a mesh on the GPU, the specification on the host:
    equal decisions and dipole terms, exact terms equal up to atan2's last bits."""
    verts, faces, _ = _sdf_mesh(mesh, "winding_number")
    w, _, n_exact, n_far = _winding(verts, faces, points, accuracy, "winding_number", index, depth)
    return (w, n_exact, n_far) if return_counts else w


def mesh_contains(mesh, points, resolution=512, index=None, return_ambiguous=False, rule="parity", accuracy=3.0):
    """rule="winding": inside = orient * winding number >= 0.5 (`winding_number` at `accuracy`; meant for meshes that are NOT
    watertight; every face id is checked; nothing is ambiguous; index: a hip.winding_index or None).  rule="parity", the default:

    (P,) bool: which of the points (P,3) float32 or float64 lie inside the mesh -- an (F,3,3) soup or a (verts, faces) pair as
    in `mesh_metrics`, on the points' device.  The rule is meshing.mesh_contains, the reference's check_mesh_contains with its
    triangle hash at `resolution` cells per axis: crossing parities of the z-column through the point, both ways; STRICT -- a
    column that passes exactly through an edge or a vertex in rescaled coordinates counts no crossing there, and the point may
    be answered "outside"; return_ambiguous=True -> (inside, ambiguous), ambiguous marking the points whose two parities
    disagree (the reference prints a warning).  Meant for watertight meshes.  index: the hip.contains_index of the mesh built
    earlier, or None.  hip.mesh_contains for a mesh on the GPU (one host synchronisation, for the index), the specification for
    one on the host; equal bit for bit."""
    from . import meshing
    if meshing.check_rule(rule, "mesh_contains") == "winding":
        verts, faces, _ = _sdf_mesh(mesh, "mesh_contains")
        _, inside, _, _ = _winding(verts, faces, points, accuracy, "mesh_contains", index)
        return (inside, torch.zeros_like(inside)) if return_ambiguous else inside
    verts, faces = _contains_mesh(mesh, "mesh_contains")
    res = meshing.check_contains_args(verts, faces, points, resolution, "mesh_contains")
    with torch.no_grad():
        if verts.is_cuda:
            from . import hip
            inside, ambiguous, _ = hip.mesh_contains(_contains_index(verts, faces, res, index, "mesh_contains"), points,
                                                     want_ambiguous=return_ambiguous)
        else:
            if index is not None:
                raise ValueError("mesh_contains: an index belongs to a mesh on the GPU")
            inside, ambiguous, _ = meshing.mesh_contains(verts, faces, points, res)
    return (inside, ambiguous) if return_ambiguous else inside


def _used_bounds(verts, faces):
    """lo, hi (3,) float64 over the vertices some face uses (ids clamped into range), on the device."""
    used = verts.double()[faces.long().clamp(0, max(int(verts.shape[0]) - 1, 0))].reshape(-1, 3)
    return used.amin(0), used.amax(0)


def _check_bounds(bounds, padding, what):
    if isinstance(padding, bool) or not isinstance(padding, (int, float, np.integer, np.floating)) or not math.isfinite(float(padding)) \
            or float(padding) < 0:
        raise ValueError("%s: padding must be a finite length >= 0, got %r" % (what, padding))
    if bounds is None:
        return None
    lo, hi = (torch.as_tensor(b, dtype=torch.float64).reshape(-1).cpu() for b in bounds)
    if lo.numel() != 3 or hi.numel() != 3 or not bool(torch.isfinite(lo).all() & torch.isfinite(hi).all() & (hi >= lo).all()):
        raise ValueError("%s: bounds must be (lo, hi), three finite numbers each with lo <= hi" % what)
    return lo, hi


def _mesh_bounds(verts, faces, bounds, what):
    """(lo, hi) float64 (3,) on the host: `bounds` as given and checked, else the bounding box of the vertices the faces use (read
    back: a host synchronisation)."""
    given = _check_bounds(bounds, 0.0, what)
    if given is not None:
        return given
    if int(faces.shape[0]) < 1 or int(verts.shape[0]) < 1:
        raise ValueError("%s: a mesh without faces has no bounds; give bounds" % what)
    lo, hi = (b.cpu() for b in _used_bounds(verts, faces))
    if not bool(torch.isfinite(lo).all() & torch.isfinite(hi).all()):
        raise ValueError("%s: the mesh's bounds are not finite; give bounds" % what)
    return lo, hi


def _lattice_cells(verts, faces, dims, resolution, bounds, padding, what):
    """The lattice arguments of `voxelize`, shared with `mesh_sdf_grid`: -> lo, hi, ext (3,) float64 on the host and dims, three ints.
    bounds (default the mesh's), widened by padding; dims cells per axis, or resolution = N cubic cells along the longest axis."""
    _check_bounds(bounds, padding, what)
    if (dims is None) == (resolution is None):
        raise ValueError("%s: give either dims or resolution" % what)
    lo, hi = _mesh_bounds(verts, faces, bounds, what)
    lo, hi = lo - float(padding), hi + float(padding)
    ext = hi - lo
    if dims is not None:
        dims = (dims,) * 3 if isinstance(dims, (int, np.integer)) and not isinstance(dims, bool) else tuple(dims)
        if len(dims) != 3 or any(isinstance(d, bool) or int(d) != d or int(d) < 1 for d in dims):
            raise ValueError("%s: dims must be one or three positive integers, got %r" % (what, dims))
        dims = tuple(int(d) for d in dims)
    else:
        if isinstance(resolution, bool) or int(resolution) != resolution or int(resolution) < 1:
            raise ValueError("%s: resolution must be a positive integer, got %r" % (what, resolution))
        longest = float(ext.max())
        if not longest > 0:
            raise ValueError("%s: resolution needs bounds with an extent" % what)
        cell = longest / int(resolution)
        dims = tuple(max(1, min(int(resolution), int(math.ceil(float(e) / cell - 1e-9)))) for e in ext)
        hi = lo + torch.tensor(dims, dtype=torch.float64) * cell
        ext = hi - lo
    if dims[0] * dims[1] * dims[2] > 2 ** 31 - 1:
        raise ValueError("%s: at most 2^31 - 1 cells" % what)
    return lo, hi, ext, dims


def _cell_centres(lo, ext, dims, dev):
    """Centre i of an axis lies at lo + (i + 0.5) (hi - lo) / N, computed in float64 and rounded to float32."""
    return [(lo[a] + (torch.arange(dims[a], dtype=torch.float64) + 0.5) * (ext[a] / dims[a])).to(torch.float32).to(dev) for a in range(3)]


def _winding_lattice(verts, faces, axes, dims, accuracy, index, what):
    """The winding number on a lattice -> w (Nx,Ny,Nz) float64, occupancy (Nx,Ny,Nz) bool: hip.mesh_winding_grid on the GPU, the
    specification on the meshgrid on the host."""
    from . import meshing
    acc = meshing.check_accuracy(accuracy, what)
    with torch.no_grad():
        if verts.is_cuda:
            from . import hip
            if index is None:
                index = hip.winding_index(verts, faces)
            elif not _is_winding_index_of(index, verts, faces, None):
                raise ValueError("%s: index must be the hip.winding_index of this mesh" % what)
            w, occ, _, _ = hip.mesh_winding_grid(index, *axes, acc)
            return w, occ
        if index is not None:
            raise ValueError("%s: an index belongs to a mesh on the GPU" % what)
        grid = torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1).reshape(-1, 3)
        w, inside, _, _ = _winding(verts, faces, grid, acc, what)
        return w.reshape(dims), inside.reshape(dims)


def voxelize(mesh, dims=None, resolution=None, bounds=None, padding=0.0, hash_resolution=512, index=None, rule="parity", accuracy=3.0):
    """rule="winding": occupancy = orient * winding number >= 0.5 as in `mesh_contains` (for meshes that are not watertight; face ids
    checked; "ambiguous" is 0; the dict gains "winding" (Nx,Ny,Nz) float64; index: a hip.winding_index or None).  Default "parity":

    The mesh (as in `mesh_contains`) on a regular lattice: -> dict with "occupancy" (Nx,Ny,Nz) bool -- whether the CENTRE of the
    cell lies inside --, "xs", "ys", "zs" the centres' float32 coordinates, "ambiguous" the number of ambiguous centres (0-dim int64
    tensor) and "bounds" (lo, hi) as tuples of floats.  The lattice spans `bounds` = (lo, hi), default the bounding box of the
    vertices the faces use (read back: a host synchronisation), widened by the length `padding` on every side; dims = (Nx, Ny, Nz)
    or one int for all three cuts each axis into that many cells, resolution = N instead makes cubic cells, N along the longest
    axis and ceil(extent / cell) >= 1 along the others.  Centre i of an axis lies at lo + (i + 0.5) (hi - lo) / N, computed in
    float64 and rounded to float32.  hip.mesh_contains_grid on the GPU (the 2-D test once per lattice column), the specification
    on the meshgrid on the host; equal bit for bit."""
    from . import meshing
    winding = meshing.check_rule(rule, "voxelize") == "winding"
    if winding:                                              # no hash: hash_resolution is not read
        verts, faces = _sdf_mesh(mesh, "voxelize")[:2]
    else:
        verts, faces = _contains_mesh(mesh, "voxelize")
        res = meshing.check_contains_args(verts, faces, None, hash_resolution, "voxelize")
    lo, hi, ext, dims = _lattice_cells(verts, faces, dims, resolution, bounds, padding, "voxelize")
    dev = verts.device
    axes = _cell_centres(lo, ext, dims, dev)
    if winding:
        w, occ = _winding_lattice(verts, faces, axes, dims, accuracy, index, "voxelize")
        return {"occupancy": occ, "xs": axes[0], "ys": axes[1], "zs": axes[2], "ambiguous": torch.zeros((), dtype=torch.int64, device=dev),
                "bounds": (tuple(lo.tolist()), tuple(hi.tolist())), "winding": w}
    with torch.no_grad():
        if verts.is_cuda:
            from . import hip
            occ, amb = hip.mesh_contains_grid(_contains_index(verts, faces, res, index, "voxelize"), *axes)
        else:
            if index is not None:
                raise ValueError("voxelize: an index belongs to a mesh on the GPU")
            grid = torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1).reshape(-1, 3)
            inside, ambiguous, _ = meshing.mesh_contains(verts, faces, grid, res)
            occ, amb = inside.reshape(dims), ambiguous.sum()
    return {"occupancy": occ, "xs": axes[0], "ys": axes[1], "zs": axes[2], "ambiguous": amb,
            "bounds": (tuple(lo.tolist()), tuple(hi.tolist()))}


def mesh_iou(mesh_a, mesh_b, n_points=100000, seed=0, bounds=None, padding=0.0, resolution=512, return_points=False, rule="parity",
             accuracy=3.0):
    """rule="winding": both meshes answer `mesh_contains(rule="winding", accuracy=accuracy)` -- the IoU of meshes that are not
    watertight; ambiguous_a and ambiguous_b are 0, and the dict gains "winding" = (w_a, w_b), two (n,) float64.  Default "parity":

    Volumetric intersection over union of two (watertight) meshes, as in `mesh_contains`, on one device -- the third number of
    the occupancy-network evaluation protocol.  n_points float32 points are drawn uniformly in `bounds` = (lo, hi), default the
    union of the two meshes' bounding boxes (of the vertices their faces use), widened by the length `padding` on every side,
    from a torch.Generator on the meshes' device seeded with `seed` (as `mesh_metrics` seeds its samples): lo + u (hi - lo) in
    float64 with u = rand(n, 3) float64, rounded to float32.  Both meshes answer `mesh_contains` at `resolution` for the same points.
    -> dict of 0-dim tensors on the device: iou = n_both / n_either in float64 from the integer counts (NaN when n_either = 0),
    n_a, n_b, n_both, n_either (int64), ambiguous_a, ambiguous_b (int64: points whose parities disagree; they count as outside),
    volume_a, volume_b (float64: the share of the points inside times the box's volume), plus n_points (Python int).
    return_points=True adds "points" (n,3) float32, "inside_a", "inside_b" (n,) bool, for tests.  On the GPU the two indices cost one
    host synchronisation each; nothing else is read back.  The same inputs and seed give the same bits."""
    from . import meshing
    winding = meshing.check_rule(rule, "mesh_iou") == "winding"
    if isinstance(n_points, bool) or int(n_points) != n_points or not 1 <= int(n_points) <= 2 ** 31 - 1:
        raise ValueError("mesh_iou: n_points must be a positive integer, got %r" % (n_points,))
    n = int(n_points)
    if winding:
        meshing.check_accuracy(accuracy, "mesh_iou")
        (va, fa), (vb, fb) = _sdf_mesh(mesh_a, "mesh_iou")[:2], _sdf_mesh(mesh_b, "mesh_iou")[:2]
    else:
        (va, fa), (vb, fb) = _contains_mesh(mesh_a, "mesh_iou"), _contains_mesh(mesh_b, "mesh_iou")
    if va.device != vb.device:
        raise ValueError("mesh_iou: the two meshes must live on one device")
    res = meshing.check_contains_args(va, fa, None, resolution, "mesh_iou")
    meshing.check_contains_args(vb, fb, None, resolution, "mesh_iou")
    given = _check_bounds(bounds, padding, "mesh_iou")
    dev = va.device
    with torch.no_grad():
        if given is None:
            if min(int(fa.shape[0]), int(fb.shape[0]), int(va.shape[0]), int(vb.shape[0])) < 1:
                raise ValueError("mesh_iou: a mesh without faces has no bounds; give bounds")
            (la, ha), (lb, hb) = _used_bounds(va, fa), _used_bounds(vb, fb)
            lo, hi = torch.minimum(la, lb), torch.maximum(ha, hb)
        else:
            lo, hi = given[0].to(dev), given[1].to(dev)
        lo, hi = lo - float(padding), hi + float(padding)
        gen = torch.Generator(device=dev).manual_seed(int(seed))
        u = torch.rand(n, 3, dtype=torch.float64, device=dev, generator=gen)
        pts = (lo + u * (hi - lo)).to(torch.float32).contiguous()
        if winding:
            w_a, in_a, _, _ = _winding(va, fa, pts, accuracy, "mesh_iou")
            w_b, in_b, _, _ = _winding(vb, fb, pts, accuracy, "mesh_iou")
            amb_a, amb_b = torch.zeros_like(in_a), torch.zeros_like(in_b)
        else:
            in_a, amb_a = mesh_contains((va, fa), pts, res, return_ambiguous=True)
            in_b, amb_b = mesh_contains((vb, fb), pts, res, return_ambiguous=True)
        n_a, n_b = in_a.sum(), in_b.sum()
        n_both, n_either = (in_a & in_b).sum(), (in_a | in_b).sum()
        volume = (hi - lo).prod()
        out = {"iou": n_both.double() / n_either.double(), "n_a": n_a, "n_b": n_b, "n_both": n_both, "n_either": n_either,
               "ambiguous_a": amb_a.sum(), "ambiguous_b": amb_b.sum(), "volume_a": n_a.double() / n * volume,
               "volume_b": n_b.double() / n * volume, "n_points": n}
        if winding:
            out["winding"] = (w_a, w_b)
    if return_points:
        out.update(points=pts, inside_a=in_a, inside_b=in_b)
    return out


# ---- signed distance to a mesh, remeshing (DESIGN.md "Signed distance to a mesh on the device") ----------------------------
SDF_KEYS = ("sdf", "d2", "face", "closest", "inside", "ambiguous", "gradient")


def _sdf_mesh(mesh, what):
    """`_contains_mesh`, float32 vertices, and every face id checked (a host synchronisation): a distance needs real triangles.
    -> verts, faces, tris (F,3,3) float32."""
    verts, faces = _contains_mesh(mesh, what)
    V = int(verts.shape[0])
    if faces.numel() and not bool(((faces >= 0) & (faces < V)).all()):
        raise ValueError("%s: a face names a vertex outside [0, %d)" % (what, V))
    tris = verts[faces.long()].contiguous() if faces.numel() else verts.new_zeros((0, 3, 3))
    return verts, faces, tris


def mesh_sdf(mesh, points, trunc=float("inf"), resolution=512, index=None, contains_index=None, rule="parity", accuracy=3.0):
    """rule="winding": the sign comes from `mesh_contains(rule="winding", accuracy=accuracy)` -- a signed distance to a mesh that is
    not watertight; "ambiguous" is all False and the dict gains "winding" (P,) float64; contains_index: a hip.winding_index or None.
    Default "parity":

    The signed distance of points (P,3) float32 to a mesh -- an (F,3,3) soup or a (verts, faces) pair as in `mesh_contains`, on the
    points' device -> dict: "sdf" (P,) float32 = meshing.signed_distance(d2, inside, trunc), negative inside; "d2" (P,) float64, "face"
    (P,) int32 and "closest" (P,3) float64 of the closest triangle (+inf, -1, NaN for a point farther than `trunc`, outside the band);
    "inside", "ambiguous" (P,) bool, `mesh_contains` at `resolution`, for every point; "gradient" (P,3) float64, the unit vector
    sign (p - closest) / |p - closest|, NaN where d2 == 0 and outside the band.  The rule is meshing.mesh_sdf.  On the GPU it is
    hip.mesh_closest plus hip.mesh_contains (index: the hip.mesh_index of the mesh's soup, contains_index: its hip.contains_index,
    built earlier, or None), on the host the specification.  The sign is the parity rule's: meant for watertight meshes."""
    from . import meshing
    winding = meshing.check_rule(rule, "mesh_sdf") == "winding"
    if winding:
        meshing.check_accuracy(accuracy, "mesh_sdf")
    t = meshing.check_trunc(trunc, "mesh_sdf")
    verts, faces, tris = _sdf_mesh(mesh, "mesh_sdf")
    res = meshing.check_contains_args(verts, faces, points, resolution, "mesh_sdf")
    if points.dtype != torch.float32:
        raise ValueError("mesh_sdf: points must be (P, 3) float32")
    with torch.no_grad():
        if verts.is_cuda:
            from . import hip
            pts = points.detach().contiguous()
            if int(tris.shape[0]) < 1:
                d2, face, closest = meshing.soup_closest(tris, pts, t)
            else:
                d2, face, closest, _ = hip.mesh_closest(_ray_index(tris, index, "mesh_sdf"), pts)
                inf = torch.full_like(d2, float("inf"))
                out = (d2 > t * t) | ((face < 0) & ~torch.isnan(d2))        # beyond the band; or no triangle gave a number
                d2, face = torch.where(out, inf, d2), torch.where(out, torch.full_like(face, -1), face)
                closest = torch.where(out[:, None], torch.full_like(closest, float("nan")), closest)
            if not winding:
                inside, ambiguous, _ = hip.mesh_contains(_contains_index(verts, faces, res, contains_index, "mesh_sdf"), pts,
                                                         want_ambiguous=True)
        else:
            if index is not None or contains_index is not None:
                raise ValueError("mesh_sdf: an index belongs to a mesh on the GPU")
            if winding:                                      # the closest triangle alone: the parity pass would be thrown away
                d2, face, closest = meshing.soup_closest(tris, points, t)
            else:
                d2, face, closest, inside, ambiguous = meshing.mesh_sdf(verts, faces, points, t, res)
        if winding:
            w, inside, _, _ = _winding(verts, faces, points, accuracy, "mesh_sdf", contains_index)
            ambiguous = torch.zeros_like(inside)
        dv = points.detach().double() - closest
        norm = torch.sqrt((dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1]) + dv[:, 2] * dv[:, 2])
        gradient = torch.where(inside[:, None], -dv, dv) / norm[:, None]        # 0 / 0 on the surface, NaN outside the band
    out = {"sdf": meshing.signed_distance(d2, inside, t), "d2": d2, "face": face, "closest": closest, "inside": inside,
           "ambiguous": ambiguous, "gradient": gradient}
    if winding:
        out["winding"] = w
    return out


def mesh_sdf_grid(mesh, dims=None, resolution=None, n_side=None, bounds=None, padding=0.0, trunc=None, nodes="centres",
                  hash_resolution=512, index=None, want_face=False, rule="parity", accuracy=3.0):
    """rule="winding": "inside" is hip.mesh_winding_grid's occupancy (`voxelize(rule="winding")`), handed to hip.mesh_sdf_grid -- the
    signed field of a mesh that is not watertight; "ambiguous" is 0 and the dict gains "winding" (Nx,Ny,Nz) float64; index: a
    hip.winding_index or None.  Default "parity":

    The truncated signed distance field of a mesh (as in `mesh_sdf`) on a regular lattice -> dict: "sdf" (Nx,Ny,Nz) float32,
    meshing.signed_distance; "d2" (Nx,Ny,Nz) float64, +inf outside the band; "face" (Nx,Ny,Nz) int32 with want_face=True, else None;
    "inside" (Nx,Ny,Nz) bool and "ambiguous" (0-dim int64), `voxelize`'s; "xs", "ys", "zs" the nodes' float32 coordinates; "bounds"
    (lo, hi); "band", the number of nodes within trunc (0-dim int64 on the device); "trunc" and "step" (floats); "box" and "info".
    nodes="centres": dims / resolution / bounds / padding mean exactly what they mean in `voxelize`, whose lattice this is.
    nodes="corners" with n_side=N: the cube lattice of hip.lattice_box(lo, hi, padding) with N nodes per axis, node i at origin +
    i side / (N - 1) in float64 rounded to float32 -- the lattice hip.marching_cubes_indexed and hip.lattice_to_world assume; "box" is
    its (origin xyz, side), else None.  trunc: the width of the band, default three lattice steps (the largest of the three).  On the
    GPU hip.mesh_contains_grid and hip.mesh_sdf_grid (csrc/meshsdf.hpp: the cost follows the band, "info" are its counters), on the
    host the specification on the meshgrid; d2, face and inside are equal bit for bit."""
    from . import meshing
    what = "mesh_sdf_grid"
    winding = meshing.check_rule(rule, what) == "winding"
    if winding:
        meshing.check_accuracy(accuracy, what)
    verts, faces, tris = _sdf_mesh(mesh, what)
    res = meshing.check_contains_args(verts, faces, None, hash_resolution, what)
    dev = verts.device
    if nodes not in ("centres", "corners"):
        raise ValueError("%s: nodes must be 'centres' or 'corners', got %r" % (what, nodes))
    box = None
    if nodes == "corners":
        if dims is not None or resolution is not None or n_side is None:
            raise ValueError("%s: nodes='corners' takes n_side, the cube lattice's nodes per axis" % what)
        if isinstance(n_side, bool) or int(n_side) != n_side or not 2 <= int(n_side) <= 1290:
            raise ValueError("%s: n_side must be an integer in [2, 1290], got %r" % (what, n_side))
        _check_bounds(None, padding, what)
        n = int(n_side)
        lo, hi = _mesh_bounds(verts, faces, bounds, what)
        lo, hi = lo - float(padding), hi + float(padding)
        side = float((hi - lo).max())
        if not side > 0:
            raise ValueError("%s: the cube lattice needs bounds with an extent" % what)
        origin = 0.5 * (lo + hi) - 0.5 * side
        lo, hi = origin, origin + side
        step = side / (n - 1)
        axes = [(origin[a] + torch.arange(n, dtype=torch.float64) * step).to(torch.float32).to(dev) for a in range(3)]
        box = torch.cat([origin, torch.tensor([side], dtype=torch.float64)]).to(torch.float32).to(dev)
        dims = (n, n, n)
    else:
        if n_side is not None:
            raise ValueError("%s: n_side belongs to nodes='corners'; give dims or resolution" % what)
        lo, hi, ext, dims = _lattice_cells(verts, faces, dims, resolution, bounds, padding, what)
        axes = _cell_centres(lo, ext, dims, dev)
        step = float((ext / torch.tensor(dims, dtype=torch.float64)).max())
    t = meshing.check_trunc(3.0 * step if trunc is None else trunc, what)
    meshing.check_lattice_axes(*axes, what=what)     # a lattice finer than float32 resolves is refused here
    info = None
    with torch.no_grad():
        if winding:
            w, occ = _winding_lattice(verts, faces, axes, dims, accuracy, index, what)
            amb = torch.zeros((), dtype=torch.int64, device=dev)
        if verts.is_cuda:
            from . import hip
            if not winding:
                occ, amb = hip.mesh_contains_grid(_contains_index(verts, faces, res, index, what), *axes)
            d2, face, sdf, info = hip.mesh_sdf_grid(tris, *axes, t, occupancy=occ, want_face=want_face, want_info=True)
            band = info[0].long()
        else:
            if index is not None:
                raise ValueError("%s: an index belongs to a mesh on the GPU" % what)
            if not winding:
                grid = torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1).reshape(-1, 3)
                inside, ambiguous, _ = meshing.mesh_contains(verts, faces, grid, res)
                occ, amb = inside.reshape(dims), ambiguous.sum()
            d2, face = meshing.mesh_sdf_grid(tris, *axes, t)
            sdf = meshing.signed_distance(d2, occ, t)
            band = ((d2 <= t * t) & (d2 < float("inf"))).sum()
            face = face if want_face else None
    out = {"sdf": sdf, "d2": d2, "face": face, "inside": occ, "xs": axes[0], "ys": axes[1], "zs": axes[2], "ambiguous": amb,
           "bounds": (tuple(lo.tolist()), tuple(hi.tolist())), "band": band, "trunc": t, "step": step, "box": box, "info": info}
    if winding:
        out["winding"] = w
    return out


def remesh(mesh, n_side=256, offset=0.0, trunc=None, padding=None, clean=None, smooth=None, rule="parity", accuracy=3.0):
    """rule="winding": the field's sign comes from the winding number (`mesh_sdf_grid(rule="winding", accuracy=accuracy)`), so the
    input need NOT be watertight: remesh(open_mesh, rule="winding") is the REPAIR of a mesh with holes, open sheets or flipped
    patches into a watertight one -- holes are closed where the winding number crosses 1/2.  Default "parity":

    A watertight, uniform remesh of a (watertight) mesh, or an offset surface of it: the level `offset` (metres; positive grows
    the body) of its signed distance field on the cube lattice of `mesh_sdf_grid(nodes="corners", n_side=n_side)`, by
    hip.marching_cubes_indexed and hip.lattice_to_world -> (verts (V,3) float32 in the mesh's own coordinates, faces (F,3) int32).
    trunc defaults to |offset| plus three lattice steps; |offset| must stay below trunc by at least one step, so that both ends of
    every edge that crosses the level hold true distances.  padding defaults to max(offset, 0) plus two steps (the step then
    follows from extent + 2 padding = (n_side - 1) step).  clean / smooth: the policies of geometry.clean_mesh / smooth_mesh
    (check_keep, check_smooth), applied in that order.  The two capacities are read back once.  GPU only."""
    from . import meshing
    what = "remesh"
    meshing.check_rule(rule, what)
    meshing.check_accuracy(accuracy, what)
    if isinstance(offset, bool) or not isinstance(offset, (int, float, np.integer, np.floating)) or not math.isfinite(float(offset)):
        raise ValueError("remesh: offset must be a finite length, got %r" % (offset,))
    offset = float(offset)
    if isinstance(n_side, bool) or int(n_side) != n_side or not 8 <= int(n_side) <= 894:
        raise ValueError("remesh: n_side must be an integer in [8, 894], got %r" % (n_side,))
    n = int(n_side)
    if clean is not None:
        check_keep(clean)
    if smooth is not None:
        smooth = check_smooth(smooth)
    verts, faces, _ = _sdf_mesh(mesh, what)
    lo, hi = _mesh_bounds(verts, faces, None, what)
    extent = float((hi - lo).max())
    if padding is None:
        step = (extent + 2.0 * max(offset, 0.0)) / (n - 5)      # extent + 2 (max(offset, 0) + 2 step) = (n - 1) step
        padding = max(offset, 0.0) + 2.0 * step
    else:
        _check_bounds(None, padding, what)
        step = (extent + 2.0 * float(padding)) / (n - 1)
    if not step > 0:
        raise ValueError("remesh: the mesh has no extent")
    t = meshing.check_trunc(abs(offset) + 3.0 * step if trunc is None else trunc, what)
    if not abs(offset) <= t - step:
        raise ValueError("remesh: |offset| = %g must stay below trunc = %g by at least one lattice step (%g)" % (abs(offset), t, step))
    if not verts.is_cuda:
        raise ValueError("remesh runs on the HIP kernels: the mesh must live on the GPU")
    from . import hip
    with torch.no_grad():
        field = mesh_sdf_grid((verts, faces), n_side=n, padding=padding, trunc=t, nodes="corners", rule=rule, accuracy=accuracy)
        vert_cap, face_cap = meshing.MC_DEFAULT_VERT_CAP, meshing.MC_DEFAULT_CAP
        out_v, out_f, size = hip.marching_cubes_indexed(field["sdf"], offset, vert_cap, face_cap)
        V, F = size.tolist()
        if V > vert_cap or F > face_cap:   # too small for this level set: the exact sizes, once more
            out_v, out_f, size = hip.marching_cubes_indexed(field["sdf"], offset, max(V, 1), max(F, 1))
        out_v, out_f = hip.lattice_to_world(out_v[:V], field["box"]), out_f[:F]
        if clean is not None:
            kept = clean_mesh(out_v, out_f, keep=clean)
            out_v, out_f = kept["verts"], kept["faces"]
        if smooth is not None:
            out_v = smooth_mesh(out_v, out_f, **smooth)
    return out_v, out_f


# ---- ground-truth files -------------------------------------------------------------------------------------------------
_PLY_TYPES ={"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}


def _load_ply(path):
    verts, faces, _ = _read_ply(path)
    if verts is None or faces is None:
        raise ValueError("%s: a mesh needs a vertex and a face element" % path)
    return verts, faces


def _read_ply(path):
    """-> (vertices (V,3) float64 or None, faces (F,3) int64 or None: no face element, normals (V,3) float64 or None: the vertex
    element has no nx, ny, nz)."""
    with open(path, "rb") as f:
        raw = f.read()
    end = raw.find(b"end_header")
    if not raw.startswith(b"ply") or end < 0:
        raise ValueError("%s is not a PLY file" % path)
    nl = raw.find(b"\n", end)
    if nl < 0:
        raise ValueError("%s: the PLY header does not end" % path)
    header, body = raw[:end].decode("ascii", "replace").split("\n"), raw[nl + 1:]
    fmt, elements = None, []
    for line in header:
        w = line.split()
        if not w or w[0] in ("ply", "comment", "obj_info"):
            continue
        if w[0] == "format":
            fmt = w[1]
        elif w[0] == "element":
            elements.append({"name": w[1], "count": int(w[2]), "props": []})
        elif w[0] == "property":
            if not elements:
                raise ValueError("%s: a property outside an element" % path)
            if w[1] == "list":
                elements[-1]["props"].append(("list", w[2], w[3], w[4]))
            else:
                elements[-1]["props"].append(("scalar", w[1], w[2]))
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError("%s: PLY format %r is not supported (ascii and binary_little_endian are)" % (path, fmt))
    for e in elements:
        for p in e["props"]:
            for t in p[1:-1]:
                if t not in _PLY_TYPES:
                    raise ValueError("%s: unknown PLY type %r" % (path, t))
    verts = faces = normals = None
    tokens, pos = (body.split(), 0) if fmt == "ascii" else (None, 0)
    for e in elements:
        scalar_only = all(p[0] == "scalar" for p in e["props"])
        if e["name"] == "vertex":
            names = [p[2] for p in e["props"]]
            if not scalar_only or not all(k in names for k in "xyz"):
                raise ValueError("%s: the vertex element needs scalar properties x, y, z" % path)
            cols = [names.index(k) for k in "xyz"]
            ncols = [names.index(k) for k in ("nx", "ny", "nz")] if all(k in names for k in ("nx", "ny", "nz")) else None
            if fmt == "ascii":
                k = len(names)
                block = np.array(tokens[pos:pos + k * e["count"]], dtype=np.float64)
                if block.size != k * e["count"]:
                    raise ValueError("%s: the file ends inside the vertex element" % path)
                pos += k * e["count"]
                verts = block.reshape(e["count"], k)[:, cols]
                normals = block.reshape(e["count"], k)[:, ncols] if ncols else None
            else:
                dt = np.dtype([(p[2], "<" + _PLY_TYPES[p[1]]) for p in e["props"]])
                if pos + dt.itemsize * e["count"] > len(body):
                    raise ValueError("%s: the file ends inside the vertex element" % path)
                block = np.frombuffer(body, dt, e["count"], pos)
                pos += dt.itemsize * e["count"]
                verts = np.stack([block[k].astype(np.float64) for k in "xyz"], 1)
                normals = np.stack([block[k].astype(np.float64) for k in ("nx", "ny", "nz")], 1).reshape(-1, 3) if ncols else None
        elif e["name"] == "face":
            lists = [p for p in e["props"] if p[0] == "list"]
            if len(lists) != 1 or lists[0][3] not in ("vertex_indices", "vertex_index"):
                raise ValueError("%s: the face element needs one list property vertex_indices" % path)
            li = e["props"].index(lists[0])
            if fmt == "ascii" and len(e["props"]) == 1:
                # rows of "3 i j k" as one block; the first row that is not a triangle is found while the rows still align
                block = np.array(tokens[pos:pos + 4 * e["count"]], dtype=np.float64)
                rows = block[:block.size // 4 * 4].reshape(-1, 4)
                if (rows[:, 0] != 3).any():
                    r = int(np.nonzero(rows[:, 0] != 3)[0][0])
                    raise ValueError("%s: face %d has %d corners; triangle faces only" % (path, r, int(rows[r, 0])))
                if block.size != 4 * e["count"]:
                    raise ValueError("%s: the file ends inside the face element" % path)
                pos += 4 * e["count"]
                faces = rows[:, 1:].astype(np.int64)
            elif fmt == "ascii":
                out = np.empty((e["count"], 3), np.int64)
                for r in range(e["count"]):
                    for q, p in enumerate(e["props"]):
                        if pos >= len(tokens):
                            raise ValueError("%s: the file ends inside the face element" % path)
                        if p[0] == "scalar":
                            pos += 1
                            continue
                        cnt = int(tokens[pos])
                        if q == li:
                            if cnt != 3:
                                raise ValueError("%s: face %d has %d corners; triangle faces only" % (path, r, cnt))
                            out[r] = [int(t) for t in tokens[pos + 1:pos + 4]]
                        pos += 1 + cnt
                faces = out
            else:
                # every face must be a triangle: then the rows have one size and the element is one structured array
                fields = []
                for q, p in enumerate(e["props"]):
                    if p[0] == "scalar":
                        fields.append(("s%d" % q, "<" + _PLY_TYPES[p[1]]))
                    elif q == li:
                        fields += [("cnt", "<" + _PLY_TYPES[p[1]]), ("idx", "<" + _PLY_TYPES[p[2]], (3,))]
                    else:
                        raise ValueError("%s: the face element needs one list property vertex_indices" % path)
                dt = np.dtype(fields)
                have = min(e["count"], (len(body) - pos) // dt.itemsize)
                block = np.frombuffer(body, dt, have, pos)
                if (block["cnt"] != 3).any():
                    r = int(np.nonzero(block["cnt"] != 3)[0][0])
                    raise ValueError("%s: face %d has %d corners; triangle faces only" % (path, r, int(block["cnt"][r])))
                if have != e["count"]:
                    raise ValueError("%s: the file ends inside the face element" % path)
                pos += dt.itemsize * e["count"]
                faces = block["idx"].astype(np.int64)
        else:
            if not scalar_only:
                raise ValueError("%s: element %r with a list property is not supported" % (path, e["name"]))
            if fmt == "ascii":
                pos += len(e["props"]) * e["count"]
            else:
                pos += sum(np.dtype(_PLY_TYPES[p[1]]).itemsize for p in e["props"]) * e["count"]
    return verts, faces, normals


def load_mesh(path, device=None):
    """A ground-truth mesh from `path`: .npz with keys `vertices` (V,3) and `faces` (F,3), or PLY (ASCII or binary
    little-endian, triangle faces only) -> (verts (V,3) float32, faces (F,3) int64) tensors on `device` (default: the host).
    ValueError for anything else: other formats, missing keys, faces that are not triangles, indices out of range."""
    path = str(path)
    low = path.lower()
    if low.endswith(".npz"):
        with np.load(path) as z:
            for key in ("vertices", "faces"):
                if key not in z.files:
                    raise ValueError("%s has no key %r (keys: %s)" % (path, key, ", ".join(z.files)))
            verts, faces = z["vertices"], z["faces"]
    elif low.endswith(".ply"):
        verts, faces = _load_ply(path)
    else:
        raise ValueError("%s: only .npz and .ply meshes are read" % path)
    verts, faces = np.asarray(verts), np.asarray(faces)
    if verts.ndim != 2 or verts.shape[1] != 3:
        raise ValueError("%s: vertices must be (V, 3), got %s" % (path, verts.shape))
    if faces.ndim != 2 or faces.shape[1] != 3:
        raise ValueError("%s: faces must be (F, 3) triangles, got %s" % (path, faces.shape))
    if not np.issubdtype(faces.dtype, np.integer):
        raise ValueError("%s: faces must hold integer vertex indices" % path)
    if faces.size and (faces.min() < 0 or faces.max() >= verts.shape[0]):
        raise ValueError("%s: a face refers to a vertex that does not exist" % path)
    v = torch.from_numpy(np.ascontiguousarray(verts, np.float32))
    f = torch.from_numpy(np.ascontiguousarray(faces, np.int64))
    return (v.to(device), f.to(device)) if device is not None else (v, f)


def _read_geometry(path):
    """-> (vertices, faces or None, normals or None) as numpy arrays, whatever the file holds; ValueError for another format."""
    low = path.lower()
    if low.endswith(".npz"):
        with np.load(path) as z:
            if "faces" in z.files:
                if "vertices" not in z.files:
                    raise ValueError("%s has no key 'vertices' (keys: %s)" % (path, ", ".join(z.files)))
                return z["vertices"], z["faces"], z["normals"] if "normals" in z.files else None
            for key in ("points", "vertices"):
                if key in z.files:
                    return z[key], None, z["normals"] if "normals" in z.files else None
            raise ValueError("%s has neither 'points' nor 'vertices' (keys: %s)" % (path, ", ".join(z.files)))
    if low.endswith(".ply"):
        verts, faces, normals = _read_ply(path)
        if verts is None:
            raise ValueError("%s: no vertex element" % path)
        return verts, faces, normals
    raise ValueError("%s: only .npz and .ply files are read" % path)


def _cloud_from(path, points, normals, device):
    points = np.asarray(points)
    if points.ndim != 2 or points.shape[1] != 3 or points.shape[0] < 1 or not np.issubdtype(points.dtype, np.number):
        raise ValueError("%s: points must be (P, 3) with P >= 1, got %s" % (path, points.shape))
    points = np.ascontiguousarray(points, np.float32)
    if not np.isfinite(points).all():
        raise ValueError("%s: a point has a non-finite coordinate" % path)
    if normals is not None:
        normals = np.asarray(normals)
        if normals.shape != points.shape:
            raise ValueError("%s: normals must be (P, 3) = %s, got %s" % (path, points.shape, normals.shape))
        normals = torch.from_numpy(np.ascontiguousarray(normals, np.float32))
    cloud = PointCloud(torch.from_numpy(points), normals)
    return cloud.to(device) if device is not None else cloud


def load_points(path, device=None):
    """A ground-truth scan from `path`: .npz with `points` (or `vertices` and no `faces`) and optionally `normals`, or a PLY
    (ASCII or binary little-endian) with a vertex element and no faces -- no face element or one of count zero -- and optionally
    nx, ny, nz -> PointCloud of float32 tensors on `device` (default: the host).  ValueError for anything else: other formats, a
    file with faces (`load_mesh` / `load_geometry` read those), non-finite coordinates, wrong shapes, normals of another
    length."""
    path = str(path)
    points, faces, normals = _read_geometry(path)
    if faces is not None and np.asarray(faces).shape[0] > 0:
        raise ValueError("%s holds a mesh (it has faces): load_mesh or load_geometry reads it" % path)
    return _cloud_from(path, points, normals, device)


def load_geometry(path, device=None):
    """Whatever ground truth `path` holds: a (verts, faces) pair (`load_mesh`) when the file has faces, a PointCloud
    (`load_points`) otherwise."""
    path = str(path)
    points, faces, normals = _read_geometry(path)
    if faces is not None and np.asarray(faces).shape[0] > 0:
        return load_mesh(path, device)
    return _cloud_from(path, points, normals, device)


def save_points(path, points, normals=None):
    """Write a point cloud: points (P,3) float, optional normals (P,3).  `.npz`: keys `points` and, when given, `normals`
    (float32).  `.ply`: binary little-endian, one vertex element with float x y z [, float nx ny nz] and no face element.
    `load_points` reads either back bit-equal.  ValueError for another extension, wrong shapes, or normals of another length."""
    path = str(path)
    low = path.lower()
    if not low.endswith((".npz", ".ply")):
        raise ValueError("%s: only .npz and .ply clouds are written" % path)

    def host(a):
        return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)

    if isinstance(points, PointCloud):
        points, normals = points.points, points.normals if normals is None else normals
    v = host(points)
    if v.ndim != 2 or v.shape[1] != 3 or v.shape[0] < 1:
        raise ValueError("points must be (P, 3) with P >= 1, got %s" % (v.shape,))
    v = np.ascontiguousarray(v, np.float32)
    extra = {}
    if normals is not None:
        a = host(normals)
        if a.shape != v.shape:
            raise ValueError("normals must be (P, 3) = %s, got %s" % (v.shape, a.shape))
        extra["normals"] = np.ascontiguousarray(a, np.float32)
    if low.endswith(".npz"):
        with open(path, "wb") as out:
            np.savez(out, points=v, **extra)
        return
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    header = ["ply", "format binary_little_endian 1.0", "element vertex %d" % v.shape[0],
              "property float x", "property float y", "property float z"]
    if extra:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
        header += ["property float nx", "property float ny", "property float nz"]
    header.append("end_header")
    rec = np.empty(v.shape[0], np.dtype(fields))
    for i, k in enumerate("xyz"):
        rec[k] = v[:, i]
    if extra:
        for i, k in enumerate(("nx", "ny", "nz")):
            rec[k] = extra["normals"][:, i]
    with open(path, "wb") as out:
        out.write(("\n".join(header) + "\n").encode("ascii"))
        out.write(rec.tobytes())


def save_mesh(path, verts, faces, normals=None, colors=None):
    """Write an indexed mesh: verts (V,3) float, faces (F,3) integer vertex ids, optional per-vertex normals (V,3) and colors (V,3)
    in [0,1].  `.npz`: keys `vertices` (float32), `faces` (int32) and, when given, `normals` / `colors` (float32).  `.ply`: binary
    little-endian, vertex properties float x y z [, float nx ny nz] [, uchar red green blue: round(255 c), clipped], faces as
    `list uchar int vertex_indices`.  `load_mesh` reads either back: vertices bit-equal, faces equal.  ValueError for another
    extension, wrong shapes, attribute lengths that differ from V, or a face index out of range."""
    path = str(path)
    low = path.lower()
    if not low.endswith((".npz", ".ply")):
        raise ValueError("%s: only .npz and .ply meshes are written" % path)

    def host(a):
        return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)

    v, f = host(verts), host(faces)
    if v.ndim != 2 or v.shape[1] != 3:
        raise ValueError("vertices must be (V, 3), got %s" % (v.shape,))
    if f.ndim != 2 or f.shape[1] != 3:
        raise ValueError("faces must be (F, 3) triangles, got %s" % (f.shape,))
    if not np.issubdtype(f.dtype, np.integer):
        raise ValueError("faces must hold integer vertex indices")
    if f.size and (f.min() < 0 or f.max() >= v.shape[0]):
        raise ValueError("a face refers to a vertex that does not exist")
    if v.shape[0] > np.iinfo(np.int32).max:
        raise ValueError("too many vertices for 32-bit face indices")
    v, f = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)
    extra = {}
    for name, a in (("normals", normals), ("colors", colors)):
        if a is not None:
            a = host(a)
            if a.ndim != 2 or a.shape != v.shape:
                raise ValueError("%s must be (V, 3) = %s, got %s" % (name, v.shape, a.shape))
            extra[name] = np.ascontiguousarray(a, np.float32)
    if low.endswith(".npz"):
        with open(path, "wb") as out:
            np.savez(out, vertices=v, faces=f, **extra)
        return
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    header = ["ply", "format binary_little_endian 1.0", "element vertex %d" % v.shape[0],
              "property float x", "property float y", "property float z"]
    if "normals" in extra:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
        header += ["property float nx", "property float ny", "property float nz"]
    if "colors" in extra:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        header += ["property uchar red", "property uchar green", "property uchar blue"]
    header += ["element face %d" % f.shape[0], "property list uchar int vertex_indices", "end_header"]
    vrec = np.empty(v.shape[0], np.dtype(fields))
    for i, k in enumerate("xyz"):
        vrec[k] = v[:, i]
    if "normals" in extra:
        for i, k in enumerate(("nx", "ny", "nz")):
            vrec[k] = extra["normals"][:, i]
    if "colors" in extra:
        c8 = np.clip(np.rint(extra["colors"].astype(np.float64) * 255.0), 0, 255).astype(np.uint8)
        for i, k in enumerate(("red", "green", "blue")):
            vrec[k] = c8[:, i]
    frec = np.empty(f.shape[0], np.dtype([("cnt", "u1"), ("idx", "<i4", (3,))]))
    frec["cnt"] = 3
    frec["idx"] = f
    with open(path, "wb") as out:
        out.write(("\n".join(header) + "\n").encode("ascii"))
        out.write(vrec.tobytes())
        out.write(frec.tobytes())
