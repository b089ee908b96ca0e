"""Canonical-mesh branch of the model entry (``gen_cano_mesh=True``, reference metaavatar_render/models/__init__.py:
203-311 and utils/sdf_meshing.py:13-114), on the device end to end:

  1. SDF on the 256^3 lattice of [-1,1]^3 -- one launch of the SDF kernel (``arah_sdf_grid``), the values never
     leave HBM (the reference: 64 chunks with a ``.cpu()`` copy each, sdf_meshing.py:44-57);
  2. marching cubes at level 0 as three kernels (``arah_marching_cubes``, csrc/mcubes.hpp: count per lattice row, scan,
     emit) whose triangle COUNT stays on the device -- no host round trip anywhere in the branch, so that the frames of a
     test sequence keep overlapping (``marching_cubes`` below is the same extraction as tensor operations: the
     specification the kernel is tested against, and what runs for volumes that live on the host);
  3. forward skinning of the vertices (``arah_skin_lbs``), projection, rasterisation (``arah_rasterize``) and the three
     normal maps ``output_normal`` / ``normal_cano_front`` / ``normal_cano_back`` (1,512,512,3).

Third-party pieces of the reference that are not in its tree and absent from this image, restated from their
documented behaviour (parity unpinned at triangle level):
  * ``skimage.measure.marching_cubes_lewiner`` (scikit-image 0.18): same level set, same linear interpolation of the
    crossing points along lattice edges, triangles oriented like skimage's default ``gradient_direction='descent'``
    (right-hand normals point towards DECREASING values).  The triangulation inside a cell comes from a case table
    generated here (face-consistent loops, fan triangulation) instead of Lewiner's 33-case tables: the surface is the
    same to within the cell, individual facets differ.
  * ``pytorch3d`` 0.6.1 ``cameras_from_opencv_projection``, ``look_at_view_transform``, ``FoVPerspectiveCameras``
    (fov 60 deg) and ``MeshRasterizer`` (``pix_to_face``, one face per pixel, no blur, no culling): pixel (i, j) takes
    the nearest face covering its centre.
"""
import math
import os

import numpy as np
import torch

# cube corners (dx, dy, dz), the 12 edges between them and the 6 faces as cyclic corner quadruples
CORNERS = ((0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1))
EDGES = ((0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7))
FACES = ((0, 1, 2, 3), (4, 5, 6, 7), (0, 1, 5, 4), (1, 2, 6, 5), (2, 3, 7, 6), (3, 0, 4, 7))
_EDGE_ID = {frozenset(e): i for i, e in enumerate(EDGES)}
_TABLE = None


def case_table():
    """tri_edges (256, 3*T) int8 (edge ids, -1 padded) and n_tri (256,) for every inside/outside pattern of the 8
    corners (bit c set = corner c inside).  Per face the crossed edges are joined into segments -- with four crossings
    the segments cut off the INSIDE corners, a rule that depends on the face's corner signs only, so neighbouring cells
    agree on their shared face and the mesh has no cracks --, segments chain into closed loops, loops are fanned."""
    global _TABLE
    if _TABLE is not None:
        return _TABLE
    tris = []
    for case in range(256):
        inside = [(case >> c) & 1 for c in range(8)]
        nbr = {}
        for face in FACES:
            crossed = []
            for i in range(4):
                a, b = face[i], face[(i + 1) % 4]
                if inside[a] != inside[b]:
                    crossed.append(_EDGE_ID[frozenset((a, b))])
            if len(crossed) == 2:
                segs = [tuple(crossed)]
            elif len(crossed) == 4:
                segs = []
                for i in range(4):
                    if inside[face[i]]:
                        segs.append((_EDGE_ID[frozenset((face[i - 1], face[i]))],
                                     _EDGE_ID[frozenset((face[i], face[(i + 1) % 4]))]))
            else:
                segs = []
            for a, b in segs:
                nbr.setdefault(a, []).append(b)
                nbr.setdefault(b, []).append(a)
        assert all(len(v) == 2 for v in nbr.values()), case
        out, seen = [], set()
        for start in sorted(nbr):
            if start in seen:
                continue
            loop, prev, cur = [start], None, start
            while True:
                a, b = nbr[cur]
                nxt = a if a != prev else b
                if nxt == start:
                    break
                loop.append(nxt)
                prev, cur = cur, nxt
            seen.update(loop)
            assert len(loop) >= 3, case
            for i in range(1, len(loop) - 1):
                out += [loop[0], loop[i], loop[i + 1]]
        tris.append(out)
    width = max(len(t) for t in tris)
    table = -np.ones((256, width), np.int8)
    for c, t in enumerate(tris):
        table[c, :len(t)] = t
    _TABLE = (table, np.array([len(t) // 3 for t in tris], np.int64))
    return _TABLE


def _mc_triangles(sdf, level):
    """The triangles of the level set before the orientation flip: -> (corners (F,3,3) coordinates, flip (F,) bool, pa (F,3,3)
    lattice index of the lower end of every corner's edge, axis (F,3) of that edge), or None for an empty level set."""
    dev = sdf.device
    N = sdf.shape[0]
    vs = 2.0 / (N - 1)
    table_np, ntri_np = case_table()
    table = torch.from_numpy(table_np.astype(np.int64)).to(dev)
    ntri = torch.from_numpy(ntri_np).to(dev)
    corners = torch.tensor(CORNERS, device=dev)
    edges = torch.tensor(EDGES, device=dev)
    inside = sdf < level
    case = torch.zeros(N - 1, N - 1, N - 1, dtype=torch.int64, device=dev)
    for c, (dx, dy, dz) in enumerate(CORNERS):
        case += inside[dx:N - 1 + dx, dy:N - 1 + dy, dz:N - 1 + dz].to(torch.int64) << c
    cells = torch.nonzero((case != 0) & (case != 255))                      # (M,3)
    if cells.shape[0] == 0:
        return None
    ccase = case[cells[:, 0], cells[:, 1], cells[:, 2]]
    cnt = ntri[ccase]
    owner = torch.repeat_interleave(torch.arange(cells.shape[0], device=dev), cnt)           # cell of every triangle
    first = torch.cumsum(cnt, 0) - cnt
    slot = torch.arange(owner.shape[0], device=dev) - first[owner]                            # its index in the cell
    e = table[ccase[owner].unsqueeze(1), (slot * 3).unsqueeze(1) + torch.arange(3, device=dev)]   # (F,3) edge ids
    base = cells[owner]                                                                        # (F,3)
    pa = base.unsqueeze(1) + corners[edges[e][..., 0]]                                        # (F,3,3) lattice indices
    pb = base.unsqueeze(1) + corners[edges[e][..., 1]]
    # every lattice edge is interpolated from its lower to its higher end, whichever cell asks: shared vertices come out
    # bit-identical on both sides
    swap = (pa > pb).any(-1, keepdim=True)
    pa, pb = torch.where(swap, pb, pa), torch.where(swap, pa, pb)
    va = sdf[pa[..., 0], pa[..., 1], pa[..., 2]] - level
    vb = sdf[pb[..., 0], pb[..., 1], pb[..., 2]] - level
    t = (va / (va - vb)).clamp(0.0, 1.0).unsqueeze(-1)
    verts = (pa.float() + t * (pb - pa).float()) * vs - 1.0
    # orientation: the cell's corner values give the gradient direction; normals must point DOWN the gradient
    cv = torch.stack([sdf[base[:, 0] + dx, base[:, 1] + dy, base[:, 2] + dz] for dx, dy, dz in CORNERS], dim=1)   # (F,8)
    cf = corners.float()
    grad = torch.stack([(cv * (2 * cf[:, k] - 1)).sum(1) for k in range(3)], dim=1)
    nrm = torch.cross(verts[:, 1] - verts[:, 0], verts[:, 2] - verts[:, 0], dim=1)
    flip = (nrm * grad).sum(1) > 0
    return verts, flip, pa, (pb - pa).argmax(-1)


def marching_cubes(sdf, level=0.0):
    """sdf (N,N,N) tensor indexed [ix,iy,iz] on the lattice of [-1,1]^3 -> triangle soup (F,3,3) of coordinates in
    [-1,1]^3 (sdf_meshing.py:83-101: vertex = origin + index * voxel_size), right-hand normals towards decreasing
    values.  Runs on the tensor's device."""
    res = _mc_triangles(sdf, level)
    if res is None:
        return torch.zeros(0, 3, 3, device=sdf.device)
    verts, flip = res[:2]
    return torch.where(flip[:, None, None], verts[:, [0, 2, 1]], verts)


def marching_cubes_indexed(sdf, level=0.0):
    """The level set of `marching_cubes` as an INDEXED mesh, the (verts, faces) pair of sdf_meshing.py:13-114: one vertex per
    crossing lattice edge.  The edge that leaves lattice point (ix, iy, iz) along axis a (0 x, 1 y, 2 z; a point on the last
    layer of an axis has no edge along it) has the key ((ix N + iy) N + iz) 3 + a and crosses when (sdf[lo] < level) !=
    (sdf[hi] < level).  -> verts (V,3): the crossing edges in ascending key order, interpolated with the soup's arithmetic (so
    verts[faces] IS marching_cubes(sdf), bit for bit); faces (F,3) int64: the soup's triangles in its order, corner for corner;
    vert_edge (V,) int64: the keys.  Plain tensor operations on the tensor's device: the specification of
    arah_marching_cubes_indexed (csrc/mcubes.hpp), and what runs for volumes that live on the host."""
    dev = sdf.device
    N = sdf.shape[0]
    vs = 2.0 / (N - 1)
    inside = sdf < level
    cross = torch.zeros(N, N, N, 3, dtype=torch.bool, device=dev)
    cross[:-1, :, :, 0] = inside[:-1] != inside[1:]
    cross[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    cross[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    cross = cross.reshape(-1)
    vert_edge = torch.nonzero(cross)[:, 0]                                   # ascending keys
    point, axis = vert_edge // 3, vert_edge % 3
    pa = torch.stack([point // (N * N), (point // N) % N, point % N], dim=1)
    pb = pa + torch.nn.functional.one_hot(axis, 3)
    va = sdf[pa[:, 0], pa[:, 1], pa[:, 2]] - level
    vb = sdf[pb[:, 0], pb[:, 1], pb[:, 2]] - level
    t = (va / (va - vb)).clamp(0.0, 1.0).unsqueeze(-1)
    verts = (pa.float() + t * (pb - pa).float()) * vs - 1.0
    res = _mc_triangles(sdf, level)
    if res is None:
        return verts, torch.zeros(0, 3, dtype=torch.int64, device=dev), vert_edge
    _, flip, lo, ax = res
    key = ((lo[..., 0] * N + lo[..., 1]) * N + lo[..., 2]) * 3 + ax           # (F,3)
    vert_of_key = torch.cumsum(cross.to(torch.int64), 0) - 1
    faces = vert_of_key[key]
    faces = torch.where(flip[:, None], faces[:, [0, 2, 1]], faces)
    return verts, faces, vert_edge


MC_DEFAULT_VERT_CAP = 1 << 19


def indexed_mesh(sdf, level=0.0):
    """The indexed mesh of a lattice volume, trimmed to its size: -> (verts (V,3) in [-1,1]^3, faces (F,3)).  On the GPU:
    hip.marching_cubes_indexed with the default capacities, ONE read of its counts (the host synchronisation) and a second run
    with the exact sizes when either capacity was too small -- nothing is truncated.  A volume on the host goes through
    `marching_cubes_indexed`."""
    if not sdf.is_cuda:
        verts, faces, _ = marching_cubes_indexed(sdf.float(), level)
        return verts, faces
    from . import hip
    vert_cap, face_cap = MC_DEFAULT_VERT_CAP, MC_DEFAULT_CAP
    verts, faces, counts = hip.marching_cubes_indexed(sdf, level, vert_cap, face_cap)
    V, F = counts.tolist()
    if V > vert_cap or F > face_cap:
        verts, faces, counts = hip.marching_cubes_indexed(sdf, level, max(V, 1), max(F, 1))
    return verts[:V], faces[:F]


def _cc_faces(faces, n_verts, what):
    faces = torch.as_tensor(faces)
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError("%s: faces must be an (F, 3) tensor" % what)
    if faces.dtype.is_floating_point or faces.dtype.is_complex or faces.dtype == torch.bool:
        raise ValueError("%s: faces must hold integer vertex ids" % what)
    if isinstance(n_verts, bool) or int(n_verts) != n_verts or not 0 <= int(n_verts) <= 2 ** 31 - 1:
        raise ValueError("%s: n_verts must be an integer in [0, 2^31), got %r" % (what, n_verts))
    faces = faces.long()
    return faces, int(n_verts), ((faces >= 0) & (faces < int(n_verts))).all(1)


def mesh_components(faces, n_verts):
    """Connected components of an indexed mesh by SHARED VERTEX IDS: faces (F,3) integer ids over n_verts vertices; two vertices
    are connected when a face names both (positions play no part); a face with an id outside [0, n_verts) is skipped; a vertex
    no valid face names is a component of its own with 0 faces.  -> labels (V,) int32: dense component ids in [0, C), components
    numbered in ascending order of their smallest vertex id; comp_verts, comp_faces (V,) int32: the sizes of component c, zero
    for c >= C; counts (3,) int32: C, the number of valid faces, the component with the most faces (ties: the lowest id; -1
    when C = 0).  Every vertex takes the smallest label among itself and the vertices it shares a face with, then its label's
    label, until nothing changes: the fixed point is the smallest vertex id of its component.  Plain tensor operations on the
    tensor's device: the specification of arah_mesh_components (csrc/meshcc.hpp), and what runs for meshes on the host."""
    faces, V, valid = _cc_faces(faces, n_verts, "mesh_components")
    dev = faces.device
    fv = faces[valid]
    ids = torch.arange(V, device=dev)
    low = ids.clone()
    while fv.shape[0]:
        new = low.scatter_reduce(0, fv.reshape(-1), low[fv].min(1).values.repeat_interleave(3), "amin")
        new = new[new]
        if torch.equal(new, low):
            break
        low = new
    is_root = low == ids
    labels = (torch.cumsum(is_root.long(), 0) - 1)[low]
    n_comp = int(is_root.sum())
    comp_verts = torch.bincount(labels, minlength=V)
    comp_faces = torch.bincount(labels[fv[:, 0]], minlength=V)
    if n_comp:
        most = comp_faces[:n_comp].max()
        largest = int(torch.nonzero(comp_faces[:n_comp] == most)[0, 0])
    else:
        largest = -1
    counts = torch.tensor([n_comp, int(fv.shape[0]), largest], dtype=torch.int32, device=dev)
    return labels.to(torch.int32), comp_verts.to(torch.int32), comp_faces.to(torch.int32), counts


def mesh_select(faces, n_verts, labels, keep):
    """Order-preserving selection of the components with keep[c] != 0: labels (V,) of `mesh_components`, keep (V,) integer or
    bool indexed by component id.  A vertex is kept when its component is (a label outside [0, V) keeps nothing); a face when its
    ids are valid and its three vertices are kept.  -> vert_src (V,) int32: the old id of new vertex j, in the original order;
    vert_map (V,) int32: the new id of old vertex v, or -1; faces_out (F,3) int32: the kept faces in their original order with
    the new ids; face_src (F,) int32: their old rows; counts (2,) int32: kept vertices, kept faces.  Rows beyond a count are
    zero.  The specification of arah_mesh_select (csrc/meshcc.hpp)."""
    faces, V, valid = _cc_faces(faces, n_verts, "mesh_select")
    dev, F = faces.device, faces.shape[0]
    for name, t in (("labels", labels), ("keep", keep)):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != (V,) or t.dtype.is_floating_point or t.dtype.is_complex:
            raise ValueError("mesh_select: %s must be an integer tensor of shape (%d,)" % (name, V))
    labels = labels.to(dev).long()
    in_range = (labels >= 0) & (labels < V)
    kept_v = in_range & (keep.to(dev)[labels.clamp(0, max(V - 1, 0))] != 0) if V else torch.zeros(0, dtype=torch.bool, device=dev)
    src_v = torch.nonzero(kept_v)[:, 0]
    vert_map = torch.full((V,), -1, dtype=torch.int64, device=dev)
    vert_map[src_v] = torch.arange(src_v.shape[0], device=dev)
    kept_f = valid.clone()
    kept_f[valid] = kept_v[faces[valid]].all(1)
    src_f = torch.nonzero(kept_f)[:, 0]
    vert_src = torch.zeros(V, dtype=torch.int64, device=dev)
    vert_src[:src_v.shape[0]] = src_v
    faces_out = torch.zeros(F, 3, dtype=torch.int64, device=dev)
    faces_out[:src_f.shape[0]] = vert_map[faces[src_f]]
    face_src = torch.zeros(F, dtype=torch.int64, device=dev)
    face_src[:src_f.shape[0]] = src_f
    counts = torch.tensor([src_v.shape[0], src_f.shape[0]], dtype=torch.int32, device=dev)
    i32 = torch.int32
    return vert_src.to(i32), vert_map.to(i32), faces_out.to(i32), face_src.to(i32), counts


SIMPLIFY_MAX_CELLS = 1 << 27            # cells of a clustering grid
SIMPLIFY_MAX_VERTS = 1 << 26            # vertices: 2^26 fixed-point coordinates below 2^36 sum below 2^62
SIMPLIFY_MAX_FACES = 1 << 28            # faces: the duplicate table has at least twice as many slots
SIMPLIFY_MAX_DEDUP_CLUSTERS = 1 << 21   # three sorted 21-bit cluster ids make the 64-bit key of a face
SIMPLIFY_FIX_BITS = 36                  # fixed-point coordinates inside the grid lie in [0, 2^36]


def simplify_grid(origin, cell, dims, what="mesh_simplify"):
    """A clustering grid, checked: origin three finite numbers, cell a number whose float32 value and float32 reciprocal are
    positive and finite, dims three integers >= 1 with at most 2^27 cells in all.  -> (origin as three float32 values, cell as a
    float32 value, the float32 reciprocal, dims as ints, fix_scale = 2^(36 - e) with e = ceil(log2(max(dims) cell)) as a
    float: a power of two, so that the fixed-point coordinates of a vertex inside the grid lie in [0, 2^36])."""
    try:
        o = [float(np.float32(float(x))) for x in (origin.tolist() if isinstance(origin, torch.Tensor) else origin)]
        d = [int(x) for x in (dims.tolist() if isinstance(dims, torch.Tensor) else dims)]
        whole = all(float(x) == int(x) for x in (dims.tolist() if isinstance(dims, torch.Tensor) else dims))
        c = float(np.float32(float(cell)))
    except (TypeError, ValueError, OverflowError):
        raise ValueError("%s: origin must be three numbers, cell a number, dims three integers" % what)
    if len(o) != 3 or not all(math.isfinite(x) for x in o):
        raise ValueError("%s: origin must be three finite numbers, got %r" % (what, origin))
    inv = float(np.float32(1.0) / np.float32(c)) if c > 0.0 and math.isfinite(c) else float("inf")
    if not math.isfinite(inv):
        raise ValueError("%s: cell must be a positive float32 length with a finite reciprocal, got %r" % (what, cell))
    if len(d) != 3 or not whole or min(d) < 1 or d[0] * d[1] * d[2] > SIMPLIFY_MAX_CELLS:
        raise ValueError("%s: dims must be three integers >= 1 with at most 2^27 cells in all, got %r" % (what, dims))
    m, e = math.frexp(max(d) * c)                  # max(d) c = m 2^e exactly (the product of two floats below 2^53), 0.5 <= m < 1
    e = e - 1 if m == 0.5 else e                   # ceil(log2(.))
    return o, c, inv, d, math.ldexp(1.0, SIMPLIFY_FIX_BITS - e)


def mesh_simplify(verts, faces, origin, cell, dims, position="mean", dedup=True):
    """Vertex clustering of an indexed mesh on a grid: verts (V,3) float32, faces (F,3) integer ids, the grid of `simplify_grid`.

    Cell of a vertex, in float32: c = clamp(floor((v - origin) (1 / cell)), 0, dims - 1) per axis, key = cx + nx (cy + ny cz).  A
    vertex with a non-finite coordinate is invalid and has no cell.  The clusters are the occupied cells, numbered 0 .. K - 1 in
    ascending key.  Position of a cluster, exactly: q = llrint(clamp((double(v) - double(origin)) fix_scale, -2^36, 2^36)) per
    member (the clamp only touches vertices outside the grid), S = sum q and n = the members in integers, mean = float32(
    double(origin) + (double(S) / double(n)) / fix_scale).  Its representative: the member with the smallest d^2 = float32((dx dx
    + dy dy) + dz dz), d = double(v) - double(mean), every operation rounded on its own; ties go to the lowest vertex id.

    A face with an id outside [0, V) or an invalid vertex is dropped (n_invalid); the others are renamed to clusters, dropped as
    collapsed when two of the three are equal, and with `dedup` dropped as duplicates when an earlier surviving face names the
    same three clusters in any order.  With dedup and K > 2^21 the status is 1 and no face is kept (nor counted as a duplicate).

    -> verts_out (V,3) float32: the clusters' means (position="mean") or representatives (position="member"); vert_src (V,)
    int32: the representatives' ids; vert_map (V,) int32: the cluster of every vertex or -1; faces_out (F,3) int32: the kept
    faces in their original order and orientation, as cluster ids; face_src (F,) int32: their old rows; counts (6,) int32: K,
    kept faces, n_invalid, collapsed, duplicates, status.  Rows beyond K and beyond the kept faces are zero.  Clusters that lose
    all their faces stay.  Plain tensor operations on the tensors' device: the specification of arah_mesh_simplify
    (csrc/meshsimp.hpp), and what runs for meshes on the host."""
    if position not in ("mean", "member"):
        raise ValueError("mesh_simplify: position must be 'mean' or 'member', got %r" % (position,))
    if not isinstance(verts, torch.Tensor) or verts.dim() != 2 or verts.shape[1] != 3 or verts.dtype != torch.float32:
        raise ValueError("mesh_simplify: verts must be a (V, 3) float32 tensor")
    V = int(verts.shape[0])
    faces, _, in_range = _cc_faces(faces, V, "mesh_simplify")
    if faces.device != verts.device:
        raise ValueError("mesh_simplify: verts live on %s, faces on %s" % (verts.device, faces.device))
    F = int(faces.shape[0])
    if V > SIMPLIFY_MAX_VERTS or F > SIMPLIFY_MAX_FACES:
        raise ValueError("mesh_simplify: at most 2^26 vertices and 2^28 faces, got %d and %d" % (V, F))
    o, c, inv, d, scale = simplify_grid(origin, cell, dims)
    dev, i32, f64 = verts.device, torch.int32, torch.float64
    verts = verts.detach()
    o32 = torch.tensor(o, dtype=torch.float32, device=dev)
    valid = torch.isfinite(verts).all(1)
    # cells: one float32 subtraction, one float32 multiplication
    t = torch.floor((verts - o32) * torch.tensor(inv, dtype=torch.float32, device=dev))
    ci = torch.where(valid[:, None], t.clamp(0.0, float(SIMPLIFY_MAX_CELLS)), torch.zeros_like(t)).long()
    ci = torch.minimum(ci, torch.tensor([x - 1 for x in d], device=dev))      # in integers: dims - 1 need not be a float32
    key = ci[:, 0] + d[0] * (ci[:, 1] + d[1] * ci[:, 2])
    ids_v = torch.nonzero(valid)[:, 0]
    _, inverse = torch.unique(key[ids_v], sorted=True, return_inverse=True)
    K = int(inverse.max()) + 1 if ids_v.shape[0] else 0
    vert_map = torch.full((V,), -1, dtype=torch.int64, device=dev)
    vert_map[ids_v] = inverse
    # exact means
    o64 = o32.to(f64)
    q = torch.clamp((verts[ids_v].to(f64) - o64) * scale, -2.0 ** SIMPLIFY_FIX_BITS, 2.0 ** SIMPLIFY_FIX_BITS).round().long()
    S = torch.zeros(K, 3, dtype=torch.int64, device=dev).index_add_(0, inverse, q)
    n = torch.bincount(inverse, minlength=K)
    mean = (o64 + (S.to(f64) / n.to(f64)[:, None]) / scale).float()
    # representatives: the smallest (bits(d2) << 32) | id per cluster
    dd = verts[ids_v].to(f64) - mean[inverse].to(f64)
    d2 = ((dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]).float()
    packed = (d2.view(i32).long() << 32) | ids_v
    best = torch.full((K,), 2 ** 63 - 1, dtype=torch.int64, device=dev).scatter_reduce(0, inverse, packed, "amin")
    src = best & 0xFFFFFFFF
    vert_src = torch.zeros(V, dtype=torch.int64, device=dev)
    vert_src[:K] = src
    verts_out = torch.zeros(V, 3, dtype=torch.float32, device=dev)
    verts_out[:K] = mean if position == "mean" else verts[src]
    # faces
    ok = in_range.clone()
    ok[in_range] = valid[faces[in_range]].all(1)
    rows = torch.nonzero(ok)[:, 0]
    cl = vert_map[faces[rows]]
    apart = (cl[:, 0] != cl[:, 1]) & (cl[:, 1] != cl[:, 2]) & (cl[:, 0] != cl[:, 2])
    n_invalid, n_collapsed = F - int(rows.shape[0]), int(rows.shape[0]) - int(apart.sum())
    rows, cl = rows[apart], cl[apart]
    status = int(bool(dedup) and K > SIMPLIFY_MAX_DEDUP_CLUSTERS)
    n_dup = 0
    if status:
        rows, cl = rows[:0], cl[:0]
    elif dedup and rows.shape[0]:
        s = torch.sort(cl, dim=1).values
        _, which = torch.unique(s[:, 0] | (s[:, 1] << 21) | (s[:, 2] << 42), return_inverse=True)
        first = torch.full((int(which.max()) + 1,), F, dtype=torch.int64, device=dev).scatter_reduce(0, which, rows, "amin")
        first_seen = first[which] == rows
        n_dup = int(rows.shape[0]) - int(first_seen.sum())
        rows, cl = rows[first_seen], cl[first_seen]
    kept = int(rows.shape[0])
    faces_out = torch.zeros(F, 3, dtype=torch.int64, device=dev)
    faces_out[:kept] = cl
    face_src = torch.zeros(F, dtype=torch.int64, device=dev)
    face_src[:kept] = rows
    counts = torch.tensor([K, kept, n_invalid, n_collapsed, n_dup, status], dtype=i32, device=dev)
    return verts_out, vert_src.to(i32), vert_map.to(i32), faces_out.to(i32), face_src.to(i32), counts


QUADRIC_MAX_SEGMENT = 1 << 15           # (face, cluster) pairs of one cluster that are still placed: the segment is rank-sorted


def quadric_tree_sum(x, start, n):
    """The fixed in-place tree of `mesh_quadric_place` over the flat rows x (P, C): segment k is x[start[k] : start[k] + n[k]];
    for stride = 1, 2, 4, ... while stride < n: x[i] += x[i + stride] for every local i that is a multiple of 2 stride with
    i + stride < n.  -> (K, C): every segment's x[0], zeros for an empty segment.  The shape of the tree depends on n alone."""
    K, P = int(n.shape[0]), int(x.shape[0])
    x = x.clone()
    if P:
        seg = torch.repeat_interleave(torch.arange(K, device=x.device), n)
        local = torch.arange(P, device=x.device) - start[seg]
        length = n[seg]
        stride, n_max = 1, int(n.max())
        while stride < n_max:
            at = torch.nonzero((local % (2 * stride) == 0) & (local + stride < length))[:, 0]
            x[at] = x[at] + x[at + stride]      # a target is a multiple of 2 stride, a source is not: no row is both
            stride *= 2
    out = torch.zeros(K, x.shape[1], dtype=x.dtype, device=x.device)
    has = torch.nonzero(n > 0)[:, 0]
    out[has] = x[start[has]]
    return out


def quadric_terms(verts, corners, about, with_c=False):
    """The terms of `mesh_quadric_place`: corners (P,3) vertex ids of P faces, about (P,3) float64 the point each is taken about.
    -> (P,9) float64 A00 A01 A02 A11 A12 A22 b0 b1 b2; with_c: a tenth column d d, the constant of the quadric."""
    f64 = torch.float64
    pa, pb, pc = (verts[corners[:, j]].to(f64) - about for j in range(3))
    e1, e2 = pb - pa, pc - pa
    nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    d = -((nx * pa[:, 0] + ny * pa[:, 1]) + nz * pa[:, 2])
    cols = [nx * nx, nx * ny, nx * nz, ny * ny, ny * nz, nz * nz, nx * d, ny * d, nz * d]
    return torch.stack(cols + ([d * d] if with_c else []), 1)


def quadric_solve(q, reg, bound):
    """The solve of `mesh_quadric_place` over the rows of q (K, >= 9) float64: -> (y (K,3) float64 the offsets, good (K,) bool:
    t and det finite and > 0 and every |y_a| finite and <= bound (a number or a (K,) float64 tensor))."""
    A00, A01, A02, A11, A12, A22, b0, b1, b2 = (q[:, j] for j in range(9))
    t = (A00 + A11) + A22
    lam = reg * t
    M00, M11, M22, M01, M02, M12 = A00 + lam, A11 + lam, A22 + lam, A01, A02, A12
    C00 = M11 * M22 - M12 * M12
    C01 = M02 * M12 - M01 * M22
    C02 = M01 * M12 - M02 * M11
    C11 = M00 * M22 - M02 * M02
    C12 = M01 * M02 - M00 * M12
    C22 = M00 * M11 - M01 * M01
    det = (M00 * C00 + M01 * C01) + M02 * C02
    y = torch.stack([-((C00 * b0 + C01 * b1) + C02 * b2) / det, -((C01 * b0 + C11 * b1) + C12 * b2) / det,
                     -((C02 * b0 + C12 * b1) + C22 * b2) / det], 1)
    bound = bound[:, None] if isinstance(bound, torch.Tensor) else bound
    good = torch.isfinite(t) & (t > 0) & torch.isfinite(det) & (det > 0) & (torch.isfinite(y) & (y.abs() <= bound)).all(1)
    return y, good


def mesh_quadric_place(verts, faces, vert_map, means, n_clusters, cell, reg=1e-3):
    """Quadric-error placement of the clusters of `mesh_simplify`: verts (V,3) float32, faces (F,3) integer ids, vert_map (V,)
    integer (the cluster of every vertex or -1), means (V,3) float32 (verts_out at position="mean"), n_clusters = K (an integer,
    or the counts of mesh_simplify: K at [0]; clamped to [0, V]), cell the float32 cell length (> 0), reg a finite double >= 0.

    A face is VALID when its three ids lie in [0, V) and vert_map lies in [0, K) for all three; a repeated id is fine (the
    normal is zero).  A valid face contributes once to each of the one, two or three distinct clusters of its corners --
    collapsed and duplicate faces too: they carry the local shape.  Everything below is float64, every operation rounded on its
    own, no square root.  Term of face f = (a, b, c) for cluster k, with m = double(means[k]): pa = double(a) - m, pb, pc
    likewise; e1 = pb - pa, e2 = pc - pa; n = e1 x e2, every component (x y) - (z w); d = -((n0 pa0 + n1 pa1) + n2 pa2); the
    nine numbers A00 A01 A02 A11 A12 A22 = ni nj and b0 b1 b2 = ni d: Lindstrom's area^2-weighted plane quadric about the mean.
    The terms of a cluster are listed in ascending face id and summed by the fixed tree of `quadric_tree_sum`.  Solve: t = (A00
    + A11) + A22; M = A + (reg t) I; the cofactors C00 = M11 M22 - M12 M12, C01 = M02 M12 - M01 M22, C02 = M01 M12 - M02 M11,
    C11 = M00 M22 - M02 M02, C12 = M01 M02 - M00 M12, C22 = M00 M11 - M01 M01; det = (M00 C00 + M01 C01) + M02 C02; y = -(C b) /
    det, every row summed left to right and divided once; pos[k] = float32(m + y).  The cluster FALLS BACK to pos[k] = means[k],
    and is counted, when t or det is not finite or not > 0, or a |y_a| is not finite or > double(cell).  A cluster with more
    than 2^15 pairs is not placed at all (pos = mean, not counted) and sets the status 2.  Representative: the member with the
    smallest float32((dx dx + dy dy) + dz dz), d = double(v) - double(pos[k]), ties to the lowest id (0 for a cluster without a
    member).

    -> pos (V,3) float32, vert_src (V,) int32, qcounts (4,) int32 = clusters that fell back, (face, cluster) pairs, the longest
    segment, the status.  Rows from K on are zero.  Plain tensor operations on the tensors' device: the specification of
    arah_mesh_quadric_place (csrc/meshquadric.hpp), and what runs for meshes on the host."""
    what = "mesh_quadric_place"
    if not isinstance(verts, torch.Tensor) or verts.dim() != 2 or verts.shape[1] != 3 or verts.dtype != torch.float32:
        raise ValueError("%s: verts must be a (V, 3) float32 tensor" % what)
    V = int(verts.shape[0])
    faces, _, in_range = _cc_faces(faces, V, what)
    F = int(faces.shape[0])
    if V > SIMPLIFY_MAX_VERTS or F > SIMPLIFY_MAX_FACES:
        raise ValueError("%s: at most 2^26 vertices and 2^28 faces, got %d and %d" % (what, V, F))
    if not isinstance(means, torch.Tensor) or tuple(means.shape) != (V, 3) or means.dtype != torch.float32:
        raise ValueError("%s: means must be a (%d, 3) float32 tensor" % (what, V))
    if (not isinstance(vert_map, torch.Tensor) or tuple(vert_map.shape) != (V,) or vert_map.dtype.is_floating_point
            or vert_map.dtype.is_complex or vert_map.dtype == torch.bool):
        raise ValueError("%s: vert_map must be an integer tensor of shape (%d,)" % (what, V))
    dev = verts.device
    if faces.device != dev or means.device != dev or vert_map.device != dev:
        raise ValueError("%s: verts, faces, vert_map and means must live on one device" % what)
    K, c, reg = quadric_args(n_clusters, cell, reg, V, what)
    f64, i32 = torch.float64, torch.int32
    verts, means, vmap = verts.detach(), means.detach(), vert_map.detach().long()
    member = (vmap >= 0) & (vmap < K)
    ok = in_range.clone()
    ok[in_range] = member[faces[in_range]].all(1)
    rows = torch.nonzero(ok)[:, 0]
    cl = vmap[faces[rows]]                                                      # (Fv,3) clusters of the corners
    first = torch.stack([torch.ones_like(cl[:, 0], dtype=torch.bool), cl[:, 1] != cl[:, 0],
                         (cl[:, 2] != cl[:, 0]) & (cl[:, 2] != cl[:, 1])], 1)   # a cluster counts at its first corner
    pf, pk = rows[:, None].expand(-1, 3)[first], cl[first]
    order = torch.argsort(pk * max(F, 1) + pf)                                  # (cluster, face): unique keys
    pf, pk = pf[order], pk[order]
    n = torch.bincount(pk, minlength=K)[:K] if K else torch.zeros(0, dtype=torch.int64, device=dev)
    start = torch.cumsum(n, 0) - n
    longest = int(n.max()) if K else 0
    placed = n <= QUADRIC_MAX_SEGMENT
    m = means[:K].to(f64)
    # the terms
    terms = quadric_terms(verts, faces[pf], m[pk])
    keep = placed[pk]                                                           # a skipped segment is not summed
    n_sum = torch.where(placed, n, torch.zeros_like(n))
    q = quadric_tree_sum(terms[keep], torch.cumsum(n_sum, 0) - n_sum, n_sum)
    y, good = quadric_solve(q, reg, c)
    moved = (m + y).float()
    pos_k = torch.where((good & placed)[:, None], moved, means[:K])
    fallbacks = int((placed & ~good).sum())
    status = 2 if longest > QUADRIC_MAX_SEGMENT else 0
    # representatives: the smallest (bits(d2) << 32) | id per cluster
    ids_v = torch.nonzero(member)[:, 0]
    inv = vmap[ids_v]
    dd = verts[ids_v].to(f64) - pos_k[inv].to(f64)
    d2 = ((dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]).float()
    packed = ((d2.view(i32).long() & 0x7FFFFFFF) << 32) | ids_v
    best = torch.full((K,), 2 ** 63 - 1, dtype=torch.int64, device=dev).scatter_reduce(0, inv, packed, "amin")
    src = torch.where(best == 2 ** 63 - 1, torch.zeros_like(best), best & 0xFFFFFFFF)
    pos = torch.zeros(V, 3, dtype=torch.float32, device=dev)
    pos[:K] = pos_k
    vert_src = torch.zeros(V, dtype=torch.int64, device=dev)
    vert_src[:K] = src
    qcounts = torch.tensor([fallbacks, int(pf.shape[0]), longest, status], dtype=i32, device=dev)
    return pos, vert_src.to(i32), qcounts


def quadric_args(n_clusters, cell, reg, n_verts, what="mesh_quadric_place"):
    """The scalars of `mesh_quadric_place`, checked: -> (K clamped to [0, V], cell as a float32 value, reg as a float)."""
    try:
        if isinstance(n_clusters, torch.Tensor):
            if n_clusters.dtype.is_floating_point or n_clusters.numel() < 1:
                raise TypeError
            K = int(n_clusters.reshape(-1)[0])
        else:
            if isinstance(n_clusters, bool) or int(n_clusters) != n_clusters:
                raise TypeError
            K = int(n_clusters)
        c = float(np.float32(float(cell)))
        reg = float(reg)
    except (TypeError, ValueError, OverflowError):
        raise ValueError("%s: n_clusters must be an integer (or the counts of mesh_simplify), cell and reg numbers" % what)
    if not math.isfinite(c) or not c > 0.0:
        raise ValueError("%s: cell must be a finite float32 length > 0, got %r" % (what, cell))
    if not math.isfinite(reg) or reg < 0.0:
        raise ValueError("%s: reg must be a finite number >= 0, got %r" % (what, reg))
    return min(max(K, 0), n_verts), c, reg


ADJACENCY_MAX_FACES = 1 << 28           # 6 F neighbour entries fit an int32
ADJACENCY_FIELDS = ("vf_start", "vf", "nbr_start", "nbr", "nbr_out", "nbr_in", "vert_flags", "counts")


def _csr_start(rows, V, dev):
    """(V+1,) int32 starts of the CSR whose entries lie in the rows `rows` (sorted or not)."""
    start = torch.zeros(V + 1, dtype=torch.int64, device=dev)
    start[1:] = torch.cumsum(torch.bincount(rows, minlength=V), 0)
    return start.to(torch.int32)


def mesh_adjacency(faces, n_verts):
    """Who is adjacent to whom in an indexed mesh: faces (F,3) integer ids over V = n_verts vertices, F <= 2^28.  A face is VALID
    when its three ids lie in [0, V) and are pairwise different; the others are skipped.  A valid face (a, b, c) traverses the
    directed edges a->b, b->c, c->a.  -> a tuple of

        vf_start (V+1,), vf (3F,) int32     CSR of the valid faces incident to every vertex, face ids ascending within a vertex;
                                            rows from vf_start[V] on are zero
        nbr_start (V+1,), nbr (6F,) int32   CSR of the UNIQUE neighbours of every vertex, ids ascending
        nbr_out, nbr_in (6F,) int32         for the entry (v, n): the valid faces traversing v->n, and n->v; rows from
                                            nbr_start[V] on are zero (nbr's too)
        vert_flags (V,) uint8               bit 0: the vertex has an edge with exactly one face; bit 1: an edge with three or more
                                            faces; bit 2: no neighbour
        counts (8,) int32                   valid faces; undirected edges E; edges with one face (boundary); with >= 3 faces (non-
                                            manifold); with exactly two faces that traverse it in the same direction (misoriented);
                                            the largest number of neighbours of a vertex; vertices with no neighbour; the Euler
                                            characteristic (V - counts[6]) - E + counts[0]

    Integers throughout: the result is unique.  Plain tensor operations on the tensor's device: the specification of
    arah_mesh_adjacency (csrc/meshadj.hpp), and what runs for meshes on the host."""
    faces, V, in_range = _cc_faces(faces, n_verts, "mesh_adjacency")
    dev, F, i32 = faces.device, int(faces.shape[0]), torch.int32
    if F > ADJACENCY_MAX_FACES:
        raise ValueError("mesh_adjacency: at most 2^28 faces, got %d" % F)
    valid = in_range & (faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])
    rows = torch.nonzero(valid)[:, 0]
    fv = faces[rows]                                                            # (Fv,3)
    n_valid = int(rows.shape[0])
    # incident faces: the corners sorted by (vertex, face); a valid face names a vertex once, so the keys are unique
    key = torch.sort(fv.reshape(-1) * max(F, 1) + rows.repeat_interleave(3)).values
    vf = torch.zeros(3 * F, dtype=torch.int64, device=dev)
    vf[:3 * n_valid] = key % max(F, 1)
    vf_start = _csr_start(key // max(F, 1), V, dev)
    # neighbours: every directed edge s->d is an "out" of the entry (s, d) and an "in" of the entry (d, s)
    s, d = fv.reshape(-1), fv[:, [1, 2, 0]].reshape(-1)
    W = max(V, 1)
    ekey, which = torch.unique(torch.cat([s * W + d, d * W + s]), sorted=True, return_inverse=True)
    n_ent = int(ekey.shape[0])
    one, zero = torch.ones_like(s), torch.zeros_like(s)
    out = torch.zeros(n_ent, dtype=torch.int64, device=dev).index_add_(0, which, torch.cat([one, zero]))
    inn = torch.zeros(n_ent, dtype=torch.int64, device=dev).index_add_(0, which, torch.cat([zero, one]))
    ev, en = ekey // W, ekey % W
    nbr, nbr_out, nbr_in = (torch.zeros(6 * F, dtype=torch.int64, device=dev) for _ in range(3))
    nbr[:n_ent], nbr_out[:n_ent], nbr_in[:n_ent] = en, out, inn
    nbr_start = _csr_start(ev, V, dev)
    tot = out + inn
    valence = torch.bincount(ev, minlength=V)
    flags = torch.zeros(V, dtype=torch.int64, device=dev)
    flags[ev[tot == 1]] |= 1
    flags[ev[tot >= 3]] |= 2
    flags[valence == 0] |= 4
    up = en > ev                                                                # every undirected edge once
    n_edges, isolated = int(up.sum()), int((valence == 0).sum())
    counts = torch.tensor([n_valid, n_edges, int((up & (tot == 1)).sum()), int((up & (tot >= 3)).sum()),
                           int((up & (tot == 2) & (out != 1)).sum()), int(valence.max()) if V else 0, isolated,
                           (V - isolated) - n_edges + n_valid], dtype=i32, device=dev)
    return vf_start, vf.to(i32), nbr_start, nbr.to(i32), nbr_out.to(i32), nbr_in.to(i32), flags.to(torch.uint8), counts


def _adjacency_of(faces, n_verts, adjacency, what):
    """The eight arrays of `mesh_adjacency`, built here or taken from the caller (checked for their shapes only)."""
    if adjacency is None:
        return mesh_adjacency(faces, n_verts)
    adjacency = tuple(adjacency)
    F = int(faces.shape[0])
    shapes = ((n_verts + 1,), (3 * F,), (n_verts + 1,), (6 * F,), (6 * F,), (6 * F,), (n_verts,), (8,))
    if len(adjacency) != 8 or any(not isinstance(t, torch.Tensor) or tuple(t.shape) != s for t, s in zip(adjacency, shapes)):
        raise ValueError("%s: adjacency must be the eight arrays of mesh_adjacency of these faces and vertices" % what)
    return adjacency


def _mesh_verts(verts, faces, what):
    if not isinstance(verts, torch.Tensor) or verts.dim() != 2 or verts.shape[1] != 3 or verts.dtype != torch.float32:
        raise ValueError("%s: verts must be a (V, 3) float32 tensor" % what)
    V = int(verts.shape[0])
    faces, _, in_range = _cc_faces(faces, V, what)
    if faces.device != verts.device:
        raise ValueError("%s: verts live on %s, faces on %s" % (what, verts.device, faces.device))
    if int(faces.shape[0]) > ADJACENCY_MAX_FACES:
        raise ValueError("%s: at most 2^28 faces, got %d" % (what, int(faces.shape[0])))
    return verts.detach(), faces, V, in_range


def vertex_normals(verts, faces, adjacency=None):
    """Per-vertex normals of an indexed mesh from the mesh itself, pytorch3d's verts_normals_packed: the area-weighted sum of the
    incident faces' cross products.  verts (V,3) float32, faces (F,3) integer ids, adjacency: `mesh_adjacency` of them, or None.

    For vertex v its incident valid faces are walked in ascending id.  A face with a non-finite corner contributes nothing; the
    others n_f = (p1 - p0) x (p2 - p0), corners widened to float64, every subtraction, product and difference rounded on its own.
    acc starts at 0 and takes acc = acc + n_f in that order.  -> normal_sum (V,3) float64 = acc, normals (V,3) float32 =
    float32(acc / sqrt((ax ax + ay ay) + az az)), (0, 0, 0) when that length is 0 or not finite.  The ordered sum is a loop over
    k < the most incident faces of a padded gather (adding 0.0 for the padding is exact).  The specification of
    arah_mesh_vertex_normals (csrc/meshadj.hpp), and what runs for meshes on the host."""
    verts, faces, V, _ = _mesh_verts(verts, faces, "vertex_normals")
    vf_start, vf = _adjacency_of(faces, V, adjacency, "vertex_normals")[:2]
    dev, f64, F = verts.device, torch.float64, int(faces.shape[0])
    acc = torch.zeros(V, 3, dtype=f64, device=dev)
    if V == 0 or F == 0:
        return acc, acc.float()
    p = verts.to(f64)[faces.clamp(0, V - 1)]                                    # (F,3,3); rows of skipped faces are never read
    a, b = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    nf = torch.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                      a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], dim=1)
    nf = torch.where(torch.isfinite(p).all(2).all(1)[:, None], nf, torch.zeros_like(nf))
    start = vf_start.long()
    first, deg = start[:-1], start[1:] - start[:-1]
    vfl = vf.long()
    for k in range(int(deg.max())):
        has = k < deg
        f = vfl[(first + k).clamp(max=3 * F - 1)]
        acc = acc + torch.where(has[:, None], nf[f], torch.zeros_like(acc))
    length = torch.sqrt((acc[:, 0] * acc[:, 0] + acc[:, 1] * acc[:, 1]) + acc[:, 2] * acc[:, 2])
    ok = torch.isfinite(length) & (length > 0)
    unit = acc / torch.where(ok, length, torch.ones_like(length))[:, None]
    return acc, torch.where(ok[:, None], unit, torch.zeros_like(unit)).float()


def check_smooth_args(iterations, lamb, mu, method, boundary, what="mesh_smooth"):
    """The arguments of `mesh_smooth`, checked: -> (the steps' factors as float32 values widened to Python floats, one per
    step of an iteration; pin as a bool)."""
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or int(iterations) < 0:
        raise ValueError("%s: iterations must be an integer >= 0, got %r" % (what, iterations))
    for name, x in (("lamb", lamb), ("mu", mu)):
        if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or not math.isfinite(float(x)):
            raise ValueError("%s: %s must be a finite number, got %r" % (what, name, x))
    if not 0.0 < float(lamb) <= 1.0:
        raise ValueError("%s: lamb must lie in (0, 1], got %r" % (what, lamb))
    if not -1.1 <= float(mu) < 0.0:
        raise ValueError("%s: mu must lie in [-1.1, 0), got %r" % (what, mu))
    if method not in ("taubin", "laplacian"):
        raise ValueError("%s: method must be 'taubin' or 'laplacian', got %r" % (what, method))
    if boundary not in ("pin", "free"):
        raise ValueError("%s: boundary must be 'pin' or 'free', got %r" % (what, boundary))
    lam32, mu32 = float(np.float32(float(lamb))), float(np.float32(float(mu)))
    return ((lam32, mu32) if method == "taubin" else (lam32,)), boundary == "pin"


def check_smooth_weights(weights, what="mesh_smooth"):
    if not isinstance(weights, str) or weights not in ("uniform", "cotangent"):
        raise ValueError("%s: weights must be 'uniform' or 'cotangent', got %r" % (what, weights))
    return weights


def mesh_smooth(verts, faces, iterations, lamb=0.5, mu=-0.53, method="taubin", boundary="pin", adjacency=None, weights="uniform"):
    """Umbrella smoothing of an indexed mesh: verts (V,3) float32, faces (F,3) integer ids, adjacency: `mesh_adjacency` of them, or
    None.  One STEP with the factor f (the float32 value of lamb or mu, widened to float64): a vertex moves when it is finite, is
    not pinned and has a finite neighbour; s = the float64 sum of its finite unique neighbours in ascending id, m their number,
    new = float32(p + f (s / m - p)) in float64, every operation rounded on its own.  All other vertices are copied bit for
    bit.  A step reads the previous step's positions only.  method="taubin": an iteration is a lamb step and then a mu step
    (Taubin 1995: the second, negative step undoes the shrinkage of the first); "laplacian": a lamb step only.  boundary="pin":
    the vertices with vert_flags bit 0 or 1 (on a boundary or a non-manifold edge) never move; "free": they move like the others.
    lamb in (0, 1], mu in [-1.1, 0), iterations >= 0.  -> verts_out (V,3) float32; faces, the vertex count and the order stay.
    The specification of arah_mesh_smooth (csrc/meshadj.hpp), and what runs for meshes on the host.

    weights="cotangent" (the default "uniform" is the rule above): every step first takes weight = `mesh_cotangent` (mass
    "mixed"; the weights do not depend on it) of the positions it reads, and uses the entries (v, n) whose neighbour is finite and
    whose weight is finite.  A vertex moves when it is finite, is not pinned and s = the sum of |weight| over those entries in
    ascending neighbour id is finite and > 0: acc = the sum of weight (q - p) over the same entries in the same order, the weights
    with their own signs, new = float32(p + f (acc / s)).  The step is the explicit mean-curvature flow, normalised by the weights
    (not by the area) so that lamb keeps its meaning.  On a flat patch acc vanishes, whatever the sampling and whether or not the
    triangulation is Delaunay; clamping the negative weights at 0 would lose exactly that (one step then moves the interior
    vertices of a jittered planar grid by 5 % of a cell), so nothing is clamped, and |weight| in the denominator keeps every step
    inside the vertex's 1-ring: |acc| / s <= max |q - p|.  The specification of arah_mesh_smooth_cotangent
    (csrc/meshlaplace.hpp)."""
    factors, pin = check_smooth_args(iterations, lamb, mu, method, boundary)
    check_smooth_weights(weights)
    verts, faces, V, _ = _mesh_verts(verts, faces, "mesh_smooth")
    adjacency = _adjacency_of(faces, V, adjacency, "mesh_smooth")
    if weights == "cotangent":
        return _mesh_smooth_cotangent(verts, faces, V, int(iterations), factors, pin, adjacency)
    nbr_start, nbr, flags = adjacency[2], adjacency[3], adjacency[6]
    cur = verts.clone()
    F = int(faces.shape[0])
    if V == 0 or F == 0 or int(iterations) == 0:
        return cur
    f64 = torch.float64
    start = nbr_start.long()
    first, deg = start[:-1], start[1:] - start[:-1]
    width = int(deg.max())
    free = (flags & 3) == 0 if pin else torch.ones(V, dtype=torch.bool, device=verts.device)
    nb = nbr.long()
    for step in range(int(iterations) * len(factors)):
        f = factors[step % len(factors)]
        p = cur.to(f64)
        finite = torch.isfinite(cur).all(1)
        s = torch.zeros(V, 3, dtype=f64, device=verts.device)
        m = torch.zeros(V, dtype=f64, device=verts.device)
        for k in range(width):
            n = nb[(first + k).clamp(max=6 * F - 1)]
            has = (k < deg) & finite[n]
            s = s + torch.where(has[:, None], p[n], torch.zeros_like(s))
            m = m + has.to(f64)
        moves = finite & free & (m > 0)
        new = (p + f * (s / m.clamp_min(1.0)[:, None] - p)).float()
        cur = torch.where(moves[:, None], new, cur)
    return cur


def check_tangential_lamb(lamb, what="mesh_tangential_step"):
    """lamb of the tangential step, checked: -> its float32 value widened to a Python float."""
    if isinstance(lamb, bool) or not isinstance(lamb, (int, float, np.integer, np.floating)) or not 0.0 < float(lamb) <= 1.0:
        raise ValueError("%s: lamb must be a number in (0, 1], got %r" % (what, lamb))
    return float(np.float32(float(lamb)))


def mesh_tangential_step(verts, faces, normal_sum, lamb=0.5, adjacency=None):
    """One step of tangential relaxation: `mesh_smooth`'s umbrella step with the part along the vertex normal taken out, so that
    vertices slide along the surface and do not shrink it.  verts (V,3) float32, faces (F,3) integer ids, normal_sum (V,3) float64
    of `vertex_normals` of the same mesh, lamb in (0, 1] (its float32 value is the factor), adjacency `mesh_adjacency` or None.
    A vertex moves when it is finite, has neither bit 0 nor bit 1 of vert_flags (is not on a boundary or non-manifold edge), has a
    finite neighbour, and nn = (N0 N0 + N1 N1) + N2 N2 of its normal_sum N is finite and > 0.  s = the float64 sum of its finite
    unique neighbours in ascending id, m their number, d = s / m - p, t = ((d0 N0 + d1 N1) + d2 N2) / nn, new = float32(p + lamb
    (d - t N)), every operation rounded on its own; no square root.  All other vertices are copied bit for bit.  -> verts_out
    (V,3) float32.  The specification of arah_mesh_tangential (csrc/meshadj.hpp), and what runs for meshes on the host."""
    what = "mesh_tangential_step"
    f = check_tangential_lamb(lamb, what)
    verts, faces, V, _ = _mesh_verts(verts, faces, what)
    f64 = torch.float64
    if not isinstance(normal_sum, torch.Tensor) or tuple(normal_sum.shape) != (V, 3) or normal_sum.dtype != f64 \
            or normal_sum.device != verts.device:
        raise ValueError("%s: normal_sum must be the (V, 3) float64 sum of vertex_normals, on %s" % (what, verts.device))
    adjacency = _adjacency_of(faces, V, adjacency, what)
    nbr_start, nbr, flags = adjacency[2], adjacency[3], adjacency[6]
    F = int(faces.shape[0])
    if V == 0 or F == 0:
        return verts.clone()
    start = nbr_start.long()
    first, deg = start[:-1], start[1:] - start[:-1]
    nb, p, finite = nbr.long(), verts.to(f64), torch.isfinite(verts).all(1)
    s = torch.zeros(V, 3, dtype=f64, device=verts.device)
    m = torch.zeros(V, dtype=f64, device=verts.device)
    for k in range(int(deg.max())):
        n = nb[(first + k).clamp(max=6 * F - 1)]
        has = (k < deg) & finite[n]
        s = s + torch.where(has[:, None], p[n], torch.zeros_like(s))
        m = m + has.to(f64)
    N = normal_sum
    nn = (N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2]
    moves = finite & ((flags & 3) == 0) & (m > 0) & torch.isfinite(nn) & (nn > 0)
    d = s / m.clamp_min(1.0)[:, None] - p
    t = ((d[:, 0] * N[:, 0] + d[:, 1] * N[:, 1]) + d[:, 2] * N[:, 2]) / nn
    new = (p + f * (d - t[:, None] * N)).float()
    return torch.where(moves[:, None], new, verts)


# ---- the cotangent Laplacian, curvatures, cotangent smoothing ------------------------------------------------------------------------
TWO_PI = 6.283185307179586             # the doubles nearest to 2 pi and pi: kMlTwoPi, kMlPi
PI = 3.141592653589793
COTANGENT_MASSES = ("barycentric", "mixed")                                      # the kernel's mass 0, 1
COTANGENT_COUNTS = ("faces", "degenerate", "nonfinite", "obtuse", "negative_edges", "bad_area")   # counts[0 .. 5] of 8
CURVATURE_FIELDS = ("mean", "mean_abs", "gaussian", "k1", "k2")                  # the columns of mesh_curvature's first output
LAPLACIAN_MAX_CHANNELS = 32


def check_mass(mass, what="mesh_cotangent"):
    if not isinstance(mass, str) or mass not in COTANGENT_MASSES:
        raise ValueError("%s: mass must be 'barycentric' or 'mixed', got %r" % (what, mass))
    return COTANGENT_MASSES.index(mass)


def _sqrt64(x):
    """The correctly rounded square root: `_sqrt_rn` on the host, the device's own sqrt on a device."""
    return torch.sqrt(x) if x.is_cuda else _sqrt_rn(x).to(x.device)


def _dot3r(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _first_true3(m):
    """The first column of the (N,3) mask that is set, -1 when none."""
    full = torch.full(m.shape[:1], -1, dtype=torch.int64, device=m.device)
    return torch.where(m[:, 0], full + 1, torch.where(m[:, 1], full + 2, torch.where(m[:, 2], full + 3, full)))


def _cotangent_faces(verts, faces, valid, mass):
    """Per face (F,...): contributing, degenerate, nonfinite, obtuse masks; cot, angle, share (F,3), all 0 where the face does not
    contribute."""
    f64, V = torch.float64, int(verts.shape[0])
    p = verts.to(f64)[faces.clamp(0, max(V - 1, 0))]                             # (F,3,3); rows of skipped faces are never used
    finite = torch.isfinite(p).all(2).all(1)
    N = _cross3(p)
    A2 = _sqrt64(_dot3r(N, N))
    area_ok = torch.isfinite(A2) & (A2 > 0)
    contributing = valid & finite & area_ok
    dot, l2 = [], []
    for c in range(3):
        a, b = (c + 1) % 3, (c + 2) % 3
        u, w, e = p[:, a] - p[:, c], p[:, b] - p[:, c], p[:, b] - p[:, a]
        dot.append(_dot3r(u, w))
        l2.append(_dot3r(e, e))
    dot, l2 = torch.stack(dot, 1), torch.stack(l2, 1)
    safe = torch.where(contributing, A2, torch.ones_like(A2))[:, None]
    cot = dot / safe
    angle = torch.atan2(safe.expand_as(dot), dot)
    first_obtuse = _first_true3(dot < 0)
    if mass == 0:
        share = safe.expand_as(dot)
    else:
        vor = torch.stack([(l2[:, (c + 1) % 3] * cot[:, (c + 1) % 3] + l2[:, (c + 2) % 3] * cot[:, (c + 2) % 3]) * 0.125
                           for c in range(3)], 1)
        corner = torch.arange(3, device=verts.device)[None, :]
        share = torch.where((first_obtuse < 0)[:, None], vor, torch.where(first_obtuse[:, None] == corner, safe * 0.25, safe * 0.125))
    zero = torch.zeros_like(dot)
    c3 = contributing[:, None]
    return (contributing, valid & finite & ~area_ok, valid & ~finite, contributing & (first_obtuse >= 0),
            torch.where(c3, cot, zero), torch.where(c3, angle, zero), torch.where(c3, share, zero))


def mesh_cotangent(verts, faces, mass="mixed", adjacency=None):
    """The cotangent Laplacian of an indexed mesh with its lumped mass: verts (V,3) float32, faces (F,3) integer ids, mass
    "barycentric" or "mixed", adjacency `mesh_adjacency` of the mesh or None.  Float64 from the float32 inputs, every operation
    rounded on its own, square roots correctly rounded; atan2 is the only function that is not.

    PER VALID FACE (ids in range and pairwise different) with corners p0, p1, p2 widened to float64.  The face is NONFINITE when a
    coordinate is not finite.  Otherwise N = (p1 - p0) x (p2 - p0), each component (x y) - (z w) as in `vertex_normals`, nn = (N0
    N0 + N1 N1) + N2 N2, A2 = sqrt(nn) (the doubled area), and the face is DEGENERATE when A2 is 0 or not finite.  Nonfinite and
    degenerate faces contribute nothing anywhere.  For corner c of a contributing face, with a = c + 1 and b = c + 2 (mod 3): u =
    p_a - p_c, w = p_b - p_c, e = p_b - p_a; dot_c = (u0 w0 + u1 w1) + u2 w2; cot_c = dot_c / A2; angle_c = atan2(A2, dot_c); l2_c
    = (e0 e0 + e1 e1) + e2 e2, the squared length of the opposite edge.

    PER NEIGHBOUR ENTRY (v, n) of the adjacency's nbr: weight = 0.5 acc, where acc starts at 0 and takes acc = acc + cot_o for every
    contributing face that holds v and n, o its third corner, in ASCENDING FACE ID (the order of vf[v]).  A boundary edge has one
    term, a non-manifold edge as many as it has faces.  The sum does not depend on the end it is seen from, so (v, n) and (n, v)
    carry the same bits.  Nothing is clamped.

    PER VERTEX v: diag = the sum of its entries' weights in ascending neighbour id, from 0.  angle_sum = the sum of angle_c, c the
    corner of v, over its contributing faces in ascending face id, from 0.  area, by the same loop over the faces: "barycentric":
    (the sum of A2) / 6.  "mixed" (Meyer, Desbrun, Schroeder, Barr 2002): the sum of the faces' shares; with o the FIRST corner of
    the face (0, 1, 2) with dot_o < 0: none -- the Voronoi share (l2_a cot_a + l2_b cot_b) 0.125; o = c -- A2 0.25; otherwise A2
    0.125.  Both partition the area of the contributing faces.

    -> weight (6F,) float64 aligned with nbr (rows from nbr_start[V] on are zero), diag, area, angle_sum (V,) float64, counts (8,)
    int32: COTANGENT_COUNTS -- contributing, degenerate, nonfinite faces; contributing faces with a corner dot < 0; entries with n >
    v and weight < 0; vertices whose area is not > 0 -- and two zeros.  The ordered sums are loops over k < the widest segment of a
    padded gather (adding 0.0 for the padding is exact, and a sum that starts at +0 never becomes -0).  The specification of
    arah_mesh_cotangent (csrc/meshlaplace.hpp), and what runs for meshes on the host."""
    m = check_mass(mass)
    verts, faces, V, in_range = _mesh_verts(verts, faces, "mesh_cotangent")
    adjacency = _adjacency_of(faces, V, adjacency, "mesh_cotangent")
    vf_start, vf, nbr_start, nbr = adjacency[:4]
    dev, f64, F = verts.device, torch.float64, int(faces.shape[0])
    weight = torch.zeros(6 * F, dtype=f64, device=dev)
    diag, area, angle_sum = (torch.zeros(V, dtype=f64, device=dev) for _ in range(3))
    if V == 0 or F == 0:
        return weight, diag, area, angle_sum, torch.tensor([0, 0, 0, 0, 0, V, 0, 0], dtype=torch.int32, device=dev)
    valid = in_range & (faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])
    contributing, degenerate, nonfinite, obtuse, cot, angle, share = _cotangent_faces(verts, faces, valid, m)
    ids = torch.arange(V, device=dev)
    fstart, vfl = vf_start.long(), vf.long()
    ffirst, fdeg = fstart[:-1], fstart[1:] - fstart[:-1]
    zero = torch.zeros(V, dtype=f64, device=dev)
    for k in range(int(fdeg.max())):
        has = k < fdeg
        f = vfl[(ffirst + k).clamp(max=3 * F - 1)]
        c = _first_true3(faces[f] == ids[:, None]).clamp(min=0)
        angle_sum = angle_sum + torch.where(has, angle[f, c], zero)
        area = area + torch.where(has, share[f, c], zero)
    if m == 0:
        area = area / 6.0
    nstart, nb = nbr_start.long(), nbr.long()
    nfirst, ndeg = nstart[:-1], nstart[1:] - nstart[:-1]
    E = int(nstart[-1])
    ev, en = torch.repeat_interleave(ids, ndeg), nb[:E]
    acc = torch.zeros(E, dtype=f64, device=dev)
    for k in range(int(fdeg.max())):
        f = vfl[(ffirst[ev] + k).clamp(max=3 * F - 1)]
        cv, cn = _first_true3(faces[f] == ev[:, None]), _first_true3(faces[f] == en[:, None])
        hit = (k < fdeg[ev]) & (cv >= 0) & (cn >= 0)
        acc = acc + torch.where(hit, cot[f, (3 - cv - cn).clamp(0, 2)], torch.zeros_like(acc))
    weight[:E] = 0.5 * acc
    for k in range(int(ndeg.max())):
        diag = diag + torch.where(k < ndeg, weight[(nfirst + k).clamp(max=6 * F - 1)], zero)
    counts = torch.tensor([int(contributing.sum()), int(degenerate.sum()), int(nonfinite.sum()), int(obtuse.sum()),
                           int(((en > ev) & (weight[:E] < 0)).sum()), int((~(area > 0)).sum()), 0, 0], dtype=torch.int32, device=dev)
    return weight, diag, area, angle_sum, counts


def _laplacian_x(x, V, dev, what):
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or int(x.shape[0]) != V or x.dtype not in (torch.float32, torch.float64) \
            or not 1 <= int(x.shape[1]) <= LAPLACIAN_MAX_CHANNELS or x.device != dev:
        raise ValueError("%s: x must be a (V, C) float32 or float64 tensor with 1 <= C <= %d, on %s" % (what, LAPLACIAN_MAX_CHANNELS, dev))
    return x.detach()


def _laplacian_weight(weight, adjacency, what):
    """weight (6F,) float64 beside the eight arrays of `mesh_adjacency` -> (weight, nbr_start, nbr, V)."""
    adjacency = tuple(adjacency) if adjacency is not None else ()
    if len(adjacency) != 8 or any(not isinstance(t, torch.Tensor) for t in adjacency):
        raise ValueError("%s: adjacency must be the eight arrays of mesh_adjacency" % what)
    nbr_start, nbr = adjacency[2], adjacency[3]
    if not isinstance(weight, torch.Tensor) or weight.dtype != torch.float64 or weight.shape != nbr.shape or weight.device != nbr.device:
        raise ValueError("%s: weight must be the (6F,) float64 weights of mesh_cotangent, beside nbr" % what)
    return weight.detach(), nbr_start, nbr, int(nbr_start.shape[0]) - 1


def laplacian_apply(weight, adjacency, x):
    """y = L x for the weights of `mesh_cotangent`: x (V,C) float32 or float64, 1 <= C <= 32.  y[v] = the sum over v's neighbour
    entries in ascending neighbour id, from 0, of weight(v, n) (x[n] - x[v]) in float64, every operation rounded on its own, column
    by column; an entry whose weight or whose x[n] (in that column) is not finite is skipped, and where x[v] itself is not finite y
    is NaN (the quiet NaN with no payload: the bits of an arithmetic NaN differ between machines).  -> y (V,C) float64.  (L is negative
    semi-definite: diag is the sum of the weights, the matrix has -diag on its diagonal.)  The specification of
    arah_mesh_laplacian_apply (csrc/meshlaplace.hpp), and what runs for meshes on the host."""
    weight, nbr_start, nbr, V = _laplacian_weight(weight, adjacency, "laplacian_apply")
    x = _laplacian_x(x, V, weight.device, "laplacian_apply")
    xd = x.to(torch.float64)
    y = torch.zeros_like(xd)
    rows = int(nbr.shape[0])
    if V == 0 or rows == 0:
        return y
    start, nb = nbr_start.long(), nbr.long()
    first, deg = start[:-1], start[1:] - start[:-1]
    for k in range(int(deg.max())):
        i = (first + k).clamp(max=rows - 1)
        n, w = nb[i], weight[i]
        ok = ((k < deg) & torch.isfinite(w))[:, None] & torch.isfinite(xd[n])
        y = y + torch.where(ok, w[:, None] * (xd[n] - xd), torch.zeros_like(y))
    return torch.where(torch.isfinite(xd), y, torch.full_like(y, float("nan")))


def mesh_curvature(verts, faces, mass="mixed", adjacency=None, laplacian=None, normal_sum=None):
    """Mean, Gaussian and principal curvatures at the vertices of an indexed mesh (Meyer, Desbrun, Schroeder, Barr 2002): verts
    (V,3) float32, faces (F,3) integer ids, mass as in `mesh_cotangent`, adjacency `mesh_adjacency` or None, laplacian the five
    outputs of `mesh_cotangent` of the mesh or None, normal_sum (V,3) float64 of `vertex_normals` or None.

    L = `laplacian_apply`(weight, verts); K = (-L) / area, Meyer's mean-curvature normal 2 kappa_H n.  N = normal_sum, len =
    sqrt((N0 N0 + N1 N1) + N2 N2).
        mean_normal = 0.5 K              mean_abs = 0.5 sqrt((K0 K0 + K1 K1) + K2 K2)
        mean = 0.5 (((K0 N0 + K1 N1) + K2 N2) / len)
        gaussian = (TWO_PI - angle_sum) / area, (PI - angle_sum) / area for a vertex with vert_flags bit 0 (on a boundary)
        r = sqrt(max(mean mean - gaussian, 0)), k1 = mean + r, k2 = mean - r
    TWO_PI and PI are the nearest doubles.  The sign of mean follows the mesh's own orientation, whatever it is: with counter-
    clockwise faces seen from outside a convex part has mean > 0.  THE PROJECT'S OWN LEVEL SETS (marching cubes of a signed
    distance) ARE ORIENTED CLOCKWISE SEEN FROM OUTSIDE, so a convex part of a body has mean < 0 there; mean_abs and gaussian do not
    depend on the orientation.  A vertex is INVALID when it has vert_flags bit 1 (non-manifold) or bit 2 (isolated), a non-finite
    coordinate, an area that is not finite and > 0, or a len that is not finite and > 0: NaN in every output, valid = 0.

    -> curv (V,5) float64 with the columns CURVATURE_FIELDS, mean_normal (V,3) float64, valid (V,) uint8, counts (1,) int32 the
    invalid vertices.  The specification of arah_mesh_curvature (csrc/meshlaplace.hpp), bit for bit given the same angle_sum."""
    what = "mesh_curvature"
    check_mass(mass, what)
    verts, faces, V, _ = _mesh_verts(verts, faces, what)
    adjacency = _adjacency_of(faces, V, adjacency, what)
    if laplacian is None:
        laplacian = mesh_cotangent(verts, faces, mass, adjacency)
    weight, _, area, angle_sum = tuple(laplacian)[:4]
    if normal_sum is None:
        normal_sum = vertex_normals(verts, faces, adjacency)[0]
    f64, dev = torch.float64, verts.device
    for t, shape in ((area, (V,)), (angle_sum, (V,)), (normal_sum, (V, 3))):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != f64 or t.device != dev:
            raise ValueError("%s: laplacian must be the outputs of mesh_cotangent, normal_sum of vertex_normals, on %s" % (what, dev))
    flags = adjacency[6].long()
    L = laplacian_apply(weight, adjacency, verts)
    N = normal_sum
    length = _sqrt64(_dot3r(N, N))
    valid = ((flags & 6) == 0) & torch.isfinite(verts).all(1) & torch.isfinite(area) & (area > 0) & torch.isfinite(length) & (length > 0)
    a = torch.where(valid, area, torch.ones_like(area))
    K = (-L) / a[:, None]
    mean = 0.5 * (_dot3r(K, N) / torch.where(valid, length, torch.ones_like(length)))
    pi = torch.where((flags & 1) != 0, torch.full_like(a, PI), torch.full_like(a, TWO_PI))
    gauss = (pi - angle_sum) / a
    disc = mean * mean - gauss
    root = _sqrt64(torch.where(disc > 0, disc, torch.zeros_like(disc)))
    curv = torch.stack([mean, 0.5 * _sqrt64(_dot3r(K, K)), gauss, mean + root, mean - root], 1)
    nan = torch.full_like(curv[:, :1], float("nan"))
    curv = torch.where(valid[:, None], curv, nan)
    mean_normal = torch.where(valid[:, None], 0.5 * K, nan)
    return curv, mean_normal, valid.to(torch.uint8), torch.tensor([V - int(valid.sum())], dtype=torch.int32, device=dev)


def _mesh_smooth_cotangent(verts, faces, V, iterations, factors, pin, adjacency):
    """The steps of `mesh_smooth` with weights="cotangent"."""
    nbr_start, nbr, flags = adjacency[2], adjacency[3], adjacency[6]
    cur, F, dev, f64 = verts.clone(), int(faces.shape[0]), verts.device, torch.float64
    if V == 0 or F == 0 or iterations == 0:
        return cur
    start, nb = nbr_start.long(), nbr.long()
    first, deg = start[:-1], start[1:] - start[:-1]
    width = int(deg.max())
    free = (flags & 3) == 0 if pin else torch.ones(V, dtype=torch.bool, device=dev)
    for step in range(iterations * len(factors)):
        f = factors[step % len(factors)]
        weight = mesh_cotangent(cur, faces, "mixed", adjacency)[0]
        p, finite = cur.to(f64), torch.isfinite(cur).all(1)
        acc = torch.zeros(V, 3, dtype=f64, device=dev)
        s = torch.zeros(V, dtype=f64, device=dev)
        for k in range(width):
            i = (first + k).clamp(max=6 * F - 1)
            n, w = nb[i], weight[i]
            has = (k < deg) & finite[n] & torch.isfinite(w)
            s = s + torch.where(has, w.abs(), torch.zeros_like(s))
            acc = acc + torch.where(has[:, None], w[:, None] * (p[n] - p), torch.zeros_like(acc))
        moves = finite & free & torch.isfinite(s) & (s > 0)
        new = (p + f * (acc / torch.where(moves, s, torch.ones_like(s))[:, None])).float()
        cur = torch.where(moves[:, None], new, cur)
    return cur


# ---- systems with the cotangent operator: preconditioned conjugate gradients -------------------------------------------------------
SOLVE_MAX_VERTS = 1 << 24               # kMsMaxVerts: blocks of 256, then at most 256 chunks of 256 blocks' sums
SOLVE_COUNTS = ("solved", "pinned", "not_live", "bad_rhs", "bad_area", "bad_diagonal")   # counts[0 .. 5] of 8; a vertex's class
SOLVE_STATUS = ("max_iter", "converged", "breakdown")                            # a column's status 0, 1, 2


def check_solve_args(mass_coef, stiff_coef, tol, max_iter, what="laplacian_solve"):
    """The scalars of `laplacian_solve`, checked: -> (mass_coef, stiff_coef, tol) as Python floats and max_iter as an int."""
    for name, x in (("mass_coef", mass_coef), ("stiff_coef", stiff_coef), ("tol", tol)):
        if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or not math.isfinite(float(x)):
            raise ValueError("%s: %s must be a finite number, got %r" % (what, name, x))
    if float(mass_coef) < 0.0:
        raise ValueError("%s: mass_coef must be >= 0, got %r" % (what, mass_coef))
    if not float(stiff_coef) > 0.0:
        raise ValueError("%s: stiff_coef must be > 0, got %r" % (what, stiff_coef))
    if float(tol) < 0.0:
        raise ValueError("%s: tol must be >= 0, got %r" % (what, tol))
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or int(max_iter) < 0:
        raise ValueError("%s: max_iter must be an integer >= 0, got %r" % (what, max_iter))
    return float(mass_coef), float(stiff_coef), float(tol), int(max_iter)


def check_solve_size(n_verts, what="laplacian_solve"):
    if n_verts > SOLVE_MAX_VERTS:
        raise ValueError("%s: at most 2^24 vertices (the inner product's tree has three levels of 256), got %d" % (what, n_verts))


def check_solve_tensors(area, rhs, x0, pinned, V, dev, what="laplacian_solve"):
    """area (V,), rhs and x0 (V,C) float64 with 1 <= C <= 32, pinned (V,) bool or None, all on dev: -> C."""
    check_solve_size(V, what)
    f64 = torch.float64
    if not isinstance(area, torch.Tensor) or tuple(area.shape) != (V,) or area.dtype != f64 or area.device != dev:
        raise ValueError("%s: area must be the (V,) float64 area of mesh_cotangent, on %s" % (what, dev))
    for name, t in (("rhs", rhs), ("x0", x0)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or int(t.shape[0]) != V or t.dtype != f64 or t.device != dev \
                or not 1 <= int(t.shape[1]) <= LAPLACIAN_MAX_CHANNELS:
            raise ValueError("%s: %s must be a (V, C) float64 tensor with 1 <= C <= %d, on %s" % (what, name, LAPLACIAN_MAX_CHANNELS, dev))
    if rhs.shape != x0.shape:
        raise ValueError("%s: rhs is %s, x0 is %s" % (what, tuple(rhs.shape), tuple(x0.shape)))
    if pinned is not None and (not isinstance(pinned, torch.Tensor) or tuple(pinned.shape) != (V,) or pinned.dtype != torch.bool
                               or pinned.device != dev):
        raise ValueError("%s: pinned must be a (V,) bool tensor on %s, or None" % (what, dev))
    return int(rhs.shape[1])


def solve_dot(u, v):
    """<u, v> per column of (V,C) tensors: `quadric_tree_sum` over the V products u_i v_i taken as ONE segment, written as the
    pairs it consists of -- level by level x[2j] + x[2j + 1], an odd last element carried up unchanged.  The tree over aligned
    blocks of 256 followed by the same tree over the blocks' sums is this same tree, which is how the device takes it.  -> (C,);
    zeros for V = 0."""
    x = u * v
    if x.shape[0] == 0:
        return torch.zeros(x.shape[1], dtype=x.dtype, device=x.device)
    while x.shape[0] > 1:
        even = x.shape[0] & ~1
        s = x[0:even:2] + x[1:even:2]
        x = torch.cat([s, x[even:]]) if even < x.shape[0] else s
    return x[0]


def laplacian_solve(weight, area, adjacency, rhs, x0, pinned=None, mass_coef=0.0, stiff_coef=1.0, tol=1e-10, max_iter=10000):
    """Solve, for up to 32 independent columns, by Jacobi-preconditioned conjugate gradients in float64,

        mass_coef area_v x_v - stiff_coef sum_n w_vn (x_n - x_v) = rhs_v        at every SOLVED vertex v,

    with x = x0 at every other vertex.  weight (6F,) and area (V,) float64 of `mesh_cotangent`, adjacency `mesh_adjacency`; rhs and
    x0 (V,C) float64, 1 <= C <= 32; pinned (V,) bool or None; mass_coef >= 0, stiff_coef > 0, tol >= 0 finite Python floats;
    max_iter >= 0; V <= 2^24.  (mass_coef 0, stiff_coef 1 with pins: a Dirichlet problem, the harmonic extension; mass_coef 1,
    stiff_coef t, rhs = area p: an implicit smoothing step.)  The cotangent stiffness is positive semi-definite whatever the signs
    of its weights, so negative weights are allowed.  Every operation is float64 and rounded on its own.

    CLASSES.  live_v: the row x0[v] is finite in every column.  An entry (v, n) of nbr is USABLE when its weight is finite and
    live_n: decided once, from x0, never from an iterate.  dS_v = the sum of the usable weights of v in ascending neighbour id,
    from 0.  a_v = area_v, and +0 when mass_coef is 0 (the area is not looked at then).  d_v = mass_coef a_v + stiff_coef dS_v.
    The class of v is the first that applies: 1 pinned; 2 not live; 3 its rhs row is not finite; 4 mass_coef != 0 and area_v is not
    finite and > 0; 5 d_v is not finite and > 0; otherwise 0: SOLVED.  Everything else is HELD: a held vertex acts as a Dirichlet
    value where its x0 is finite and is left out of its neighbours' sums where it is not.

    OPERATOR.  On solved rows Op(y)_v = mass_coef (a_v y_v) - stiff_coef acc, acc = the sum over the usable entries in ascending
    neighbour id, from 0, of w (y_n - y_v); on held rows +0.  r, z, p, q are +0 on held rows throughout.

    INNER PRODUCT.  <u, v> = `solve_dot`: the tree of `quadric_tree_sum` over the V products as one segment; its shape depends on
    V alone.

    START, per column.  r = rhs - Op(x0) on solved rows; z = r / d; p = z; rz = <r, z>; rr = <r, r>; r0 = rr; thr = (tol tol) r0.
    A column whose r0 is not finite has status 2 (breakdown); otherwise one with rr <= thr has status 1 (converged) with 0
    iterations -- r0 = 0 is such a case.

    STEP, per column with status 0, at most max_iter times.  q = Op(p); pq = <p, q>.  If pq is not finite or not > 0: status 2, and
    the column stops unchanged.  alpha = rz / pq; x = x + alpha p; r = r - alpha q; z = r / d (solved rows only); rz' = <r, z>; rr =
    <r, r>; iters += 1.  If rr <= thr: status 1, and the column stops.  Otherwise beta = rz' / rz; p = z + beta p; rz = rz'.  A
    stopped column's arrays never change again; columns do not wait for each other; after max_iter steps the status stays 0.

    -> x (V,C) float64, iters (C,) int32, status (C,) int32 (SOLVE_STATUS), rr and r0 (C,) float64, counts (8,) int32 (SOLVE_COUNTS
    by class, and two zeros), classes (V,) uint8.  The specification of arah_mesh_solve_begin / arah_mesh_solve_steps
    (csrc/meshsolve.hpp), and what runs for meshes on the host."""
    what = "laplacian_solve"
    mc, sc, tol, max_iter = check_solve_args(mass_coef, stiff_coef, tol, max_iter, what)
    weight, nbr_start, nbr, V = _laplacian_weight(weight, adjacency, what)
    dev, f64, i32 = weight.device, torch.float64, torch.int32
    C = check_solve_tensors(area, rhs, x0, pinned, V, dev, what)
    rhs, x0 = rhs.detach(), x0.detach()
    rows = int(nbr.shape[0])
    live = torch.isfinite(x0).all(1)
    start = nbr_start.long()
    first, deg = start[:-1], (start[1:] - start[:-1]).clamp(min=0)
    width = int(deg.max()) if V and rows else 0
    k = torch.arange(width, device=dev)
    idx = (first[:, None] + k[None, :]).clamp(0, max(rows - 1, 0))                # (V, width): the padded rows of the entries
    n = nbr.long()[idx] if width else torch.zeros(V, 0, dtype=torch.int64, device=dev)
    in_range = (n >= 0) & (n < V)
    n = n.clamp(0, max(V - 1, 0))
    w = weight[idx] if width else torch.zeros(V, 0, dtype=f64, device=dev)
    usable = (k[None, :] < deg[:, None]) & in_range & torch.isfinite(w) & live[n]
    zero_v = torch.zeros(V, dtype=f64, device=dev)
    dS = zero_v.clone()
    for j in range(width):
        dS = dS + torch.where(usable[:, j], w[:, j], zero_v)
    a = area.detach() if mc != 0.0 else zero_v
    d = mc * a + sc * dS
    cls = torch.full((V,), 5, dtype=torch.int64, device=dev)
    cls[torch.isfinite(d) & (d > 0)] = 0
    if mc != 0.0:
        cls[~(torch.isfinite(a) & (a > 0))] = 4
    cls[~torch.isfinite(rhs).all(1)] = 3
    cls[~live] = 2
    if pinned is not None:
        cls[pinned] = 1
    solved = (cls == 0)[:, None]
    counts = torch.cat([torch.bincount(cls, minlength=6), torch.zeros(2, dtype=torch.int64, device=dev)]).to(i32)
    d1 = torch.where(solved[:, 0], d, torch.ones_like(d))[:, None]
    zero = torch.zeros(V, C, dtype=f64, device=dev)

    def op(y):
        acc = zero.clone()
        for j in range(width):
            acc = acc + torch.where(usable[:, j, None], w[:, j, None] * (y[n[:, j]] - y), zero)
        return torch.where(solved, mc * (a[:, None] * y) - sc * acc, zero)

    x = x0.clone()
    r = torch.where(solved, rhs - op(x0), zero)
    z = torch.where(solved, r / d1, zero)
    p = z.clone()
    rz, rr = solve_dot(r, z), solve_dot(r, r)
    r0 = rr.clone()
    thr = (tol * tol) * r0
    status = torch.where(~torch.isfinite(r0), 2, torch.where(rr <= thr, 1, 0)).to(i32)
    iters = torch.zeros(C, dtype=i32, device=dev)
    for _ in range(max_iter):
        run = status == 0
        if not bool(run.any()):
            break
        q = op(p)
        pq = solve_dot(p, q)
        broken = run & ~(torch.isfinite(pq) & (pq > 0))
        status[broken] = 2
        run = run & ~broken
        move = solved & run[None, :]
        alpha = rz / torch.where(run, pq, torch.ones_like(pq))
        x = torch.where(move, x + alpha * p, x)
        r = torch.where(move, r - alpha * q, r)
        z = torch.where(move, r / d1, z)
        rz_new, rr_new = solve_dot(r, z), solve_dot(r, r)
        rr = torch.where(run, rr_new, rr)
        iters = iters + run.to(i32)
        done = run & (rr_new <= thr)
        status[done] = 1
        go = run & ~done
        beta = rz_new / torch.where(go, rz, torch.ones_like(rz))
        p = torch.where(solved & go[None, :], z + beta * p, p)
        rz = torch.where(go, rz_new, rz)
    return x, iters, status, rr, r0, counts, cls.to(torch.uint8)


def check_implicit_args(iterations, time, boundary, what="mesh_smooth_implicit"):
    """-> (time as a Python float, pin as a bool)."""
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or int(iterations) < 0:
        raise ValueError("%s: iterations must be an integer >= 0, got %r" % (what, iterations))
    if time is None or isinstance(time, bool) or not isinstance(time, (int, float, np.integer, np.floating)) \
            or not math.isfinite(float(time)) or not float(time) > 0.0:
        raise ValueError("%s: method='implicit' needs time, a finite length squared > 0, got %r" % (what, time))
    if boundary not in ("pin", "free"):
        raise ValueError("%s: boundary must be 'pin' or 'free', got %r" % (what, boundary))
    return float(time), boundary == "pin"


def mesh_smooth_implicit(verts, faces, iterations, time, boundary="pin", adjacency=None, tol=1e-10, max_iter=10000, backend=None):
    """Implicit fairing (Desbrun, Meyer, Schroeder, Barr 1999, "Implicit fairing of irregular meshes using diffusion and curvature
    flow"): every iteration takes weight and area = `mesh_cotangent`(cur, faces, "mixed") of the positions it reads and solves
    (M + time S) p' = M p over the three coordinates with `laplacian_solve`: mass_coef 1, stiff_coef time, rhs = area p (float64,
    one rounding), x0 = p, pinned = the vertices with vert_flags bit 0 or 1 under boundary="pin", none under "free"; the solved
    vertices take float32(p'), rounded once, the held ones stay bit for bit.  time is a length squared, > 0: one step removes
    detail below about sqrt(time), whatever the mesh's resolution, where an explicit step is stable only for time below about an
    edge length squared.  A column that does not converge raises RuntimeError with its status and residual.  -> verts_out (V,3)
    float32.  backend: the module whose mesh_cotangent / laplacian_solve run (this one when None; hip for meshes on the GPU)."""
    what = "mesh_smooth_implicit"
    time, pin = check_implicit_args(iterations, time, boundary, what)
    _, _, tol, max_iter = check_solve_args(1.0, time, tol, max_iter, what)
    if backend is None:
        verts, faces, V, _ = _mesh_verts(verts, faces, what)
        adjacency = _adjacency_of(faces, V, adjacency, what)
        import sys
        backend = sys.modules[__name__]
    else:
        V = int(verts.shape[0])
    check_solve_size(V, what)
    cur = verts.clone()
    if V == 0 or int(faces.shape[0]) == 0 or int(iterations) == 0:
        return cur
    pinned = (adjacency[6] & 3) != 0 if pin else None
    for it in range(int(iterations)):
        weight, _, area, _, _ = backend.mesh_cotangent(cur, faces, "mixed", adjacency=adjacency)
        p = cur.to(torch.float64)
        x, iters, status, rr, r0, _, classes = backend.laplacian_solve(weight, area, adjacency, area[:, None] * p, p, pinned=pinned,
                                                                       mass_coef=1.0, stiff_coef=time, tol=tol, max_iter=max_iter)
        status = status.tolist()
        if any(s != 1 for s in status):
            res = torch.sqrt(rr / torch.where(r0 > 0, r0, torch.ones_like(r0))).tolist()
            raise RuntimeError("%s: iteration %d did not converge: status %s, residual %s after %s steps"
                               % (what, it, [SOLVE_STATUS[s] for s in status], res, iters.tolist()))
        cur = torch.where((classes == 0)[:, None], x.float(), cur)
    return cur


# ---- edge-collapse decimation: one round ---------------------------------------------------------------------------------------------
COLLAPSE_MAX_UNION = 32               # faces around an edge that is still a candidate: kMqShort, one lane's tree
COLLAPSE_COUNTS = ("n_verts", "n_faces", "selected", "applied", "candidates", "pinned", "link", "long_edges", "nonfinite", "over_error",
                   "flips", "fallbacks")
COLLAPSE_REASONS = ("candidate", "pinned", "link", "long_edges", "nonfinite", "over_error", "flips")   # counts[4 + reason]
COLLAPSE_BOUNDED_REASONS = COLLAPSE_REASONS + ("not_short", "too_long")   # reasons 7 and 8: counts[12], counts[13]
COLLAPSE_BOUNDED_COUNTS = COLLAPSE_COUNTS + ("not_short", "too_long")
COLLAPSE_NO_EDGE = 255                  # edge_reason of a neighbour entry that names no edge (nbr <= owner, or past the entries)
_COLLAPSE_EMPTY = 2 ** 63 - 1


def collapse_args(need, reg, max_cost, what="mesh_collapse_round"):
    """The scalars of `mesh_collapse_round`, checked: -> (need, reg as a float, max_cost as a float32 value)."""
    try:
        if isinstance(need, bool) or int(need) != need:
            raise TypeError
        need, reg, max_cost = int(need), float(reg), float(np.float32(float(max_cost)))
    except (TypeError, ValueError, OverflowError):
        raise ValueError("%s: need must be an integer, reg and max_cost numbers" % what)
    if not 0 <= need <= 2 ** 31 - 1:
        raise ValueError("%s: need must lie in [0, 2^31), got %r" % (what, need))
    if not math.isfinite(reg) or reg < 0.0:
        raise ValueError("%s: reg must be a finite number >= 0, got %r" % (what, reg))
    if math.isnan(max_cost) or max_cost < 0.0:
        raise ValueError("%s: max_cost must be a number >= 0 (inf: no bound), got %r" % (what, max_cost))
    return need, reg, max_cost


def _ragged(first, n):
    """Rows first[k] .. first[k] + n[k] of a flat array for every k: -> (k of every row, the rows), k ascending, rows ascending."""
    k = torch.repeat_interleave(torch.arange(n.shape[0], device=n.device), n)
    return k, first[k] + (torch.arange(k.shape[0], device=n.device) - (torch.cumsum(n, 0) - n)[k])


def _cross3(p):
    """(p1 - p0) x (p2 - p0) of corners p (P,3,3) float64, every component (x y) - (z w) as in `quadric_terms`."""
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    return torch.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                        e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)


def _d2_f32(p, q):
    d = p.to(torch.float64) - q.to(torch.float64)
    return ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).float()


def collapse_bounds(short_len2, long_len2, what="mesh_collapse_round"):
    """The two length bounds of `mesh_collapse_round`, checked: -> None without any, else (short_len2, long_len2) as floats >= 0,
    infinity for the one that is not given."""
    if short_len2 is None and long_len2 is None:
        return None
    out = []
    for name, x in (("short_len2", short_len2), ("long_len2", long_len2)):
        if x is None:
            x = float("inf")
        if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or not float(x) >= 0.0:
            raise ValueError("%s: %s must be a number >= 0 (inf: no bound), got %r" % (what, name, x))
        out.append(float(x))
    return tuple(out)


def mesh_collapse_round(verts, faces, need, reg=1e-3, max_cost=float("inf"), adjacency=None, details=False, short_len2=None,
                        long_len2=None):
    """One round of edge-collapse decimation: verts (V,3) float32, faces (F,3) integer ids, need >= 0 the most edges to collapse,
    reg the regulariser of `mesh_quadric_place`'s solve, max_cost a float32 bound on an edge's cost, adjacency `mesh_adjacency`
    of the mesh or None.  Many independent edges collapse at once; which ones is decided on integers and on the bits of rounded
    numbers, so the order in which a device's threads arrive does not show.  All floating point is float64 from the float32
    inputs, every operation rounded on its own; no square root.

    PINNED: a vertex with a non-finite coordinate, or without a neighbour, or with a neighbour entry that is not "one face each
    way" (nbr_out = nbr_in = 1).  The others are free.

    EDGES: the neighbour entry i = (u, v) with v > u names the edge {u, v}; i is its id.  The first test that fails is the edge's
    reason (COLLAPSE_REASONS) and is counted:
      1 pinned      u or v is pinned.
      2 link        the edge's two faces (the faces of vf[u] that name v, ascending) have the third vertices a and b; a = b, or
                    nbr[u] and nbr[v] have other than two ids in common (a and b always are), or a or b has fewer than four
                    neighbours.
      3 long_edges  n = |vf[u]| + |vf[v]| - 2, the faces that touch u or v each once, is above COLLAPSE_MAX_UNION = 32.
      4 nonfinite   m = (double(u) + double(v)) 0.5.  The ten numbers of every such face about m (`quadric_terms` and c = d d),
                    in ascending face id, are summed by `quadric_tree_sum`.  `quadric_solve` with reg and the bound max_a |u_a -
                    v_a| gives the offset y; a solve that is not good is counted (fallbacks) and y = 0.  pos = float32(m + y),
                    the midpoint's own float32 bits after a fall-back.  Ay_r = (A_r0 y0 + A_r1 y1) + A_r2 y2 for the rows r of the
                    symmetric A; raw = (((y0 Ay_0 + y1 Ay_1) + y2 Ay_2) + 2 ((b0 y0 + b1 y1) + b2 y2)) + c; cost32 = float32(raw),
                    +0 unless raw > 0.  The reason holds when float32(raw) is not finite.
      5 over_error  cost32 > max_cost.
      6 flips       for a face of the n that does not name both u and v: N = (p1 - p0) x (p2 - p0) of its corners, N' the same
                    with the corner that is u or v at double(pos); the reason holds unless (N0 N'0 + N1 N'1) + N2 N'2 > 0 for
                    every such face.
    An edge without a reason is a CANDIDATE with key = (bits(cost32) << 32) | i.

    BOUNDED (short_len2 or long_len2 given, the other one infinity; COLLAPSE_BOUNDED_REASONS): two more tests, for a remesher that
    removes short edges only and must not make long ones.
      7 not_short   BEFORE every other test: the edge's squared length (dx dx + dy dy) + dz dz in float64 is not below short_len2
                    (or is not a number).
      8 too_long    after test 6: a corner other than u and v of a face of the n that does not name both lies farther from pos
                    than long_len2 -- its squared distance to double(pos), formed the same way, exceeds long_len2.
    counts then has fourteen entries: the twelve of COLLAPSE_COUNTS, then the edges with reason 7 and with reason 8.  Without
    bounds nothing changes: twelve counts, the reasons 0 .. 6.

    SELECTION: m1[x] = the least key of the candidates at x; m2[x] = the least of m1 over x and its neighbours; a candidate is
    selected when m2[u] = m2[v] = its key.  Keys are unique, so a selected edge is the least at every vertex of N[u] and N[v]:
    no end of another selected edge is u, v or a neighbour of either, and the faces two selected edges touch are disjoint.  Of the
    selected edges the first `need` in ascending id are APPLIED.

    APPLY: v becomes u, u moves to pos; vert_src of u is v when float32(|double(v) - double(pos)|^2) is below u's, else u.  A
    valid face that names both ends of an applied edge goes; every other face stays in its order, its ids in [0, V) renamed (the
    others as they are; an id that does not fit int32 is -1).  The merged vertices go, the others keep their order.

    -> verts_out (V,3) float32, faces_out (F,3) int32, vert_src (V,) int32, face_src (F,) int32 (ids of THIS round's input),
    counts (12,) int32 in the order of COLLAPSE_COUNTS; rows past the counts are zero.  details: also edge_pos (6F,3) float32,
    edge_key (6F,) int64 (-1: no candidate) and edge_reason (6F,) uint8 (COLLAPSE_NO_EDGE where the entry names no edge, pos
    zero before reason 4), and selected (6F,) bool.  Plain tensor operations on the tensors' device: the specification of
    arah_mesh_collapse_round (csrc/meshcollapse.hpp), and what runs for meshes on the host."""
    what = "mesh_collapse_round"
    need, reg, max_cost = collapse_args(need, reg, max_cost, what)
    bounds = collapse_bounds(short_len2, long_len2, what)
    raw_faces = torch.as_tensor(faces)
    verts, faces, V, in_range = _mesh_verts(verts, faces, what)
    if raw_faces.dtype != torch.int32:
        faces = torch.where((faces >= 0) & (faces <= 2 ** 31 - 1), faces, torch.full_like(faces, -1))
    F, dev = int(faces.shape[0]), verts.device
    f64, i32, i64 = torch.float64, torch.int32, torch.int64
    adjacency = _adjacency_of(faces, V, adjacency, what)
    vf_start, vf, nbr_start, nbr, nbr_out, nbr_in = (t.long() for t in adjacency[:6])
    E = int(nbr_start[V])
    val, nvf = nbr_start[1:] - nbr_start[:-1], vf_start[1:] - vf_start[:-1]
    ids_v = torch.arange(V, device=dev)
    ev, en = torch.repeat_interleave(ids_v, val), nbr[:E]
    pinned = ~torch.isfinite(verts).all(1) | (val == 0)
    pinned[ev[(nbr_out[:E] != 1) | (nbr_in[:E] != 1)]] = True
    eid = torch.nonzero(en > ev)[:, 0]
    u, v = ev[eid], en[eid]
    n_edges = int(eid.shape[0])
    reason = torch.zeros(n_edges, dtype=i64, device=dev)
    pos = torch.zeros(n_edges, 3, dtype=torch.float32, device=dev)
    cost_bits = torch.zeros(n_edges, dtype=i64, device=dev)
    fallbacks = 0
    reason[pinned[u] | pinned[v]] = 1
    if bounds is not None:
        reason[~(_d2_f64(verts[u].to(f64), verts[v].to(f64)) < bounds[0])] = 7
    # 2: the link condition
    at = torch.nonzero(reason == 0)[:, 0]
    if at.numel():
        ub, vb = u[at], v[at]
        k, rows = _ragged(vf_start[ub], nvf[ub])
        fcs = vf[rows]
        shared = (faces[fcs] == vb[k][:, None]).any(1)
        third = faces[fcs[shared]].sum(1) - ub[k[shared]] - vb[k[shared]]          # two per edge: nbr_out = nbr_in = 1
        a, b = third[0::2], third[1::2]
        k, rows = _ragged(nbr_start[ub], val[ub])
        ekey = ev * max(V, 1) + en                                                  # ascending: the entries' own order
        want = vb[k] * max(V, 1) + nbr[rows]
        found = ekey[torch.searchsorted(ekey, want).clamp(max=E - 1)] == want
        common = torch.zeros(at.shape[0], dtype=i64, device=dev).index_add_(0, k, found.long())
        reason[at[(a == b) | (common != 2) | (val[a] < 4) | (val[b] < 4)]] = 2
    # 3: the faces around the edge
    n_union = nvf[u] + nvf[v] - 2
    reason[(reason == 0) & (n_union > COLLAPSE_MAX_UNION)] = 3
    # 4 .. 6: position, cost, flips
    at = torch.nonzero(reason == 0)[:, 0]
    if at.numel():
        ub, vb, K = u[at], v[at], int(at.shape[0])
        ku, ru = _ragged(vf_start[ub], nvf[ub])
        kv, rv = _ragged(vf_start[vb], nvf[vb])
        pair = torch.unique(torch.cat([ku * max(F, 1) + vf[ru], kv * max(F, 1) + vf[rv]]), sorted=True)
        pk, pf = pair // max(F, 1), pair % max(F, 1)
        n = torch.bincount(pk, minlength=K)
        pu, pv = verts[ub].to(f64), verts[vb].to(f64)
        m = (pu + pv) * 0.5
        q = quadric_tree_sum(quadric_terms(verts, faces[pf], m[pk], with_c=True), torch.cumsum(n, 0) - n, n)
        y, good = quadric_solve(q, reg, (pu - pv).abs().amax(1))
        fallbacks = int((~good).sum())
        y = torch.where(good[:, None], y, torch.zeros_like(y))
        p_new = torch.where(good[:, None], (m + y).float(), m.float())
        A00, A01, A02, A11, A12, A22, b0, b1, b2, c = (q[:, j] for j in range(10))
        y0, y1, y2 = y[:, 0], y[:, 1], y[:, 2]
        Ay0 = (A00 * y0 + A01 * y1) + A02 * y2
        Ay1 = (A01 * y0 + A11 * y1) + A12 * y2
        Ay2 = (A02 * y0 + A12 * y1) + A22 * y2
        raw = (((y0 * Ay0 + y1 * Ay1) + y2 * Ay2) + 2.0 * ((b0 * y0 + b1 * y1) + b2 * y2)) + c
        finite = torch.isfinite(raw.float())
        cost32 = torch.where(raw > 0, raw.float(), torch.zeros_like(raw, dtype=torch.float32))
        ids = faces[pf]
        moves = (ids == ub[pk][:, None]) | (ids == vb[pk][:, None])
        before = verts[ids].to(f64)
        after = torch.where(moves[:, :, None], p_new[pk].to(f64)[:, None, :], before)
        N, N2 = _cross3(before), _cross3(after)
        dot = (N[:, 0] * N2[:, 0] + N[:, 1] * N2[:, 1]) + N[:, 2] * N2[:, 2]
        flipped = torch.zeros(K, dtype=torch.bool, device=dev)
        flipped[pk[(moves.sum(1) == 1) & ~(dot > 0)]] = True
        far = torch.zeros(K, dtype=torch.bool, device=dev)
        if bounds is not None:
            gap = before - p_new[pk].to(f64)[:, None, :]
            gap2 = (gap[:, :, 0] * gap[:, :, 0] + gap[:, :, 1] * gap[:, :, 1]) + gap[:, :, 2] * gap[:, :, 2]
            far[pk[(moves.sum(1) == 1) & (~moves & (gap2 > bounds[1])).any(1)]] = True
        over = cost32 > max_cost
        reason[at] = torch.where(~finite, 4, torch.where(over, 5, torch.where(flipped, 6, torch.where(far, 8, 0)))).to(i64)
        pos[at] = p_new
        cost_bits[at] = cost32.view(i32).long()
    cand = reason == 0
    key = torch.where(cand, (cost_bits << 32) | eid, torch.full_like(eid, _COLLAPSE_EMPTY))
    # selection
    m1 = torch.full((V,), _COLLAPSE_EMPTY, dtype=i64, device=dev)
    m1 = m1.scatter_reduce(0, torch.cat([u, v]), torch.cat([key, key]), "amin")
    m2 = m1.scatter_reduce(0, ev, m1[en], "amin")
    selected = cand & (m2[u] == key) & (m2[v] == key)
    n_selected = int(selected.sum())
    applied = torch.nonzero(selected)[:need, 0]
    # apply
    ua, va, pa = u[applied], v[applied], pos[applied]
    merge_to = ids_v.clone()
    merge_to[va] = ua
    moved = verts.clone()
    moved[ua] = pa
    src = ids_v.clone()
    src[ua] = torch.where(_d2_f32(verts[va], pa) < _d2_f32(verts[ua], pa), va, ua)
    keep = merge_to == ids_v
    new_id = torch.cumsum(keep.long(), 0) - 1
    nv = int(keep.sum())
    verts_out = torch.zeros(V, 3, dtype=torch.float32, device=dev)
    vert_src = torch.zeros(V, dtype=i64, device=dev)
    verts_out[:nv], vert_src[:nv] = moved[keep], src[keep]
    named = (faces >= 0) & (faces < V)
    renamed = torch.where(named, new_id[merge_to[faces.clamp(0, max(V - 1, 0))]] if V else faces, faces)
    valid = in_range & (faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])
    gone = valid & ((renamed[:, 0] == renamed[:, 1]) | (renamed[:, 1] == renamed[:, 2]) | (renamed[:, 0] == renamed[:, 2]))
    rows = torch.nonzero(~gone)[:, 0]
    nf = int(rows.shape[0])
    faces_out = torch.zeros(F, 3, dtype=i64, device=dev)
    face_src = torch.zeros(F, dtype=i64, device=dev)
    faces_out[:nf], face_src[:nf] = renamed[rows], rows
    counts = torch.tensor([nv, nf, n_selected, int(applied.shape[0])] + [int((reason == r).sum()) for r in range(7)]
                          + [fallbacks] + ([int((reason == r).sum()) for r in (7, 8)] if bounds is not None else []), dtype=i32,
                          device=dev)
    out = (verts_out, faces_out.to(i32), vert_src.to(i32), face_src.to(i32), counts)
    if not details:
        return out
    edge_pos = torch.zeros(6 * F, 3, dtype=torch.float32, device=dev)
    edge_key = torch.full((6 * F,), -1, dtype=i64, device=dev)
    edge_reason = torch.full((6 * F,), COLLAPSE_NO_EDGE, dtype=torch.uint8, device=dev)
    edge_sel = torch.zeros(6 * F, dtype=torch.bool, device=dev)
    edge_pos[eid], edge_reason[eid], edge_sel[eid] = pos, reason.to(torch.uint8), selected
    edge_key[eid] = torch.where(cand, key, torch.full_like(key, -1))
    return out + (edge_pos, edge_key, edge_reason, edge_sel)


# ---- subdivision: one round -----------------------------------------------------------------------------------------------------------
SUBDIVIDE_MAX_FACES = 1 << 26           # 4 F output faces and V + 3 F output vertices fit an int32
SUBDIVIDE_METHODS = {"midpoint": 0, "loop": 1}
SUBDIVIDE_COUNTS = ("n_verts", "n_faces", "edges", "marked", "faces_0", "faces_1", "faces_2", "faces_3", "invalid", "marked_nonfinite",
                    "interior", "rim", "kept")


def subdivide_args(method, max_len2, n_verts, n_faces, what="mesh_subdivide_round"):
    """The scalars of `mesh_subdivide_round`, checked: -> (the method's number, max_len2 as a float or None)."""
    if method not in SUBDIVIDE_METHODS:
        raise ValueError("%s: method must be 'midpoint' or 'loop', got %r" % (what, method))
    if max_len2 is not None:
        if isinstance(max_len2, bool) or not isinstance(max_len2, (int, float, np.integer, np.floating)):
            raise ValueError("%s: max_len2 must be a number or None, got %r" % (what, max_len2))
        max_len2 = float(max_len2)
        if math.isnan(max_len2) or max_len2 < 0.0:
            raise ValueError("%s: max_len2 must be a number >= 0 (inf: nothing is marked), got %r" % (what, max_len2))
        if method == "loop":
            raise ValueError("%s: method='loop' refines every edge: it takes no threshold" % what)
    if n_faces > SUBDIVIDE_MAX_FACES or n_verts + 3 * n_faces >= 2 ** 31:
        raise ValueError("%s: at most 2^26 faces and V + 3 F < 2^31, got V = %d, F = %d" % (what, n_verts, n_faces))
    return SUBDIVIDE_METHODS[method], max_len2


def _d2_f64(p, q):
    """(dx dx + dy dy) + dz dz of float32 points in float64, every operation rounded on its own."""
    d = p.to(torch.float64) - q.to(torch.float64)
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def mesh_subdivide_round(verts, faces, method="midpoint", max_len2=None, adjacency=None):
    """One round of subdivision of an indexed mesh: verts (V,3) float32, faces (F,3) integer ids (F <= 2^26, V + 3 F < 2^31; a face
    is valid as `mesh_adjacency` defines it), adjacency `mesh_adjacency` of the mesh or None.  Integers decide; all floating point
    is float64 from the float32 inputs, every operation rounded on its own, and reads the INPUT positions only.  A vertex is
    finite when its three coordinates are.

    EDGES AND MARKS: the neighbour entry (v, n) with n > v names the edge with the ends lo = v and hi = n, in ascending (v, n)
    order.  max_len2 = None: every edge is marked.  Otherwise (a Python float >= 0, midpoint only) an edge is marked when both ends
    are finite and d2 > max_len2, d2 = (dx dx + dy dy) + dz dz.  The k-th marked edge becomes vertex V + k; old vertices keep
    their ids.

    POSITIONS, "midpoint": old vertices are copied bit for bit; a new vertex is float32((lo + hi) 0.5); when an end is not finite
    (a uniform round only) it takes the bits of its lowest-id non-finite end, a copy without arithmetic.

    POSITIONS, "loop" (Warren's weights: no cosine).  An entry is REGULAR when nbr_out = nbr_in = 1.  A new vertex on a regular
    edge with finite lo, hi, c and d -- c the third corner of the face traversing lo->hi, d of the one traversing hi->lo -- is
    float32((lo + hi) 0.375 + (c + d) 0.125); every other new vertex takes the midpoint rule above.  An old vertex is INTERIOR
    when it is finite, has k >= 1 edges, all regular, and all its neighbours are finite: it moves to float32(p (1 - k beta) + s
    beta), s the sum of its neighbours in ascending id starting from 0, beta = 3/16 for k = 3 and 3.0 / (8.0 k) otherwise.  An
    old vertex is a RIM vertex when it is finite (a non-finite one is never put through arithmetic), exactly two of its edges
    have one face, every other edge is regular and the neighbours b0 < b1 across the two are finite: it moves to float32(p 0.75
    + (b0 + b1) 0.125).  Every other old vertex stays bit for bit.

    FACES: a valid face (a, b, c) with m marked edges becomes 1 + m faces in its orientation; x, y, z are the new vertices on ab,
    bc, ca.  m = 0: (a,b,c).  m = 3: (a,x,z), (x,b,y), (z,y,c), (x,y,z).  m = 1, rotated cyclically so that ab is marked:
    (a,x,c), (x,b,c).  m = 2, rotated so that ca is unmarked: (x,b,y), then (a,x,y), (a,y,c) when d2(a, y) < d2(x, c) on the
    OUTPUT float32 positions, else -- ties included -- (a,x,c), (x,y,c).  An invalid face is copied as one face (an id that does
    not fit int32 is -1).  Faces are ordered by input face, then by template.  Marks belong to edges: no T-junction.

    -> verts_out (V+3F,3) float32, faces_out (4F,3) int32, vert_src (V+3F,2) int32 ((v, v) or (lo, hi)), face_src (4F,) int32,
    counts (13,) int32 in the order of SUBDIVIDE_COUNTS; rows past the counts are zero.  Plain tensor operations on the tensors'
    device: the specification of arah_mesh_subdivide_round (csrc/meshsubdiv.hpp), and what runs for meshes on the host."""
    what = "mesh_subdivide_round"
    raw_faces = torch.as_tensor(faces)
    verts, faces, V, in_range = _mesh_verts(verts, faces, what)
    F, dev = int(faces.shape[0]), verts.device
    loop, max_len2 = subdivide_args(method, max_len2, V, F, what)
    if raw_faces.dtype != torch.int32:
        faces = torch.where((faces >= 0) & (faces <= 2 ** 31 - 1), faces, torch.full_like(faces, -1))
    f64, i32, i64 = torch.float64, torch.int32, torch.int64
    adjacency = _adjacency_of(faces, V, adjacency, what)
    nbr_start, nbr, nbr_out, nbr_in = (t.long() for t in adjacency[2:6])
    E = int(nbr_start[V])
    val = nbr_start[1:] - nbr_start[:-1]
    ids_v = torch.arange(V, device=dev)
    ev, en, n_out, n_in = torch.repeat_interleave(ids_v, val), nbr[:E], nbr_out[:E], nbr_in[:E]
    finite = torch.isfinite(verts).all(1)
    p64 = verts.to(f64)
    W = max(V, 1)
    ekey = ev * W + en                                                           # ascending: the entries' own order
    # marks and ranks
    is_edge = en > ev
    both = finite[ev] & finite[en]
    marked = is_edge & (both & (_d2_f64(verts[ev], verts[en]) > max_len2) if max_len2 is not None else torch.ones_like(is_edge))
    rank = torch.cumsum(marked.long(), 0) - 1
    me = torch.nonzero(marked)[:, 0]
    n_marked = int(me.shape[0])
    lo, hi = ev[me], en[me]
    # the entries of the faces' edges; Loop: the opposite corners by traversal direction
    valid = in_range & (faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])
    rows = torch.nonzero(valid)[:, 0]
    fv = faces[rows]
    fs, fd, ft = fv, fv[:, [1, 2, 0]], fv[:, [2, 0, 1]]                          # edge j: source, destination, third corner
    fent = torch.searchsorted(ekey, torch.minimum(fs, fd) * W + torch.maximum(fs, fd)) if rows.numel() else fs   # (Fv,3), all found
    # old vertices
    verts_out = torch.zeros(V + 3 * F, 3, dtype=torch.float32, device=dev)
    vert_src = torch.zeros(V + 3 * F, 2, dtype=i64, device=dev)
    moved = verts.clone()
    n_interior = n_rim = 0
    regular = (n_out == 1) & (n_in == 1)
    if loop and E:
        one = (n_out + n_in) == 1
        irregular = torch.zeros(V, dtype=i64, device=dev).index_add_(0, ev, (~regular).long())
        odd = torch.zeros(V, dtype=i64, device=dev).index_add_(0, ev, (~regular & ~one).long())
        n_one = torch.zeros(V, dtype=i64, device=dev).index_add_(0, ev, one.long())
        nonfin = torch.zeros(V, dtype=i64, device=dev).index_add_(0, ev, (~finite[en]).long())
        first = nbr_start[:-1]
        s = torch.zeros(V, 3, dtype=f64, device=dev)
        for k in range(int(val.max())):                                          # the ordered sum: a padded gather, + 0.0 is exact
            has = k < val
            n = nbr[(first + k).clamp(max=6 * F - 1)]
            s = s + torch.where(has[:, None], p64[n], torch.zeros_like(s))
        kf = val.to(f64)
        beta = torch.where(val == 3, torch.full_like(kf, 0.1875), 3.0 / (8.0 * kf.clamp_min(1.0)))
        keep = 1.0 - kf * beta
        interior = finite & (val > 0) & (irregular == 0) & (nonfin == 0)
        new_int = (p64 * keep[:, None] + s * beta[:, None]).float()
        # the rim neighbours: the one-face entries of a vertex in ascending order, the first and the second
        oe = torch.nonzero(one)[:, 0]
        b0, b1 = torch.zeros(V, dtype=i64, device=dev), torch.zeros(V, dtype=i64, device=dev)
        if oe.numel():
            ov = ev[oe]
            nth = torch.arange(oe.shape[0], device=dev) - (torch.cumsum(n_one, 0) - n_one)[ov]
            b0[ov[nth == 0]] = en[oe[nth == 0]]
            b1[ov[nth == 1]] = en[oe[nth == 1]]
        rim = finite & (n_one == 2) & (odd == 0) & finite[b0] & finite[b1]
        new_rim = (p64 * 0.75 + (p64[b0] + p64[b1]) * 0.125).float()
        moved = torch.where(interior[:, None], new_int, torch.where(rim[:, None], new_rim, verts))
        n_interior, n_rim = int(interior.sum()), int(rim.sum())
    verts_out[:V] = moved
    vert_src[:V] = ids_v[:, None]
    # new vertices
    n_nonfinite = 0
    if n_marked:
        plo, phi = p64[lo], p64[hi]
        new = ((plo + phi) * 0.5).float()
        if loop:
            opp = torch.zeros(E, 2, dtype=i64, device=dev)
            along = fs < fd
            opp[fent[along], 0] = ft[along]
            opp[fent[~along], 1] = ft[~along]
            c, d = opp[me, 0], opp[me, 1]
            stencil = regular[me] & finite[c] & finite[d]
            new = torch.where(stencil[:, None], ((plo + phi) * 0.375 + (p64[c] + p64[d]) * 0.125).float(), new)
        bad = ~both[me]
        n_nonfinite = int(bad.sum())
        copy = torch.where(finite[lo][:, None], verts[hi], verts[lo])
        verts_out[V:V + n_marked] = torch.where(bad[:, None], copy, new)
        vert_src[V:V + n_marked] = torch.stack([lo, hi], 1)
    # faces
    faces_out = torch.zeros(4 * F, 3, dtype=i64, device=dev)
    face_src = torch.zeros(4 * F, dtype=i64, device=dev)
    per = [0, 0, 0, 0]
    n_faces_out = 0
    if F:
        nv = torch.full((F, 3), -1, dtype=i64, device=dev)
        if rows.numel():
            nv[rows] = torch.where(marked[fent], V + rank[fent], torch.full_like(fent, -1))
        has = nv >= 0
        m = has.sum(1)
        per = [int((valid & (m == j)).sum()) for j in range(4)]
        # the rotation: one mark -> the marked edge first; two marks -> the unmarked edge last
        r = torch.zeros(F, dtype=i64, device=dev)
        r = torch.where(m == 1, torch.where(has[:, 0], 0, torch.where(has[:, 1], 1, 2)), r)
        r = torch.where(m == 2, torch.where(~has[:, 2], 0, torch.where(~has[:, 0], 1, 2)), r)
        turn = (r[:, None] + torch.arange(3, device=dev)[None, :]) % 3
        a, b, c = (torch.gather(faces, 1, turn)[:, j] for j in range(3))
        x, y, z = (torch.gather(nv, 1, turn)[:, j] for j in range(3))
        pos = verts_out
        safe = lambda t: t.clamp(0, V + 3 * F - 1)                               # rows of other templates are never used
        ay = (m == 2) & (_d2_f64(pos[safe(a)], pos[safe(y)]) < _d2_f64(pos[safe(x)], pos[safe(c)]))
        tpl = torch.zeros(F, 4, 3, dtype=i64, device=dev)
        tri = lambda *t: torch.stack(t, 1)
        tpl[:, 0] = tri(a, b, c)
        for sel, rows_t in (((m == 3), (tri(a, x, z), tri(x, b, y), tri(z, y, c), tri(x, y, z))),
                            ((m == 1), (tri(a, x, c), tri(x, b, c))),
                            ((m == 2) & ay, (tri(x, b, y), tri(a, x, y), tri(a, y, c))),
                            ((m == 2) & ~ay, (tri(x, b, y), tri(a, x, c), tri(x, y, c)))):
            for j, t in enumerate(rows_t):
                tpl[:, j] = torch.where(sel[:, None], t, tpl[:, j])
        n_of = 1 + m
        keep_row = torch.arange(4, device=dev)[None, :] < n_of[:, None]
        n_faces_out = int(n_of.sum())
        faces_out[:n_faces_out] = tpl[keep_row]
        face_src[:n_faces_out] = torch.arange(F, device=dev)[:, None].expand(F, 4)[keep_row]
    n_edges = int(is_edge.sum())
    counts = torch.tensor([V + n_marked, n_faces_out, n_edges, n_marked] + per + [F - int(valid.sum()), n_nonfinite, n_interior, n_rim,
                           V - n_interior - n_rim], dtype=i32, device=dev)
    return verts_out, faces_out.to(i32), vert_src.to(i32), face_src.to(i32), counts


# ---- edge flips: one round -----------------------------------------------------------------------------------------------------------
FLIP_CRITERIA = {"delaunay": 0, "valence": 1}
FLIP_COUNTS = ("edges", "candidates", "selected", "not_interior", "same_corner", "exists", "nonfinite", "criterion", "normals")
FLIP_REASONS = ("candidate", "not_interior", "same_corner", "exists", "nonfinite", "criterion", "normals")   # counts[2 + reason], r >= 1
FLIP_NO_EDGE = 255                      # edge_reason of a neighbour entry that names no edge (nbr <= owner, or past the entries)
FLIP_SALT_STEP = 0x9e3779b9             # the entry id is xor-ed with salt times this (mod 2^32) before it is hashed
_M32 = 0xffffffff


def flip_args(criterion, salt, what="mesh_flip_round"):
    """The scalars of `mesh_flip_round`, checked: -> (the criterion's number, salt as an integer in [0, 2^32))."""
    if criterion not in FLIP_CRITERIA:
        raise ValueError("%s: criterion must be 'delaunay' or 'valence', got %r" % (what, criterion))
    if isinstance(salt, bool) or not isinstance(salt, (int, np.integer)) or not 0 <= int(salt) <= _M32:
        raise ValueError("%s: salt must be an integer in [0, 2^32), got %r" % (what, salt))
    return FLIP_CRITERIA[criterion], int(salt)


def _mul32(x, m):
    """x m mod 2^32 for an int64 tensor x in [0, 2^32) and a constant m in [0, 2^32): no product leaves the int64 range."""
    return ((x * (m & 0xffff)) + (((x * (m >> 16)) & 0xffff) << 16)) & _M32


def flip_hash32(x):
    """The integer hash of the flip keys, on int64 tensors holding values in [0, 2^32): x ^= x >> 16, x *= 0x7feb352d, x ^= x >> 15,
    x *= 0x846ca68b, x ^= x >> 16, all mod 2^32 (a two-round multiply-xorshift finaliser; a bijection of the 32-bit integers)."""
    x = x ^ (x >> 16)
    x = _mul32(x, 0x7feb352d)
    x = x ^ (x >> 15)
    x = _mul32(x, 0x846ca68b)
    return x ^ (x >> 16)


def mesh_flip_round(verts, faces, criterion="delaunay", salt=0, adjacency=None, details=False):
    """One round of edge flips: verts (V,3) float32, faces (F,3) integer ids, criterion "delaunay" or "valence", salt the round
    number (an integer in [0, 2^32)), adjacency `mesh_adjacency` of the mesh or None.  Many independent edges flip at once; which
    ones is decided on integers, so the order in which a device's threads arrive does not show.  All floating point is float64
    from the float32 inputs, every operation rounded on its own; no square root, no trigonometry.

    EDGES: the neighbour entry i = (u, v) with v > u names the edge {u, v}; i is its id.  The first test that fails is the edge's
    reason (FLIP_REASONS) and is counted:
      1 not_interior  the entry does not carry one face each way (nbr_out = nbr_in = 1): a boundary, non-manifold or misoriented
                      edge.  Otherwise fa is the valid face that traverses u->v and a its third corner, fb the one that traverses
                      v->u and b its third corner.
      2 same_corner   a = b.
      3 exists        b is a neighbour of a: the flipped edge {a, b} is there already.
      4 nonfinite     one of u, v, a, b has a non-finite coordinate.
      5 criterion     Na = (u - a) x (v - a) and Nb = (v - b) x (u - b), the cross products of the corners (a, u, v) and (b, v, u),
                      N1 = (u - a) x (b - a) and N2 = (v - b) x (a - b) those of the new faces' corners (a, u, b) and (b, v, a),
                      every component (x y) - (z w).
                      "delaunay": d_x = ((u - x) . (v - x)) summed left to right for x = a, b; c_a = (Na0 Na0 + Na1 Na1) + Na2 Na2,
                      c_b the same of Nb.  The edge stays when d_a >= 0 and d_b >= 0; it flips when d_a < 0 and d_b < 0;
                      otherwise, with n the corner whose d is negative and o the other one, it flips when (d_n d_n) c_o >
                      (d_o d_o) c_n -- cot(angle at a) + cot(angle at b) < 0, strictly, so that co-circular quads stay.  The
                      edge flips when this test asks for it AND the same test of the flipped edge {a, b} does not ask to come
                      back: its corners are u and v, d_x = ((a - x) . (b - x)) for x = u, v, c_u and c_v the squared lengths of
                      N1 and N2 below.  The four angles of a quad in space sum to at most 2 pi, so in exact arithmetic the
                      second half never refuses; with rounded numbers a nearly co-circular quad (marching-cubes meshes are
                      full of them) can ask both ways, and would flip back and forth for ever.
                      "valence": deg = the number of neighbours, target = 4 for a vertex with vert_flags bit 0 (on a boundary)
                      and 6 otherwise; the edge flips when the sum of |deg - target| over u, v, a, b is strictly smaller with u
                      and v one lower and a and b one higher.  Integers only.
                      The reason holds when the criterion does not ask for the flip.
      6 normals       the reason holds unless (N 0 M 0 + N 1 M 1) + N 2 M 2 > 0 for every N of N1, N2 and every M of Na, Nb.
    An edge without a reason is a CANDIDATE with key = (hash32(i ^ (salt 0x9e3779b9 mod 2^32)) << 32) | i (`flip_hash32`), an
    unsigned 64-bit integer.

    SELECTION: lock[x] = the least key of the candidates that have x among their u, v, a, b; a candidate is selected when the
    locks of its four vertices all hold its key.  Keys are unique, so two selected flips share no vertex: they rewrite disjoint
    faces, create different edges, and no test one of them passed reads anything the other changes.

    APPLY: faces_out is a copy of faces (ids that do not fit int32 are -1) in which, for a selected edge, row fa is (a, u, b) and
    row fb is (b, v, a).  Vertices, the face count and the order stay.

    -> faces_out (F,3) int32, face_flag (F,) uint8 (1: the row was rewritten), counts (9,) int32 in the order of FLIP_COUNTS.
    details: also edge_key (6F,) int64 (the key's 64 bits, -1: no candidate), edge_reason (6F,) uint8 (FLIP_NO_EDGE where the
    entry names no edge) and selected (6F,) bool.  Plain tensor operations on the tensors' device: the specification of
    arah_mesh_flip_round (csrc/meshflip.hpp), and what runs for meshes on the host."""
    what = "mesh_flip_round"
    crit, salt = flip_args(criterion, salt, what)
    raw_faces = torch.as_tensor(faces)
    verts, faces, V, in_range = _mesh_verts(verts, faces, what)
    if raw_faces.dtype != torch.int32:
        faces = torch.where((faces >= 0) & (faces <= 2 ** 31 - 1), faces, torch.full_like(faces, -1))
    F, dev = int(faces.shape[0]), verts.device
    f64, i32, i64 = torch.float64, torch.int32, torch.int64
    adjacency = _adjacency_of(faces, V, adjacency, what)
    vf_start, vf, nbr_start, nbr, nbr_out, nbr_in = (t.long() for t in adjacency[:6])
    on_rim = (adjacency[6].long() & 1) != 0
    E = int(nbr_start[V])
    val, nvf = nbr_start[1:] - nbr_start[:-1], vf_start[1:] - vf_start[:-1]
    ev, en = torch.repeat_interleave(torch.arange(V, device=dev), val), nbr[:E]
    eid = torch.nonzero(en > ev)[:, 0]
    u, v = ev[eid], en[eid]
    n_edges = int(eid.shape[0])
    reason = torch.zeros(n_edges, dtype=i64, device=dev)
    reason[(nbr_out[eid] != 1) | (nbr_in[eid] != 1)] = 1
    qa, qb, qfa, qfb = (torch.zeros(n_edges, dtype=i64, device=dev) for _ in range(4))
    at = torch.nonzero(reason == 0)[:, 0]
    if at.numel():
        ub, vb = u[at], v[at]
        k, rows = _ragged(vf_start[ub], nvf[ub])
        fcs = vf[rows]
        shared = (faces[fcs] == vb[k][:, None]).any(1)
        fs, ks = fcs[shared], k[shared]                                             # two per edge: nbr_out = nbr_in = 1
        ids, us, vs = faces[fs], ub[k[shared]], vb[k[shared]]
        fwd = ((ids[:, 0] == us) & (ids[:, 1] == vs)) | ((ids[:, 1] == us) & (ids[:, 2] == vs)) | ((ids[:, 2] == us) & (ids[:, 0] == vs))
        third = ids.sum(1) - us - vs
        a, b, fa, fb = (torch.zeros(at.shape[0], dtype=i64, device=dev) for _ in range(4))
        a[ks[fwd]], fa[ks[fwd]], b[ks[~fwd]], fb[ks[~fwd]] = third[fwd], fs[fwd], third[~fwd], fs[~fwd]
        ekey = ev * max(V, 1) + en                                                  # ascending: the entries' own order
        want = a * max(V, 1) + b
        exists = ekey[torch.searchsorted(ekey, want).clamp(max=E - 1)] == want
        finite = torch.isfinite(verts).all(1)
        finite4 = finite[ub] & finite[vb] & finite[a] & finite[b]
        p = verts.to(f64)
        pu, pv, pa, pb = p[ub], p[vb], p[a], p[b]
        Na, Nb = _cross3(torch.stack([pa, pu, pv], 1)), _cross3(torch.stack([pb, pv, pu], 1))
        N1, N2 = _cross3(torch.stack([pa, pu, pb], 1)), _cross3(torch.stack([pb, pv, pa], 1))
        if crit == 0:
            def dot3(x, y):
                return (x[:, 0] * y[:, 0] + x[:, 1] * y[:, 1]) + x[:, 2] * y[:, 2]

            def wants(da, db, ca, cb):
                a_neg = (da * da) * cb > (db * db) * ca
                b_neg = (db * db) * ca > (da * da) * cb
                return torch.where((da < 0) & (db < 0), torch.ones_like(exists),
                                   torch.where((da < 0) & (db >= 0), a_neg, torch.where((db < 0) & (da >= 0), b_neg, torch.zeros_like(exists))))
            asks = wants(dot3(pu - pa, pv - pa), dot3(pu - pb, pv - pb), dot3(Na, Na), dot3(Nb, Nb))
            back = wants(dot3(pa - pu, pb - pu), dot3(pa - pv, pb - pv), dot3(N1, N1), dot3(N2, N2))
            asks = asks & ~back
        else:
            def off(x, step):
                return (val[x] + step - torch.where(on_rim[x], 4, 6)).abs()
            before = off(ub, 0) + off(vb, 0) + off(a, 0) + off(b, 0)
            after = off(ub, -1) + off(vb, -1) + off(a, 1) + off(b, 1)
            asks = after < before
        good = torch.ones_like(exists)
        for N in (N1, N2):
            for M in (Na, Nb):
                good = good & ((N[:, 0] * M[:, 0] + N[:, 1] * M[:, 1]) + N[:, 2] * M[:, 2] > 0)
        r = torch.where(a == b, 2, torch.where(exists, 3, torch.where(~finite4, 4, torch.where(~asks, 5, torch.where(~good, 6, 0)))))
        reason[at] = r.to(i64)
        qa[at], qb[at], qfa[at], qfb[at] = a, b, fa, fb
    cand = reason == 0
    # the key with its upper half shifted by 2^31: the signed order of `skey` is the unsigned order of the key
    h = flip_hash32(eid ^ ((salt * FLIP_SALT_STEP) & _M32))
    top = torch.iinfo(i64).max
    skey = torch.where(cand, (h - 2 ** 31) * 2 ** 32 + eid, torch.full_like(eid, top))
    lock = torch.full((V,), top, dtype=i64, device=dev)
    ci = torch.nonzero(cand)[:, 0]
    quad = torch.cat([u[ci], v[ci], qa[ci], qb[ci]])
    lock = lock.scatter_reduce(0, quad, skey[ci].repeat(4), "amin")
    selected = cand.clone()
    selected[ci] = (lock[quad].reshape(4, -1) == skey[ci][None, :]).all(0)
    si = torch.nonzero(selected)[:, 0]
    faces_out = faces.clone()
    face_flag = torch.zeros(F, dtype=torch.uint8, device=dev)
    faces_out[qfa[si]] = torch.stack([qa[si], u[si], qb[si]], 1)
    faces_out[qfb[si]] = torch.stack([qb[si], v[si], qa[si]], 1)
    face_flag[qfa[si]] = 1
    face_flag[qfb[si]] = 1
    counts = torch.tensor([n_edges, int(cand.sum()), int(si.shape[0])] + [int((reason == r).sum()) for r in range(1, 7)],
                          dtype=i32, device=dev)
    out = (faces_out.to(i32), face_flag, counts)
    if not details:
        return out
    edge_key = torch.full((6 * F,), -1, dtype=i64, device=dev)
    edge_reason = torch.full((6 * F,), FLIP_NO_EDGE, dtype=torch.uint8, device=dev)
    edge_sel = torch.zeros(6 * F, dtype=torch.bool, device=dev)
    edge_reason[eid], edge_sel[eid] = reason.to(torch.uint8), selected
    edge_key[eid] = torch.where(cand, skey ^ torch.iinfo(i64).min, torch.full_like(skey, -1))
    return out + (edge_key, edge_reason, edge_sel)


# ---- orientation, boundary loops, hole filling -----------------------------------------------------------------------------------
ORIENT_POLICIES ={"seed": 0, "majority": 1, "negative": 2, "positive": 3}
ORIENT_VOL_BITS = 18                    # quantised coordinates lie in [-2^18, 2^18]: a determinant of three stays below 2^57
FILL_MAX_EDGES = 1 << 26                # edges of a filled loop: 2^26 fixed-point coordinates below 2^36 sum below 2^62


def check_orient_policy(policy, what="mesh_orient"):
    if not isinstance(policy, str) or policy not in ORIENT_POLICIES:
        raise ValueError("%s: policy must be one of %s, got %r" % (what, ", ".join(ORIENT_POLICIES), policy))
    return ORIENT_POLICIES[policy]


def check_max_edges(max_edges, what="mesh_fill_holes"):
    if isinstance(max_edges, bool) or not isinstance(max_edges, (int, np.integer)) or not 0 <= int(max_edges) <= FILL_MAX_EDGES:
        raise ValueError("%s: max_edges must be an integer in [0, 2^26], got %r" % (what, max_edges))
    return int(max_edges)


def finite_bounds(verts):
    """(lo, hi), three float32 values each as Python floats: the box of the vertices whose three coordinates are finite, or None
    when there is none.  One host synchronisation for a tensor on the device."""
    if int(verts.shape[0]) == 0:
        return None
    v = verts.detach().float()
    finite = torch.isfinite(v).all(1, keepdim=True)
    inf = torch.full_like(v, float("inf"))
    lo, hi = torch.stack([torch.where(finite, v, inf).amin(0), torch.where(finite, v, -inf).amax(0)]).tolist()
    return None if lo[0] > hi[0] else (lo, hi)


def _pow2_scale(extent, bits):
    """2^(bits - e), e = ceil(log2(extent)): a length of at most `extent` times it is at most 2^bits.  1 for no extent."""
    if not extent > 0.0:
        return 1.0
    m, e = math.frexp(extent)
    e = e - 1 if m == 0.5 else e
    return math.ldexp(1.0, bits - e)


def orient_quant(verts):
    """The lattice of the exact volumes of `mesh_orient`, shared by the specification and the device: -> (origin, scale); origin =
    the float32 midpoint float32((lo + hi) / 2) of `finite_bounds`, scale = the power of two 2^(18 - e), e = ceil(log2(the largest
    distance of a bound from the origin along an axis)).  (0, 0, 0) and 1 without a finite vertex or an extent."""
    box = finite_bounds(verts)
    if box is None:
        return [0.0, 0.0, 0.0], 1.0
    lo, hi = box
    origin = [float(np.float32((l + h) / 2.0)) for l, h in zip(lo, hi)]
    half = max(max(h - o, o - l) for l, h, o in zip(lo, hi, origin))
    return origin, _pow2_scale(half, ORIENT_VOL_BITS)


def fill_quant(verts):
    """The fixed-point lattice of the new vertices of `mesh_fill_holes`, with the constants of `mesh_simplify`: -> (origin, scale);
    origin = the lower corner of `finite_bounds`, scale = 2^(36 - e), e = ceil(log2(the longest side)), so that the fixed-point
    coordinates of a finite vertex lie in [0, 2^36]."""
    box = finite_bounds(verts)
    if box is None:
        return [0.0, 0.0, 0.0], 1.0
    lo, hi = box
    return [float(x) for x in lo], _pow2_scale(max(h - l for l, h in zip(lo, hi)), SIMPLIFY_FIX_BITS)


def _check_quant(quant, what):
    try:
        origin, scale = quant
        origin, scale = [float(np.float32(float(x))) for x in origin], float(scale)
    except (TypeError, ValueError):
        raise ValueError("%s: quant must be (origin of three numbers, scale), got %r" % (what, quant))
    if len(origin) != 3 or not all(math.isfinite(x) for x in origin) or not (scale > 0.0 and math.isfinite(scale)):
        raise ValueError("%s: quant must be a finite origin and a finite scale > 0, got %r" % (what, quant))
    return origin, scale


def _min_labels(n, a, b):
    """The smallest node id of every node's connected component in the graph with n nodes and the edges (a[i], b[i]): every node
    takes the smallest label among itself and its neighbours, then its label's label, until nothing changes."""
    low = torch.arange(n, device=a.device)
    both = torch.cat([a, b])
    while both.shape[0]:
        m = torch.minimum(low[a], low[b])
        new = low.scatter_reduce(0, both, torch.cat([m, m]), "amin")
        new = new[new]
        if torch.equal(new, low):
            break
        low = new
    return low


def _faces_i32(faces, raw):
    """The faces as the device sees them: int32, an id that does not fit one replaced by -1 when the input is of another type."""
    if raw.dtype == torch.int32:
        return faces.to(torch.int32)
    return torch.where((faces >= 0) & (faces <= 2 ** 31 - 1), faces, torch.full_like(faces, -1)).to(torch.int32)


def _orient_args(verts, faces, what):
    """verts (V,3) float32 or a vertex count, faces: -> (verts or None, faces as int64, V, the valid rows' mask, the faces as the
    device sees them)."""
    raw = torch.as_tensor(faces)
    if isinstance(verts, torch.Tensor) and verts.dim() > 0:
        v, f, V, in_range = _mesh_verts(verts, faces, what)
    else:
        v = None
        f, V, in_range = _cc_faces(faces, verts, what)
        if int(f.shape[0]) > ADJACENCY_MAX_FACES:
            raise ValueError("%s: at most 2^28 faces, got %d" % (what, int(f.shape[0])))
    valid = in_range & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    return v, f, V, valid, _faces_i32(f, raw)


def _half_edges(f, valid, V):
    """The directed edges of the valid faces in ascending (face, corner) order: -> (start, end, face, the number of valid faces on
    the undirected edge of each)."""
    rows = torch.nonzero(valid)[:, 0]
    fv = f[rows]
    s, d, face = fv.reshape(-1), fv[:, [1, 2, 0]].reshape(-1), rows.repeat_interleave(3)
    W = max(V, 1)
    _, which, cnt = torch.unique(torch.minimum(s, d) * W + torch.maximum(s, d), return_inverse=True, return_counts=True)
    return s, d, face, (cnt[which] if s.shape[0] else s)


def mesh_orient(verts, faces, policy="majority", adjacency=None, quant=None):
    """Consistent orientation of an indexed mesh: verts (V,3) float32 -- or just the vertex count under the policies "seed" and
    "majority" --, faces (F,3) integer ids, F <= 2^28.

    VALIDITY and TRAVERSAL are those of `mesh_adjacency`.  Two valid faces are NEIGHBOURS across an undirected edge when exactly two
    valid faces lie on it: CONSISTENT (s = 0) when they traverse it in opposite directions, inconsistent (s = 1) otherwise; an edge
    with one face or with three or more carries no constraint.  ORIENTATION COMPONENTS are the classes of faces connected through
    such edges, numbered in ascending order of their lowest face id; an invalid face belongs to none (label -1).

    The relative flips come from the DOUBLE COVER: the nodes are 2 f + bit, a pair (f, g, s) joins 2 f with 2 g + s and 2 f + 1
    with 2 g + (1 - s), and root(x) is the smallest node of x's connected component.  root(2 f) >> 1 is the lowest face of f's
    component.  The component is NON-ORIENTABLE when root(2 f) == root(2 f + 1) (a Moebius strip): its faces are never flipped
    and have b = 0.  Otherwise b(f) = root(2 f) & 1 is the flip of f relative to the component's lowest face.

    The POLICY fixes what is left free in an orientable component: "seed" the lowest face keeps its orientation; "majority" the
    orientation held by more faces wins (the component is reversed when more faces have b = 1 than b = 0; a tie is "seed");
    "negative" / "positive" the component's signed volume gets that sign (the project's own meshes are negative).  The volume is
    an exact integer: q = llrint(clamp((double(v) - double(origin)) scale, -2^18, 2^18)) with (origin, scale) = quant, by default
    `orient_quant(verts)`; det(q0, q1, q2) of a face in int64 (|det| < 2^57), negated for a face with b = 1; a face with a
    non-finite vertex contributes nothing; the low 32 bits (unsigned) and the arithmetic high part d >> 32 are summed apart per
    component, the volume is hi 2^32 + lo.  A component whose volume is zero (smaller than a lattice step, an open sheet seen
    edge-on) falls back to "majority".  Under "seed" and "majority" the two sums stay zero.

    -> flip (F,) uint8: 1 where the face is reversed; face_comp (F,) int32; faces_out (F,3) int32: a flipped row (a, b, c) is
    (a, c, b), every other row is the input's, row order and vertices never change; comp_faces (F,) int32, comp_flags (F,) int32
    (bit 0 non-orientable, bit 1 the policy reversed the component), comp_vol_hi, comp_vol_lo (F,) int64, indexed by component
    and zero from the number of components on; counts (6,) int32: valid faces, components, non-orientable components, faces with
    b = 1, components reversed by the policy, faces flipped.  Integers throughout: the result is unique.  `adjacency` (the arrays
    of `mesh_adjacency`) is what the device searches partners in; here it is only checked for its shapes.  Plain tensor operations
    on the tensor's device: the specification of arah_mesh_orient (csrc/meshorient.hpp), and what runs for meshes on the host."""
    pol = check_orient_policy(policy)
    by_volume = pol >= 2
    v, f, V, valid, f32 = _orient_args(verts, faces, "mesh_orient")
    if by_volume and v is None:
        raise ValueError("mesh_orient: policy %r needs the vertices, not their number" % (policy,))
    dev, F, i32, i64 = f.device, int(f.shape[0]), torch.int32, torch.int64
    if adjacency is not None:
        _adjacency_of(f, V, adjacency, "mesh_orient")
    if by_volume:
        origin, scale = _check_quant(orient_quant(v) if quant is None else quant, "mesh_orient")
    # the pairs: the two half-edges of every undirected edge with exactly two faces, adjacent after a sort by edge
    s, d, face, on_edge = _half_edges(f, valid, V)
    two = torch.nonzero(on_edge == 2)[:, 0]
    order = two[torch.sort(torch.minimum(s, d)[two] * max(V, 1) + torch.maximum(s, d)[two], stable=True).indices]
    first, second = order[0::2], order[1::2]
    same = ((s[first] < d[first]) == (s[second] < d[second])).long()
    lo_f, hi_f = torch.minimum(face[first], face[second]), torch.maximum(face[first], face[second])
    root = _min_labels(2 * F, torch.cat([2 * lo_f, 2 * lo_f + 1]), torch.cat([2 * hi_f + same, 2 * hi_f + (1 - same)]))
    r0, r1 = root[0::2], root[1::2]
    ids = torch.arange(F, device=dev)
    froot = torch.where(valid, r0 >> 1, torch.full_like(r0, -1))
    b = valid & ((r0 & 1) == 1)
    is_root = froot == ids
    dense = torch.cumsum(is_root.long(), 0) - 1
    face_comp = torch.where(valid, dense[froot.clamp_min(0)], torch.full_like(froot, -1)) if F else froot
    n_comp = int(is_root.sum())
    comp_faces = torch.bincount(face_comp[valid], minlength=F)
    ones = torch.bincount(face_comp[b], minlength=F)
    nonor = torch.zeros(F, dtype=torch.bool, device=dev)
    nonor[face_comp[valid & (r0 == r1)]] = True
    vol_hi, vol_lo = torch.zeros(F, dtype=i64, device=dev), torch.zeros(F, dtype=i64, device=dev)
    if by_volume and V:
        rows = torch.nonzero(valid)[:, 0]
        p = v[f[rows]]                                                          # (Fv,3,3): corner, axis
        finite = torch.isfinite(p).all(2).all(1)
        lim = 2.0 ** ORIENT_VOL_BITS
        x = (p.to(torch.float64) - torch.tensor(origin, dtype=torch.float64, device=dev)) * scale
        q = torch.where(finite[:, None, None], x, torch.zeros_like(x)).clamp(-lim, lim).round().long()
        det = (q[:, 0, 0] * (q[:, 1, 1] * q[:, 2, 2] - q[:, 1, 2] * q[:, 2, 1]) - q[:, 0, 1] * (q[:, 1, 0] * q[:, 2, 2] - q[:, 1, 2] * q[:, 2, 0])
               + q[:, 0, 2] * (q[:, 1, 0] * q[:, 2, 1] - q[:, 1, 1] * q[:, 2, 0]))
        det = torch.where(b[rows], -det, det)[finite]
        comp = face_comp[rows][finite]
        vol_lo.index_add_(0, comp, det & 0xFFFFFFFF)
        vol_hi.index_add_(0, comp, det >> 32)
    # the sign of hi 2^32 + lo: the carry of lo goes to hi, what is left of lo is below 2^32 and cannot outweigh it
    hi2, lo2 = vol_hi + (vol_lo >> 32), vol_lo & 0xFFFFFFFF
    sign = torch.where(hi2 > 0, 1, torch.where(hi2 < 0, -1, (lo2 > 0).long()))
    majority = ones > comp_faces - ones
    if pol == 0:
        rev = torch.zeros_like(majority)
    elif pol == 1:
        rev = majority
    else:
        rev = torch.where(sign == 0, majority, sign > 0 if pol == 2 else sign < 0)
    rev = rev & ~nonor
    comp_flags = nonor.long() | (rev.long() << 1)
    fc = face_comp.clamp_min(0)
    flip = valid & ~nonor[fc] & (b ^ rev[fc]) if F else valid
    faces_out = torch.where(flip[:, None], f32[:, [0, 2, 1]], f32)
    counts = torch.tensor([int(valid.sum()), n_comp, int(nonor.sum()), int(b.sum()), int(rev.sum()), int(flip.sum())], dtype=i32, device=dev)
    return (flip.to(torch.uint8), face_comp.to(i32), faces_out, comp_faces.to(i32), comp_flags.to(i32), vol_hi, vol_lo, counts)


# ---- self-intersections and mesh-mesh intersections -------------------------------------------------------------------------------
INTERSECT_MAX_FACES = 1 << 26            # the faces the uniform grid of the device indexes
INTERSECT_MAX_PAIRS = 2 ** 31 - 1
INTERSECT_NAMES = ("hits", "vert_hit", "pair_start", "pairs", "counts")


def check_max_pairs(max_pairs, what="mesh_intersections"):
    if isinstance(max_pairs, bool) or not isinstance(max_pairs, (int, np.integer)) or not 0 <= int(max_pairs) <= INTERSECT_MAX_PAIRS:
        raise ValueError("%s: max_pairs must be an integer in [0, 2^31 - 1], got %r" % (what, max_pairs))
    return int(max_pairs)


def check_between(between, group, what="mesh_intersections"):
    if not isinstance(between, (bool, np.bool_)):
        raise ValueError("%s: between must be True or False, got %r" % (what, between))
    if bool(between) and group is None:
        raise ValueError("%s: between=True needs a group label per face" % what)
    return bool(between)


def check_group(group, n_faces, device, what="mesh_intersections"):
    """group: None, or (F,) uint8 on the faces' device: -> the tensor or None."""
    if group is None:
        return None
    if not isinstance(group, torch.Tensor) or group.dtype != torch.uint8 or tuple(group.shape) != (int(n_faces),):
        raise ValueError("%s: group must be an (F,) uint8 tensor, F = %d" % (what, int(n_faces)))
    if group.device != device:
        raise ValueError("%s: group lives on %s, faces on %s" % (what, group.device, device))
    return group.detach()


def intersect_soup(verts, faces, quant):
    """The quantised corners of `mesh_intersections`: verts (V,3) float32, faces (F,3) integer ids, quant = (origin, scale) ->
    q (F,3,3) int64 (face, corner, axis), void (F,) bool.  q = llrint(clamp((double(v) - double(origin)) scale, -2^18, 2^18)); a face
    with an id outside [0, V) or a non-finite vertex is void and has q = 0.  q.float() is the soup the device indexes."""
    v, f, V, in_range = _mesh_verts(verts, faces, "mesh_intersections")
    origin, scale = _check_quant(quant, "mesh_intersections")
    F, dev = int(f.shape[0]), f.device
    if V == 0 or F == 0:
        return torch.zeros(F, 3, 3, dtype=torch.int64, device=dev), torch.ones(F, dtype=torch.bool, device=dev)
    p = v[f.clamp(0, V - 1)]                                                        # (F,3,3): corner, axis
    void = ~in_range | ~torch.isfinite(p).all(2).all(1)
    lim = 2.0 ** ORIENT_VOL_BITS
    x = (p.to(torch.float64) - torch.tensor(origin, dtype=torch.float64, device=dev)) * scale
    q = torch.where(void[:, None, None], torch.zeros_like(x), x).clamp(-lim, lim).round().long()
    return q, void


def _orient4(a, b, c, d):
    """det[b - a; c - a; d - a] of (..., 3) int64 rows.  |q| <= 2^18: every difference is at most 2^19 in magnitude, every triple
    product at most 2^57, and the six of them add up to less than 6 2^57 < 2^60: exact in int64."""
    u, v, w = b - a, c - a, d - a
    return (u[..., 0] * (v[..., 1] * w[..., 2] - v[..., 2] * w[..., 1]) - u[..., 1] * (v[..., 0] * w[..., 2] - v[..., 2] * w[..., 0])
            + u[..., 2] * (v[..., 0] * w[..., 1] - v[..., 1] * w[..., 0]))


def _edges_cross(e, t):
    """(K,3,3) int64 each: does an edge of triangle e[k] properly cross triangle t[k]? -> (K,) bool."""
    side = [_orient4(t[:, 0], t[:, 1], t[:, 2], e[:, k]) for k in range(3)]
    cut = torch.zeros(e.shape[0], dtype=torch.bool, device=e.device)
    for k in range(3):
        j = (k + 1) % 3
        apart = ((side[k] > 0) & (side[j] < 0)) | ((side[k] < 0) & (side[j] > 0))
        s = [_orient4(e[:, k], e[:, j], t[:, m], t[:, (m + 1) % 3]) for m in range(3)]
        inside = ((s[0] >= 0) & (s[1] >= 0) & (s[2] >= 0)) | ((s[0] <= 0) & (s[1] <= 0) & (s[2] <= 0))
        cut = cut | (apart & inside)
    return cut


def mesh_intersections(verts, faces, group=None, between=False, quant=None, max_pairs=1 << 20, chunk_pairs=1 << 22):
    """Which faces of an indexed mesh cut through each other: verts (V,3) float32, faces (F,3) integer ids, F <= 2^26.  With `group`
    (F,) uint8 and between=True only pairs of faces from different groups count: the intersections BETWEEN two meshes.

    Integers only, so the answer is unique, symmetric in the two faces, and independent of the order of the faces, of their winding
    and of the order anything arrives in.

    QUANTISATION.  q = llrint(clamp((double(v) - double(origin)) scale, -2^18, 2^18)) per coordinate, (origin, scale) = quant, by
    default `orient_quant(verts)` (the lattice of `mesh_orient`'s volume policies).  A face with a vertex id outside [0, V) or a
    non-finite vertex is VOID: it intersects nothing and is counted.  Vertices that share an id share a q, and vertices of an
    unwelded soup that coincide still coincide after quantisation.

    ORIENTATION.  orient(a, b, c, d) = det[b - a; c - a; d - a] in int64: every difference is at most 2^19 in magnitude, every
    triple product at most 2^57, the six-term determinant stays below 2^60.

    PROPER CROSSING.  The segment pq properly crosses the triangle abc when orient(a,b,c,p) and orient(a,b,c,q) are both non-zero
    and of opposite sign, and orient(p,q,a,b), orient(p,q,b,c), orient(p,q,c,a) are all >= 0 or all <= 0 (the piercing point lies in
    the closed triangle).

    INTERSECTING FACES.  Two faces f != g intersect when any of the six tests holds: the three edges of one against the other
    face, both ways.  There is no special case for neighbours: an edge with an endpoint in the other face's plane never crosses it
    properly, so faces that share a vertex or an edge are reported only when they really fold through each other.  Exact
    duplicates, touching contact (a vertex or an edge lying in the other face's plane) and coplanar overlap are NOT intersections.
    A degenerate face (zero area; a repeated id is not void) has orient(a,b,c,.) = 0 everywhere: it can cut with its edges but
    cannot be cut.

    -> hits (F,) int32: the number of faces each face intersects; vert_hit (V,) uint8: 1 for every corner of a face with hits > 0;
    pair_start (F+1,) int32 and pairs (n,2) int32: the pairs f < g ordered by f, then g -- pair_start[f] is where f's pairs begin
    among ALL pairs and is always exact, pairs holds the first n = min(total, max_pairs) of them; counts (5,) int32: pairs, faces
    hit, vertices hit, void faces, pairs written.  Nothing is silently truncated: counts[0] > counts[4] says so.  More than
    2^31 - 1 pairs raise ValueError.

    A chunked brute force over all (f, g > f) with the integer box reject, chunk_pairs bounding the temporaries (the result does not
    depend on it); plain tensor operations on the tensor's device: the specification of arah_mesh_intersections
    (csrc/meshintersect.hpp), and what runs for meshes on the host."""
    what = "mesh_intersections"
    v, f, V, _ = _mesh_verts(verts, faces, what)
    F, dev, i32 = int(f.shape[0]), f.device, torch.int32
    if F > INTERSECT_MAX_FACES:
        raise ValueError("%s: at most 2^26 faces, got %d" % (what, F))
    between = check_between(between, group, what)
    group = check_group(group, F, dev, what)
    cap = check_max_pairs(max_pairs, what)
    if isinstance(chunk_pairs, bool) or not isinstance(chunk_pairs, (int, np.integer)) or int(chunk_pairs) < 1:
        raise ValueError("%s: chunk_pairs must be a positive integer, got %r" % (what, chunk_pairs))
    q, void = intersect_soup(v, f, _check_quant(orient_quant(v) if quant is None else quant, what))
    lo, hi = q.amin(1), q.amax(1)                                                   # (F,3): the integer boxes
    ids = torch.arange(F, device=dev)
    rows = max(1, int(chunk_pairs) // max(F, 1))
    found = []
    for f0 in range(0, F, rows):
        a = slice(f0, min(f0 + rows, F))
        cand = (ids[a, None] < ids[None, :]) & ~void[a, None] & ~void[None, :]
        cand = cand & (lo[a, None] <= hi[None, :]).all(2) & (lo[None, :] <= hi[a, None]).all(2)
        if between:
            cand = cand & (group[a, None] != group[None, :])
        i, j = torch.nonzero(cand, as_tuple=True)                                    # row-major: ordered by f, then g
        i = i + f0
        hit = _edges_cross(q[j], q[i]) | _edges_cross(q[i], q[j])
        found.append(torch.stack([i[hit], j[hit]], 1))
    allp = torch.cat(found) if found else torch.zeros(0, 2, dtype=torch.int64, device=dev)
    total = int(allp.shape[0])
    if total > INTERSECT_MAX_PAIRS:
        raise ValueError("%s: %d pairs do not fit an int32 count" % (what, total))
    above = torch.bincount(allp[:, 0], minlength=F)
    hits = above + torch.bincount(allp[:, 1], minlength=F)
    pair_start = torch.zeros(F + 1, dtype=torch.int64, device=dev)
    pair_start[1:] = torch.cumsum(above, 0)
    vert_hit = torch.zeros(V, dtype=torch.uint8, device=dev)
    vert_hit[f[hits > 0].reshape(-1)] = 1                                           # a face that is hit is not void: ids in range
    pairs = allp[:cap]
    counts = torch.tensor([total, int((hits > 0).sum()), int(vert_hit.sum()), int(void.sum()), int(pairs.shape[0])], dtype=i32, device=dev)
    return hits.to(i32), vert_hit, pair_start.to(i32), pairs.to(i32).contiguous(), counts


def mesh_boundary_loops(faces, n_verts, adjacency=None):
    """The boundary of an indexed mesh: faces (F,3) integer ids over V = n_verts vertices, validity and traversal as in
    `mesh_adjacency`.  A BOUNDARY HALF-EDGE is a directed edge a->b of a valid face whose undirected edge carries exactly one valid
    face; they are numbered in ascending (face, corner) order, corner c of (i0, i1, i2) starting the edge i_c -> i_(c+1).  A LOOP is a
    connected component of the boundary half-edges through shared vertex ids; loops are numbered in ascending order of their
    smallest vertex id.  A loop is SIMPLE when every vertex on it has exactly one outgoing and one incoming boundary half-edge: a
    connected simple loop is one closed polygon; two holes that touch at a vertex, or a hole in a misoriented neighbourhood, are
    not simple.  -> edges (3F,2) int32, edge_face (3F,) int32, edge_loop (3F,) int32, zero from the number of half-edges B on;
    loop_edges (V,) int32, loop_simple (V,) uint8, loop_vert (V,) int32 (the loop's smallest vertex), indexed by loop and zero
    from the number of loops L on; counts (3,) int32: B, L, the simple loops.  `adjacency` is what the device reads the edges'
    face counts from; here it is only checked for its shapes.  The specification of arah_mesh_boundary_loops."""
    f, V, in_range = _cc_faces(faces, n_verts, "mesh_boundary_loops")
    dev, F, i32 = f.device, int(f.shape[0]), torch.int32
    if F > ADJACENCY_MAX_FACES:
        raise ValueError("mesh_boundary_loops: at most 2^28 faces, got %d" % F)
    if adjacency is not None:
        _adjacency_of(f, V, adjacency, "mesh_boundary_loops")
    valid = in_range & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    s, d, face, on_edge = _half_edges(f, valid, V)
    keep = on_edge == 1
    a, b, face = s[keep], d[keep], face[keep]
    B = int(a.shape[0])
    low = _min_labels(V, a, b)
    vout, vin = torch.bincount(a, minlength=V), torch.bincount(b, minlength=V)
    on = (vout + vin) > 0
    is_root = on & (low == torch.arange(V, device=dev))
    dense = torch.cumsum(is_root.long(), 0) - 1
    L = int(is_root.sum())
    loop_of_edge = dense[low[a]]
    edges = torch.zeros(3 * F, 2, dtype=torch.int64, device=dev)
    edges[:B] = torch.stack([a, b], 1)
    edge_face, edge_loop = (torch.zeros(3 * F, dtype=torch.int64, device=dev) for _ in range(2))
    edge_face[:B], edge_loop[:B] = face, loop_of_edge
    loop_edges = torch.bincount(loop_of_edge, minlength=V)
    bad = torch.zeros(V, dtype=torch.bool, device=dev)
    bad[dense[low[on & ((vout != 1) | (vin != 1))]]] = True
    loop_simple = ~bad & (torch.arange(V, device=dev) < L)
    loop_vert = torch.zeros(V, dtype=torch.int64, device=dev)
    loop_vert[:L] = torch.nonzero(is_root)[:, 0]
    counts = torch.tensor([B, L, int(loop_simple.sum())], dtype=i32, device=dev)
    return edges.to(i32), edge_face.to(i32), edge_loop.to(i32), loop_edges.to(i32), loop_simple.to(torch.uint8), loop_vert.to(i32), counts


def mesh_fill_holes(verts, faces, max_edges=64, adjacency=None, loops=None, quant=None):
    """Small holes of an indexed mesh closed by a fan: verts (V,3) float32, faces (F,3) integer ids, loops: the arrays of
    `mesh_boundary_loops` of the mesh (built here when None).  A loop is FILLED when it is simple, 3 <= loop_edges <= max_edges and
    none of its vertices has a non-finite coordinate.  The filled loops, in loop order, append one vertex each after the V
    existing ones; every half-edge a->b of a filled loop appends, in edge order, the face (b, a, new vertex) after the F existing
    ones: it runs against the half-edge, so it is consistent with the face that owns it.  The new vertex is the mean of the
    loop's vertices by the fixed-point rule of `mesh_simplify`: q = llrint(clamp((double(v) - double(origin)) scale, -2^36,
    2^36)), S = sum q over the loop's n vertices in integers, float32(double(origin) + (double(S) / double(n)) / scale), with
    (origin, scale) = quant, by default `fill_quant(verts)`: the position does not depend on the order of arrival.

    -> verts_out (V + V // 3, 3) float32, vert_src (V + V // 3,) int32: a vertex's own id for the old ones, the loop's smallest
    vertex id for a new one (attributes are gathered by it, never averaged); faces_out (4F,3) int32, face_loop (4F,) int32: -1
    for the old faces, the loop of a new one; counts (5,) int32: boundary half-edges, loops, simple loops, filled loops, faces
    added.  Rows behind the filled loops and the added faces are zero.  The specification of arah_mesh_fill_holes."""
    max_edges = check_max_edges(max_edges)
    raw = torch.as_tensor(faces)
    v, f, V, _ = _mesh_verts(verts, faces, "mesh_fill_holes")
    dev, F, i32, f64 = f.device, int(f.shape[0]), torch.int32, torch.float64
    origin, scale = _check_quant(fill_quant(v) if quant is None else quant, "mesh_fill_holes")
    if loops is None:
        loops = mesh_boundary_loops(f, V, adjacency=adjacency)
    edges, _, edge_loop, loop_edges, loop_simple, loop_vert, lcounts = loops
    B, L, n_simple = lcounts.tolist()
    a, b, l = edges[:B, 0].long(), edges[:B, 1].long(), edge_loop[:B].long()
    n = loop_edges.long()
    cand = (loop_simple != 0) & (n >= 3) & (n <= max_edges) & (torch.arange(V, device=dev) < L)
    finite = torch.isfinite(v[a]).all(1) if B else torch.zeros(0, dtype=torch.bool, device=dev)
    nonfinite = torch.zeros(V, dtype=torch.bool, device=dev)
    nonfinite[l[cand[l] & ~finite]] = True
    filled = cand & ~nonfinite
    lrank = torch.where(filled, torch.cumsum(filled.long(), 0) - 1, torch.full((V,), -1, dtype=torch.int64, device=dev))
    Lf = int(filled.sum())
    o64 = torch.tensor(origin, dtype=f64, device=dev)
    use = filled[l] if B else finite
    lim = 2.0 ** SIMPLIFY_FIX_BITS
    q = torch.clamp((v[a[use]].to(f64) - o64) * scale, -lim, lim).round().long()
    S = torch.zeros(V, 3, dtype=torch.int64, device=dev).index_add_(0, l[use], q)
    which = torch.nonzero(filled)[:, 0]
    verts_out = torch.zeros(V + V // 3, 3, dtype=torch.float32, device=dev)
    verts_out[:V] = v
    verts_out[V:V + Lf] = (o64 + (S[which].to(f64) / n[which].to(f64)[:, None]) / scale).float()
    vert_src = torch.zeros(V + V // 3, dtype=torch.int64, device=dev)
    vert_src[:V] = torch.arange(V, device=dev)
    vert_src[V:V + Lf] = loop_vert.long()[which]
    Bf = int(use.sum())
    faces_out = torch.zeros(4 * F, 3, dtype=torch.int64, device=dev)
    faces_out[:F] = _faces_i32(f, raw).long()
    faces_out[F:F + Bf] = torch.stack([b[use], a[use], V + lrank[l[use]]], 1)
    face_loop = torch.zeros(4 * F, dtype=torch.int64, device=dev)
    face_loop[:F] = -1
    face_loop[F:F + Bf] = l[use]
    counts = torch.tensor([B, L, n_simple, Lf, Bf], dtype=i32, device=dev)
    return verts_out, vert_src.to(i32), faces_out.to(i32), face_loop.to(i32), counts


RASTER_CULL = {"none": 0, "back": 1, "front": 2}
_RASTER_EMPTY = 2 ** 63 - 1             # a pixel nothing covers; every real key is below it (z > 0: its bits are below 2^31)
_RASTER_CHUNK = 1 << 22                 # fragments the specification tests at a time


def check_raster_args(verts_uvz, faces, height, width, cull, what="mesh_rasterize"):
    """The arguments of `mesh_rasterize`, checked (nothing is converted or copied): -> (verts (V,3) float32, H, W, the cull code)."""
    if not isinstance(verts_uvz, torch.Tensor) or verts_uvz.dim() != 2 or verts_uvz.shape[1] != 3 or verts_uvz.dtype != torch.float32:
        raise ValueError("%s: verts_uvz must be a (V, 3) float32 tensor of (u, v, depth)" % what)
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError("%s: faces must be an (F, 3) tensor" % what)
    if faces.dtype.is_floating_point or faces.dtype.is_complex or faces.dtype == torch.bool:
        raise ValueError("%s: faces must hold integer vertex ids" % what)
    if faces.device != verts_uvz.device:
        raise ValueError("%s: verts live on %s, faces on %s" % (what, verts_uvz.device, faces.device))
    for name, x in (("height", height), ("width", width)):
        if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or int(x) < 1:
            raise ValueError("%s: %s must be an integer >= 1, got %r" % (what, name, x))
    if int(height) * int(width) > 2 ** 31 - 1 or int(faces.shape[0]) > 2 ** 31 - 1:
        raise ValueError("%s: at most 2^31 - 1 pixels and faces" % what)
    if cull not in RASTER_CULL:
        raise ValueError("%s: cull must be 'none', 'back' or 'front', got %r" % (what, cull))
    return verts_uvz.detach(), int(height), int(width), RASTER_CULL[cull]


def _raster_edges(p, px, py):
    """e0 = E(1,2), e1 = E(2,0), e2 = E(0,1) of the corners p (...,3,3) at the pixel centres (px, py), float32, every operation
    rounded on its own."""
    dx, dy = p[..., 0] - px[..., None], p[..., 1] - py[..., None]
    return (dx[..., 1] * dy[..., 2] - dx[..., 2] * dy[..., 1], dx[..., 2] * dy[..., 0] - dx[..., 0] * dy[..., 2],
            dx[..., 0] * dy[..., 1] - dx[..., 1] * dy[..., 0])


def mesh_rasterize(verts_uvz, faces, height, width, z_near=1e-4, cull="none"):
    """An indexed mesh drawn, one face per pixel: what pytorch3d's MeshRasterizer returns (pix_to_face, zbuf, bary_coords with
    perspective correction, no blur).  verts_uvz (V,3) float32 = (u, v, z) per vertex, pixel coordinates and view depth, what
    `project_opencv` / `project_lookat` return; faces (F,3) integer ids.  Pixel (i, j) has its centre at px = j + 0.5, py = i +
    0.5.  -> pix_to_face (H,W) int32, depth (H,W) float32, bary (H,W,3) float32; -1 in all three where nothing covers.

    All float32 arithmetic has every operation rounded on its own.

      * A face is VALID when its three ids lie in [0, V), all three z are finite and > float32(z_near), and area2 = (x1-x0)*(y2-y0) -
        (x2-x0)*(y1-y0) is finite and not 0 (a repeated id gives 0).  cull="back" also drops area2 < 0, "front" area2 > 0.  Under
        `project_opencv` (u to the right, v DOWN, looking along +z) a face seen from the side its right-hand normal (p1 - p0) x
        (p2 - p0) points to has area2 < 0: that camera frame is right-handed with z away from the viewer, so such a face's
        normal has a negative z there, and area2 has the sign of that z.
      * Its pixels are those whose centres lie in the closed bounding box of its three vertices, clipped to the image: columns
        max(ceil(xmin - 0.5), 0) .. min(floor(xmax - 0.5), W - 1), rows alike, whatever the size of the box.  (A centre inside the
        triangle lies inside its box; said here so that the kernels and this agree on every sliver as well.)
      * Edge functions E(a,b) = (xa-px)*(yb-py) - (xb-px)*(ya-py): e0 = E(1,2), e1 = E(2,0), e2 = E(0,1).  The pixel is COVERED when
        all three are >= 0 (area2 > 0) or all three <= 0 (area2 < 0), and s = (e0+e1)+e2 != 0.  The test is inclusive on purpose:
        E(a,b) is -E(b,a) bit for bit, so two consistently oriented faces that share an edge leave no pixel centre between them
        uncovered; the depth key settles who gets a centre both cover.
      * The fragment's depth, perspective-correct: q = ((e0/z0 + e1/z1) + e2/z2) / s, z = 1/q; a fragment whose z is not finite and
        > 0 is dropped.
      * The pixel goes to the smallest 64-bit key (bits(z) << 32) | face id: the nearest face, and the lowest id on an exact tie.
        depth is the key's z bit for bit.
      * The winner's barycentrics in float64 from the same float32 e_k: b_k = e_k / ((e0+e1)+e2), p_k = b_k / z_k, bary_k =
        float32(p_k / ((p0+p1)+p2)).

    Plain tensor operations on the tensors' device (with host synchronisations): the specification of arah_mesh_rasterize
    (csrc/meshraster.hpp), and what runs for meshes on the host."""
    verts, H, W, cull = check_raster_args(verts_uvz, faces, height, width, cull)
    faces = faces.detach().long()
    dev, V, F, f32 = verts.device, int(verts.shape[0]), int(faces.shape[0]), torch.float32
    keys = torch.full((H * W,), _RASTER_EMPTY, dtype=torch.int64, device=dev)
    if V > 0 and F > 0:
        ok = ((faces >= 0) & (faces < V)).all(1)
        p = verts[faces.clamp(0, V - 1)]                                        # (F,3,3); rows of invalid faces are never used
        x, y, z = p[..., 0], p[..., 1], p[..., 2]
        ok = ok & (z > torch.tensor(float(z_near), dtype=f32, device=dev)).all(1) & torch.isfinite(z).all(1)
        area2 = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (x[:, 2] - x[:, 0]) * (y[:, 1] - y[:, 0])
        ok = ok & torch.isfinite(area2) & (area2 != 0)
        if cull == 1:
            ok = ok & ~(area2 < 0)
        elif cull == 2:
            ok = ok & ~(area2 > 0)
        # the clipped box: in float32, held to [-1, the largest float32 below 2^31], then integers (NaN only in faces already dropped)
        lim = 2147483520.0

        def to_int(t):
            return torch.nan_to_num(t, nan=-1.0).clamp(-1.0, lim).long()
        j0 = to_int(torch.ceil(x.min(1).values - 0.5)).clamp_min(0)
        j1 = to_int(torch.floor(x.max(1).values - 0.5)).clamp_max(W - 1)
        i0 = to_int(torch.ceil(y.min(1).values - 0.5)).clamp_min(0)
        i1 = to_int(torch.floor(y.max(1).values - 0.5)).clamp_max(H - 1)
        ok = ok & (j0 <= j1) & (i0 <= i1)
        rows = torch.nonzero(ok)[:, 0]
        n_box = ((j1 - j0 + 1) * (i1 - i0 + 1))[rows]
        n_box, order = torch.sort(n_box)
        rows = rows[order]
        sizes = n_box.tolist()
        a = 0
        while a < len(sizes):                                                   # faces of like size together, <= _RASTER_CHUNK fragments
            lo, b = a + 1, min(len(sizes), a + max(1, _RASTER_CHUNK // sizes[a]))
            while lo < b:                                                        # the most faces whose padded boxes fit (sizes ascend)
                mid = (lo + b + 1) // 2
                lo, b = (mid, b) if (mid - a) * sizes[mid - 1] <= _RASTER_CHUNK else (lo, mid - 1)
            r = rows[a:b]
            k = torch.arange(sizes[b - 1], device=dev)[None, :]                  # (1,n): the box in row-major order
            w = (j1[r] - j0[r] + 1)[:, None]
            inside = k < n_box[a:b, None]
            i, j = i0[r][:, None] + k // w, j0[r][:, None] + k % w
            pr, pos = p[r][:, None], (area2[r] > 0)[:, None]
            e0, e1, e2 = _raster_edges(pr, j.to(f32) + 0.5, i.to(f32) + 0.5)
            cov = torch.where(pos, (e0 >= 0) & (e1 >= 0) & (e2 >= 0), (e0 <= 0) & (e1 <= 0) & (e2 <= 0))
            s = (e0 + e1) + e2
            q = ((e0 / pr[..., 0, 2] + e1 / pr[..., 1, 2]) + e2 / pr[..., 2, 2]) / s
            zf = torch.ones_like(q) / q
            cov = inside & cov & (s != 0) & torch.isfinite(zf) & (zf > 0)
            key = (zf.contiguous().view(torch.int32).long() << 32) | r[:, None]
            pix, key = (i * W + j)[cov], key[cov]
            # the smallest key per pixel: sorted by key, then stably by pixel, the first of every run
            key, o = torch.sort(key)
            pix, o = torch.sort(pix[o], stable=True)
            key = key[o]
            first = torch.ones_like(pix, dtype=torch.bool)
            first[1:] = pix[1:] != pix[:-1]
            pix, key = pix[first], key[first]
            keys[pix] = torch.minimum(keys[pix], key)
            a = b
    hit = keys != _RASTER_EMPTY
    face = torch.where(hit, keys & 0xffffffff, torch.zeros_like(keys))
    depth = torch.where(hit, (keys >> 32).to(torch.int32).view(f32), torch.full((), -1.0, dtype=f32, device=dev))
    bary = torch.full((H * W, 3), -1.0, dtype=f32, device=dev)
    if V > 0 and F > 0:
        pw = verts[faces.clamp(0, V - 1)[face]]                                 # (HW,3,3): the winner's corners
        pid = torch.arange(H * W, device=dev)
        e = torch.stack(_raster_edges(pw, (pid % W).to(f32) + 0.5, (pid // W).to(f32) + 0.5), dim=1).to(torch.float64)
        b = e / ((e[:, 0] + e[:, 1]) + e[:, 2])[:, None]
        pk = b / pw[..., 2].to(torch.float64)
        bary = torch.where(hit[:, None], (pk / ((pk[:, 0] + pk[:, 1]) + pk[:, 2])[:, None]).to(f32), bary)
    pix_to_face = torch.where(hit, face, torch.full_like(face, -1)).to(torch.int32)
    return pix_to_face.reshape(H, W), depth.reshape(H, W), bary.reshape(H, W, 3)


def check_interpolate_args(pix_to_face, bary, faces, attr, what="interpolate_attributes"):
    """The arguments of `interpolate_attributes`, checked (nothing is converted or copied): -> (pix_to_face (H,W), bary (H,W,3)
    float32, attr (V,C) float32)."""
    if not isinstance(pix_to_face, torch.Tensor) or pix_to_face.dim() != 2 or pix_to_face.dtype.is_floating_point \
            or pix_to_face.dtype == torch.bool or pix_to_face.numel() == 0:
        raise ValueError("%s: pix_to_face must be an (H, W) integer tensor" % what)
    if not isinstance(bary, torch.Tensor) or tuple(bary.shape) != (*pix_to_face.shape, 3) or bary.dtype != torch.float32:
        raise ValueError("%s: bary must be the (H, W, 3) float32 tensor of pix_to_face's rasterisation" % what)
    if not isinstance(attr, torch.Tensor) or attr.dim() != 2 or attr.dtype != torch.float32 or not 1 <= int(attr.shape[1]) <= 32:
        raise ValueError("%s: attr must be a (V, C) float32 tensor with 1 <= C <= 32" % what)
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError("%s: faces must be an (F, 3) tensor" % what)
    if faces.dtype.is_floating_point or faces.dtype.is_complex or faces.dtype == torch.bool:
        raise ValueError("%s: faces must hold integer vertex ids" % what)
    if len({pix_to_face.device, bary.device, faces.device, attr.device}) != 1:
        raise ValueError("%s: pix_to_face, bary, faces and attr must live on one device" % what)
    return pix_to_face.detach(), bary.detach(), attr.detach()


def interpolate_attributes(pix_to_face, bary, faces, attr, background=0.0):
    """Per-vertex attributes attr (V,C) float32, 1 <= C <= 32, drawn with the pix_to_face (H,W) and bary (H,W,3) of
    `mesh_rasterize` (pytorch3d's interpolate_face_attributes): -> (H,W,C) float32, float32((b0*a0 + b1*a1) + b2*a2) with the
    products and sums in float64 on the float32 bary and attribute values, every operation rounded on its own.  float32(background)
    where pix_to_face names no face of this mesh (-1), or a face with an id outside [0, V).  The specification of
    arah_mesh_interpolate (csrc/meshraster.hpp), and what runs for meshes on the host."""
    p2f, bary, attr = check_interpolate_args(pix_to_face, bary, faces, attr)
    p2f, faces = p2f.long(), faces.detach().long()
    dev, V, F, C, f64 = attr.device, int(attr.shape[0]), int(faces.shape[0]), int(attr.shape[1]), torch.float64
    out = torch.full((*p2f.shape, C), float(background), dtype=torch.float32, device=dev)
    if V == 0 or F == 0:
        return out
    named = (p2f >= 0) & (p2f < F)
    ids = faces[p2f.clamp(0, F - 1)]                                            # (H,W,3)
    named = named & ((ids >= 0) & (ids < V)).all(-1)
    a = attr.to(f64)[ids.clamp(0, V - 1)]                                       # (H,W,3,C)
    b = bary.to(f64)[..., None]
    val = ((b[..., 0, :] * a[..., 0, :] + b[..., 1, :] * a[..., 1, :]) + b[..., 2, :] * a[..., 2, :]).to(torch.float32)
    return torch.where(named[..., None], val, out)


RAY_CULL = {"none": 0, "back": 1, "front": 2}


def check_raycast_args(tris, origins, dirs, t_min, t_max, cull, what="mesh_raycast"):
    """The arguments of `mesh_raycast`, checked (nothing is converted or copied): -> (float(t_min), float(t_max), the cull code)."""
    if not isinstance(tris, torch.Tensor) or tris.dim() != 3 or tuple(tris.shape[1:]) != (3, 3) or tris.dtype != torch.float32:
        raise ValueError("%s: tris must be an (F, 3, 3) float32 triangle soup" % what)
    if tris.shape[0] < 1:
        raise ValueError("%s: tris holds no triangle" % what)
    for name, x in (("origins", origins), ("dirs", dirs)):
        if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[1] != 3 or x.dtype != torch.float32:
            raise ValueError("%s: %s must be (R, 3) float32" % (what, name))
    if origins.shape[0] != dirs.shape[0]:
        raise ValueError("%s: %d origins but %d directions" % (what, origins.shape[0], dirs.shape[0]))
    if len({tris.device, origins.device, dirs.device}) != 1:
        raise ValueError("%s: tris, origins and dirs must live on one device" % what)
    if int(origins.shape[0]) > 2 ** 31 - 1 - 256 or int(tris.shape[0]) > 2 ** 31 - 1:
        raise ValueError("%s: at most 2^31 - 257 rays and 2^31 - 1 faces" % what)
    for name, x in (("t_min", t_min), ("t_max", t_max)):
        if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or math.isnan(float(x)):
            raise ValueError("%s: %s must be a number, got %r" % (what, name, x))
    if cull not in RAY_CULL:
        raise ValueError("%s: cull must be 'none', 'back' or 'front', got %r" % (what, cull))
    return float(t_min), float(t_max), RAY_CULL[cull]


def mesh_raycast(tris, origins, dirs, t_min=0.0, t_max=float("inf"), cull="none", chunk_bytes=1 << 28):
    """The first hit of every ray o + t d with the triangle soup tris (F,3,3) float32, origins and dirs (R,3) float32 (dirs need not
    be unit: t is in units of |d|): -> t (R,) float64, face (R,) int32, bary (R,3) float64; a miss is face -1, t +inf, bary 0.  Brute
    force over all faces, on the tensors' device; the specification of arah_mesh_raycast (csrc/meshray.hpp).

    The test is Woop, Benthin and Wald's watertight one ("Watertight Ray/Triangle Intersection", JCGT 2013) in float64 on the float32
    inputs, every operation rounded on its own.  kz = the axis of the largest |d| (the lowest on a tie), kx = (kz+1)%3,
    ky = (kx+1)%3, swapped when d[kz] < 0; Sx = d[kx]/d[kz], Sy = d[ky]/d[kz], Sz = 1/d[kz].  For a face a, b, c: A = a - o,
    Ax = A[kx] - Sx A[kz], Ay = A[ky] - Sy A[kz], Az = A[kz] (B, C alike); U = Cx By - Cy Bx, V = Ax Cy - Ay Cx, W = Bx Ay - By Ax.
    The face is missed when (U<0 or V<0 or W<0) and (U>0 or V>0 or W>0) -- inclusive: a ray through a shared edge or vertex is
    accepted by at least one of the faces -- or when det = (U+V)+W is 0.  det > 0 is a hit on the FRONT of the face, the side its
    normal (b-a)x(c-a) points to (the ray runs against the normal); cull="back" drops the hits with det < 0, cull="front" those
    with det > 0.  t = ((U (Sz Az) + V (Sz Bz)) + W (Sz Cz)) / det is accepted when it is finite, t_min <= t <= t_max, and the
    hit is ON THE RAY: with bary = (U, V, W) / det and A0 = a - o (B0, C0 alike), |((bary_0 A0 + bary_1 B0) + bary_2 C0) - t d| <=
    2^-26 m along each of kx, ky, kz, m the largest magnitude among the coordinates of o, a, b, c.  Woop's test leaves this to the
    conditioning of det: for a ray IN the plane of a face two of U, V, W are exactly 0 and the third is rounding noise, det is
    not 0, and a "hit" comes out at a corner far beside the ray; such a face is a miss here (a true hit is on the ray to
    ~2^-50 m).  The answer is the lexicographic minimum of (t, face) over the accepted faces, bary of that face.  A ray whose
    direction is zero or not finite, or whose origin is not finite, hits nothing; a face with a vertex that is not finite is never
    hit.  chunk_bytes bounds the (rays x faces) temporaries; the result does not depend on it."""
    t_min, t_max, cull_code = check_raycast_args(tris, origins, dirs, t_min, t_max, cull)
    f64, dev = torch.float64, tris.device
    R, F = int(origins.shape[0]), int(tris.shape[0])
    t_out = torch.full((R,), float("inf"), dtype=f64, device=dev)
    face_out = torch.full((R,), -1, dtype=torch.int32, device=dev)
    bary_out = torch.zeros(R, 3, dtype=f64, device=dev)
    if R == 0:
        return t_out, face_out, bary_out
    T, O, D = tris.detach().to(f64), origins.detach().to(f64), dirs.detach().to(f64)
    face_ok = torch.isfinite(T).all(-1).all(-1)                                             # (F,)
    face_max = T.abs().amax((1, 2))
    ad = D.abs()
    kz = torch.where((ad[:, 0] >= ad[:, 1]) & (ad[:, 0] >= ad[:, 2]), 0, torch.where(ad[:, 1] >= ad[:, 2], 1, 2))
    neg = torch.gather(D, 1, kz[:, None])[:, 0] < 0
    ray_ok = torch.isfinite(D).all(1) & torch.isfinite(O).all(1) & (ad > 0).any(1)
    ids = torch.arange(F, device=dev)
    per = max(1, int(chunk_bytes) // (F * 8 * 40))
    for axis in range(3):
        for swap in (False, True):
            kx, ky = (axis + 1) % 3, (axis + 2) % 3
            if swap:
                kx, ky = ky, kx
            rows_all = torch.nonzero(ray_ok & (kz == axis) & (neg == swap))[:, 0]
            for r0 in range(0, int(rows_all.shape[0]), per):
                rows = rows_all[r0:r0 + per]
                o, d = O[rows], D[rows]
                Sx, Sy, Sz = (d[:, kx] / d[:, axis])[:, None], (d[:, ky] / d[:, axis])[:, None], (1.0 / d[:, axis])[:, None]

                def sheared(corner):
                    Pz = T[None, :, corner, axis] - o[:, axis, None]
                    Px0, Py0 = T[None, :, corner, kx] - o[:, kx, None], T[None, :, corner, ky] - o[:, ky, None]
                    return Px0 - Sx * Pz, Py0 - Sy * Pz, Pz, Px0, Py0
                Ax, Ay, Az, Ax0, Ay0 = sheared(0)
                Bx, By, Bz, Bx0, By0 = sheared(1)
                Cx, Cy, Cz, Cx0, Cy0 = sheared(2)
                U = Cx * By - Cy * Bx
                V = Ax * Cy - Ay * Cx
                W = Bx * Ay - By * Ax
                miss = ((U < 0) | (V < 0) | (W < 0)) & ((U > 0) | (V > 0) | (W > 0))
                det = (U + V) + W
                miss = miss | (det == 0)
                if cull_code == 1:
                    miss = miss | (det < 0)
                elif cull_code == 2:
                    miss = miss | (det > 0)
                t = ((U * (Sz * Az) + V * (Sz * Bz)) + W * (Sz * Cz)) / det
                ok = ~miss & torch.isfinite(t) & (t >= t_min) & (t <= t_max) & face_ok[None, :]
                bu, bv, bw = U / det, V / det, W / det
                tol = torch.maximum(o.abs().amax(1)[:, None], face_max[None, :]) * 2.0 ** -26
                for P0, Q0, R0, k in ((Ax0, Bx0, Cx0, kx), (Ay0, By0, Cy0, ky), (Az, Bz, Cz, axis)):
                    ok = ok & ((((bu * P0 + bv * Q0) + bw * R0) - t * d[:, k, None]).abs() <= tol)
                tm = torch.where(ok, t, torch.full_like(t, float("inf")))
                best = tm.min(dim=1).values
                first = torch.where(ok & (tm == best[:, None]), ids[None, :], F).min(dim=1).values     # F: nothing accepted
                hit = first < F
                g = first.clamp(max=F - 1)[:, None]
                pick = lambda x: torch.gather(x, 1, g)[:, 0]
                dg = pick(det)
                zero = torch.zeros_like(dg)
                t_out[rows] = torch.where(hit, pick(t), torch.full_like(dg, float("inf")))
                face_out[rows] = torch.where(hit, first, torch.full_like(first, -1)).to(torch.int32)
                bary_out[rows] = torch.stack([torch.where(hit, pick(bu), zero), torch.where(hit, pick(bv), zero),
                                              torch.where(hit, pick(bw), zero)], dim=1)
    return t_out, face_out, bary_out


CONTAINS_MIN_RESOLUTION, CONTAINS_MAX_RESOLUTION = 2, 4096
CONTAINS_MAX_FACES = 1 << 28


def check_contains_args(verts, faces, points, resolution, what="mesh_contains"):
    """The arguments of `mesh_contains`, checked (nothing is converted or copied): -> int(resolution).  points may be None."""
    if isinstance(resolution, bool) or not isinstance(resolution, (int, np.integer)):
        raise ValueError("%s: resolution must be an integer, got %r" % (what, resolution))
    if not CONTAINS_MIN_RESOLUTION <= int(resolution) <= CONTAINS_MAX_RESOLUTION:
        raise ValueError("%s: resolution must lie in [%d, %d], got %d"
                         % (what, CONTAINS_MIN_RESOLUTION, CONTAINS_MAX_RESOLUTION, int(resolution)))
    if not isinstance(verts, torch.Tensor) or verts.dim() != 2 or verts.shape[1] != 3 or not verts.dtype.is_floating_point:
        raise ValueError("%s: verts must be a floating-point (V, 3) tensor" % what)
    if (not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype.is_floating_point
            or faces.dtype == torch.bool):
        raise ValueError("%s: faces must be an integer (F, 3) tensor" % what)
    if int(faces.shape[0]) > CONTAINS_MAX_FACES or int(verts.shape[0]) > 2 ** 31 - 1:
        raise ValueError("%s: at most 2^28 faces and 2^31 - 1 vertices" % what)
    if verts.device != faces.device:
        raise ValueError("%s: verts and faces must live on one device" % what)
    if points is not None:
        if (not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3
                or points.dtype not in (torch.float32, torch.float64)):
            raise ValueError("%s: points must be (P, 3) float32 or float64" % what)
        if points.device != verts.device:
            raise ValueError("%s: points live on %s, the mesh on %s" % (what, points.device, verts.device))
        if int(points.shape[0]) > 2 ** 31 - 1:
            raise ValueError("%s: at most 2^31 - 1 points" % what)
    return int(resolution)


def mesh_contains(verts, faces, points, resolution=512, chunk_pairs=1 << 24):
    """Is a point inside a mesh: verts (V,3) floating point, faces (F,3) integer, points (P,3) float32 or float64 on one device ->
    inside (P,) bool, ambiguous (P,) bool, tested (P,) int32.  The specification of arah_mesh_contains (csrc/meshcontains.hpp): the
    reference's `MeshIntersector.query` (im2mesh/utils/libmesh/inside_mesh.py) with its `TriangleHash` (triangle_hash.pyx) restated
    as a predicate over all (point, triangle) pairs.  float64 throughout, every operation rounded on its own.

    Bounds: lo, hi over the vertices that some face uses; scale = (resolution - 1) / (hi - lo), translate = 0.5 - scale lo, and
    q = scale x + translate for points and triangle corners alike.  in_box: 0 <= q <= resolution on all three axes (a NaN makes it
    false).  Candidates: a point reads the one cell ((int)q.x, (int)q.y) of the hash over the xy plane; a cell outside
    [0, resolution) -- q == resolution, which is in the box -- holds nothing.  Triangle t is a candidate iff the cell lies, on both
    axes, within [clip((int)min_t), clip((int)max_t)] of its three rescaled corners, clipped to [0, resolution - 1]; `tested`
    counts the candidates (0 for a point outside the box).  Per candidate, with A = (t1 - t3, t2 - t3) in 2-D, y = q - t3, detA =
    A00 A11 - A01 A10, s = sign(detA): u = (A11 y0 - A01 y1) s, v = (-A10 y0 + A00 y1) s; the column crosses the triangle when
    0 < u < |detA|, 0 < v < |detA| and 0 < u + v < |detA|, all STRICT (detA == 0 never passes).  n = (t3 - t1) x (t2 - t1); a
    vertical triangle (n_z == 0) is skipped; depth = t1_z |n_z| + (n_x (t1_x - q_x) + n_y (t1_y - q_y)) sign(n_z) counts into n0
    when depth >= q_z |n_z|, else into n1.  inside = in_box & n0 odd & n1 odd; ambiguous = in_box & (n0 odd != n1 odd), for which
    the reference only prints a warning.

    The rule is the reference's and is deliberately strict: a point whose z-column passes exactly through an edge or a vertex in
    rescaled coordinates counts no crossing there and may be answered "outside" (or ambiguous) although it lies inside.  The hash
    is part of the rule: a sliver triangle whose rounded 2-D test passes outside its own bounding box is not a candidate there.

    Degenerate meshes -- no face, a face id outside [0, V), a non-finite vertex that a face uses, an axis with hi == lo (the
    reference would divide by zero) --: every point is outside, not ambiguous, tested 0.  chunk_pairs bounds the (points x faces)
    temporaries; the result does not depend on it."""
    res = check_contains_args(verts, faces, points, resolution)
    f64, dev = torch.float64, verts.device
    P, F, V = int(points.shape[0]), int(faces.shape[0]), int(verts.shape[0])
    n0 = torch.zeros(P, dtype=torch.int64, device=dev)
    n1 = torch.zeros(P, dtype=torch.int64, device=dev)
    tested = torch.zeros(P, dtype=torch.int32, device=dev)
    nothing = torch.zeros(P, dtype=torch.bool, device=dev)
    if F == 0 or V == 0:
        return nothing, nothing.clone(), tested
    fc = faces.detach().long()
    if not bool(((fc >= 0) & (fc < V)).all()):
        return nothing, nothing.clone(), tested
    tri = verts.detach().to(f64)[fc]                                                        # (F,3,3)
    lo, hi = tri.reshape(-1, 3).amin(0), tri.reshape(-1, 3).amax(0)
    if not bool(torch.isfinite(tri).all()) or not bool((hi > lo).all()):
        return nothing, nothing.clone(), tested
    scale = torch.full_like(lo, float(res - 1)) / (hi - lo)       # a true division (number / tensor would multiply by a reciprocal)
    translate = 0.5 - scale * lo
    tri = scale * tri + translate
    q = scale * points.detach().to(f64) + translate
    in_box = ((0 <= q) & (q <= res)).all(1)
    t1, t2, t3 = tri[:, 0], tri[:, 1], tri[:, 2]
    A00, A01, A10, A11 = t1[:, 0] - t3[:, 0], t2[:, 0] - t3[:, 0], t1[:, 1] - t3[:, 1], t2[:, 1] - t3[:, 1]
    detA = A00 * A11 - A01 * A10
    one = torch.ones_like(detA)
    s_det, a_det = torch.where(detA > 0, one, -one), detA.abs()
    v1, v2 = t3 - t1, t2 - t1
    nx = v1[:, 1] * v2[:, 2] - v1[:, 2] * v2[:, 1]
    ny = v1[:, 2] * v2[:, 0] - v1[:, 0] * v2[:, 2]
    nz = v1[:, 0] * v2[:, 1] - v1[:, 1] * v2[:, 0]
    s_n, a_n = torch.where(nz > 0, one, -one), nz.abs()
    t1z_an = t1[:, 2] * a_n
    r0 = tri[:, :, :2].amin(1).trunc().long().clamp(0, res - 1)                             # (F,2)
    r1 = tri[:, :, :2].amax(1).trunc().long().clamp(0, res - 1)
    cell = torch.nan_to_num(q[:, :2], nan=-1.0).clamp(-1.0, res + 1.0).trunc().long()        # (P,2): (int)q
    has_cell = ((cell >= 0) & (cell < res)).all(1)
    per = max(1, int(chunk_pairs) // F)
    for p0 in range(0, P, per):
        c = cell[p0:p0 + per]
        cand = (has_cell[p0:p0 + per, None] & (r0[None, :, 0] <= c[:, None, 0]) & (c[:, None, 0] <= r1[None, :, 0])
                & (r0[None, :, 1] <= c[:, None, 1]) & (c[:, None, 1] <= r1[None, :, 1]))
        tested[p0:p0 + per] = cand.sum(1).to(torch.int32)
        pi, ti = torch.nonzero(cand, as_tuple=True)
        pi = pi + p0
        qx, qy, qz = q[pi, 0], q[pi, 1], q[pi, 2]
        y0, y1 = qx - t3[ti, 0], qy - t3[ti, 1]
        u = (A11[ti] * y0 - A01[ti] * y1) * s_det[ti]
        v = (-A10[ti] * y0 + A00[ti] * y1) * s_det[ti]
        suv = u + v
        ad, an = a_det[ti], a_n[ti]
        hit = (ad != 0) & (0 < u) & (u < ad) & (0 < v) & (v < ad) & (0 < suv) & (suv < ad) & (an != 0)
        alpha = nx[ti] * (t1[ti, 0] - qx) + ny[ti] * (t1[ti, 1] - qy)
        depth = t1z_an[ti] + alpha * s_n[ti]
        ge = depth >= qz * an
        n0.index_add_(0, pi, (hit & ge).long())
        n1.index_add_(0, pi, (hit & ~ge).long())
    odd0, odd1 = (n0 & 1).bool(), (n1 & 1).bool()
    return in_box & odd0 & odd1, in_box & (odd0 != odd1), tested


# ---- signed distance to a mesh (DESIGN.md "Signed distance to a mesh on the device") ---------------------------------------
def check_trunc(trunc, what="mesh_sdf"):
    """The width of the band as the float32 number the kernels take: a number >= 0, +inf for no cut-off -> float."""
    if isinstance(trunc, bool) or not isinstance(trunc, (int, float, np.integer, np.floating)) or math.isnan(float(trunc)) \
            or float(trunc) < 0:
        raise ValueError("%s: trunc must be a number >= 0 (+inf: no cut-off), got %r" % (what, trunc))
    with np.errstate(over="ignore"):
        return float(np.float32(trunc))


def signed_distance(d2, inside, trunc=float("inf")):
    """THE rule of the signed value: sdf = (inside ? -1 : +1) * min(sqrt(d2), trunc) in float64, rounded once to float32; negative
    inside, like the project's own SDF.  d2 = +inf (outside the band) gives +-trunc, a NaN d2 stays NaN."""
    t = check_trunc(trunc, "signed_distance")
    r = torch.sqrt(d2.to(torch.float64))
    m = torch.minimum(r, torch.full_like(r, t))
    return torch.where(inside.bool(), -m, m).to(torch.float32)


def _dot3(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def closest_on_triangles(p, a, b, c):
    """Barycentric weights (wa, wb, wc) of the point of triangle (a, b, c) closest to p, by Voronoi regions (Ericson, Real-Time
    Collision Detection 5.1.5): float64 (..., 3) tensors that broadcast; every operation rounded on its own, dot products summed
    from the left.  The specification of closest_on_triangle (csrc/meshquery.hpp), region by region in its order: vertex a, vertex
    b, edge ab, vertex c, edge ac, edge bc, interior."""
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = _dot3(ab, ap), _dot3(ac, ap)
    bp = p - b
    d3, d4 = _dot3(ab, bp), _dot3(ac, bp)
    cp = p - c
    d5, d6 = _dot3(ab, cp), _dot3(ac, cp)
    vc = d1 * d4 - d3 * d2
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    denom = 1.0 / ((va + vb) + vc)
    wb = vb * denom
    wc = vc * denom
    wa = (1.0 - wb) - wc
    zero, one = torch.zeros_like(wa), torch.ones_like(wa)

    def region(cond, ra, rb, rc):
        nonlocal wa, wb, wc
        wa, wb, wc = torch.where(cond, ra, wa), torch.where(cond, rb, wb), torch.where(cond, rc, wc)
    e43, e56 = d4 - d3, d5 - d6
    w = e43 / (e43 + e56)
    region((va <= 0) & (e43 >= 0) & (e56 >= 0), zero, 1.0 - w, w)
    w = d2 / (d2 - d6)
    region((vb <= 0) & (d2 >= 0) & (d6 <= 0), 1.0 - w, zero, w)
    region((d6 >= 0) & (d5 <= d6), zero, zero, one)
    v = d1 / (d1 - d3)
    region((vc <= 0) & (d1 >= 0) & (d3 <= 0), 1.0 - v, v, zero)
    region((d3 >= 0) & (d4 <= d3), zero, one, zero)
    region((d1 <= 0) & (d2 <= 0), one, zero, zero)
    return wa, wb, wc


def soup_closest(tris, points, trunc=float("inf"), chunk_pairs=1 << 21):
    """The closest triangle of the soup tris (F,3,3) float32 for every point (P,3) float32: -> d2 (P,) float64, face (P,) int32,
    closest (P,3) float64.  What hip.mesh_closest and hip.mesh_query compute, brute force: per pair the weights of
    `closest_on_triangles` in float64 on the float32 data, closest = (wa a + wb b) + wc c, d2 = |p - closest|^2 summed from the left;
    per point the lexicographic minimum of (d2, face id); a pair whose d2 is NaN (0 / 0 in a triangle without extent) is no
    candidate.  A soup with a vertex that is not finite, or a point that is not: d2 NaN, face -1, closest NaN.  No candidate at all
    (F = 0): d2 +inf, face -1, closest NaN.  With a finite trunc >= 0 (rounded to float32 first) a point with d2 > double(trunc)^2
    is outside the band and reports the same +inf, -1, NaN."""
    t = check_trunc(trunc, "soup_closest")
    if not isinstance(tris, torch.Tensor) or tris.dim() != 3 or tuple(tris.shape[1:]) != (3, 3) or tris.dtype != torch.float32:
        raise ValueError("soup_closest: tris must be an (F, 3, 3) float32 triangle soup")
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32:
        raise ValueError("soup_closest: points must be (P, 3) float32")
    if points.device != tris.device:
        raise ValueError("soup_closest: points live on %s, the mesh on %s" % (points.device, tris.device))
    f64, dev = torch.float64, tris.device
    P, F = int(points.shape[0]), int(tris.shape[0])
    inf, nan = float("inf"), float("nan")
    d2_out = torch.full((P,), inf, dtype=f64, device=dev)
    face_out = torch.full((P,), -1, dtype=torch.int32, device=dev)
    closest_out = torch.full((P, 3), nan, dtype=f64, device=dev)
    if P == 0 or F == 0:
        return d2_out, face_out, closest_out
    T, X = tris.detach().to(f64), points.detach().to(f64)
    if not bool(torch.isfinite(T).all()):
        return torch.full_like(d2_out, nan), face_out, closest_out
    a, b, c = T[None, :, 0], T[None, :, 1], T[None, :, 2]
    ids = torch.arange(F, device=dev)
    per = max(1, int(chunk_pairs) // F)
    for p0 in range(0, P, per):
        p = X[p0:p0 + per, None, :]
        wa, wb, wc = closest_on_triangles(p, a, b, c)
        cp = (wa[..., None] * a + wb[..., None] * b) + wc[..., None] * c
        dv = p - cp
        d2 = _dot3(dv, dv)
        d2 = torch.where(torch.isnan(d2), torch.full_like(d2, inf), d2)
        best = d2.min(dim=1).values
        first = torch.where((d2 == best[:, None]) & (d2 < inf), ids[None, :], F).min(dim=1).values      # F: no candidate
        found = first < F
        g = first.clamp(max=F - 1)
        d2_out[p0:p0 + per] = torch.where(found, best, torch.full_like(best, inf))
        face_out[p0:p0 + per] = torch.where(found, first, torch.full_like(first, -1)).to(torch.int32)
        picked = torch.gather(cp, 1, g[:, None, None].expand(-1, 1, 3))[:, 0]
        closest_out[p0:p0 + per] = torch.where(found[:, None], picked, torch.full_like(picked, nan))
    out = d2_out > t * t
    d2_out = torch.where(out, torch.full_like(d2_out, inf), d2_out)
    face_out = torch.where(out, torch.full_like(face_out, -1), face_out)
    closest_out = torch.where(out[:, None], torch.full_like(closest_out, nan), closest_out)
    bad = ~torch.isfinite(X).all(1)
    d2_out = torch.where(bad, torch.full_like(d2_out, nan), d2_out)
    face_out = torch.where(bad, torch.full_like(face_out, -1), face_out)
    closest_out = torch.where(bad[:, None], torch.full_like(closest_out, nan), closest_out)
    return d2_out, face_out, closest_out


def mesh_sdf(verts, faces, points, trunc=float("inf"), resolution=512, chunk_pairs=1 << 21):
    """The signed distance of points (P,3) float32 to the mesh verts (V,3) float32, faces (F,3) integer, as its parts: -> d2 (P,)
    float64, face (P,) int32, closest (P,3) float64, inside (P,) bool, ambiguous (P,) bool.  d2, face and closest are `soup_closest`
    of verts[faces] with the band `trunc`; inside and ambiguous are `mesh_contains` at `resolution`, unchanged and reported for every
    point, in the band or not.  The signed value is signed_distance(d2, inside, trunc).  The sign is the reference's parity rule: it
    is meant for watertight meshes, and `ambiguous` counts the points it could not decide.  A face id outside [0, V) raises."""
    check_contains_args(verts, faces, points, resolution, "mesh_sdf")
    if verts.dtype != torch.float32 or points.dtype != torch.float32:
        raise ValueError("mesh_sdf: verts and points must be float32")
    fc = faces.detach().long()
    if fc.numel() and not bool(((fc >= 0) & (fc < int(verts.shape[0]))).all()):
        raise ValueError("mesh_sdf: a face names a vertex outside [0, %d)" % int(verts.shape[0]))
    tris = verts.detach()[fc] if fc.numel() else verts.new_zeros((0, 3, 3))
    d2, face, closest = soup_closest(tris, points, trunc, chunk_pairs)
    inside, ambiguous, _ = mesh_contains(verts, faces, points, resolution)
    return d2, face, closest, inside, ambiguous


def check_lattice_axes(xs, ys, zs, what="mesh_sdf_grid"):
    """The three axes of a lattice: non-empty 1-D float32 tensors on one device, finite and strictly ascending (a host
    synchronisation) -> (Nx, Ny, Nz)."""
    for name, x in (("xs", xs), ("ys", ys), ("zs", zs)):
        if not isinstance(x, torch.Tensor) or x.dim() != 1 or x.dtype != torch.float32 or x.shape[0] < 1:
            raise ValueError("%s: %s must be a non-empty 1-D float32 tensor" % (what, name))
        if not bool(torch.isfinite(x).all()) or (x.shape[0] > 1 and not bool((x[1:] > x[:-1]).all())):
            raise ValueError("%s: %s must be finite and strictly ascending" % (what, name))
    if len({xs.device, ys.device, zs.device}) != 1:
        raise ValueError("%s: the axes must live on one device" % what)
    dims = (int(xs.shape[0]), int(ys.shape[0]), int(zs.shape[0]))
    if dims[0] * dims[1] * dims[2] > 2 ** 31 - 1:
        raise ValueError("%s: at most 2^31 - 1 lattice nodes" % what)
    return dims


def mesh_sdf_grid(tris, xs, ys, zs, trunc, chunk_pairs=1 << 21):
    """`soup_closest` on the nodes of the lattice xs x ys x zs (meshgrid, indexing "ij"): -> d2 (Nx,Ny,Nz) float64, face (Nx,Ny,Nz)
    int32.  The specification of arah_mesh_sdf_grid (csrc/meshsdf.hpp), which equals it bit for bit; the number of nodes in the band
    is (d2 <= double(trunc)^2 and d2 < inf).sum()."""
    dims = check_lattice_axes(xs, ys, zs)
    grid = torch.stack(torch.meshgrid(xs, ys, zs, indexing="ij"), dim=-1).reshape(-1, 3)
    d2, face, _ = soup_closest(tris, grid, trunc, chunk_pairs)
    return d2.reshape(dims), face.reshape(dims)


# ---- generalized winding numbers (DESIGN.md "Winding numbers on the device") ------------------------------------------------
WINDING_MAX_DEPTH = 7                   # three times 7 bits: the Morton key of a leaf fits 21 bits
WINDING_MAX_FACES = 1 << 28
WINDING_MAX_LEAF = 1 << 15              # faces of one leaf cell the device accepts at depth > 0 (its ranking is quadratic in a cell)
WINDING_FOUR_PI = 4.0 * math.pi
WINDING_RULES = ("parity", "winding")


def _sqrt_rn(x):
    """The correctly rounded square root of a float64 tensor on the host, as the device's: torch.sqrt on the CPU is a vectorised
    approximation that misses the last bit of about one number in a hundred."""
    return torch.from_numpy(np.sqrt(x.detach().contiguous().numpy()))


def check_rule(rule, what="mesh_contains"):
    if not isinstance(rule, str) or rule not in WINDING_RULES:
        raise ValueError("%s: rule must be 'parity' or 'winding', got %r" % (what, rule))
    return rule


def check_accuracy(accuracy, what="mesh_winding"):
    """The opening parameter of the traversal: a number >= 1, +inf for the exact sum -> float."""
    if isinstance(accuracy, bool) or not isinstance(accuracy, (int, float, np.integer, np.floating)) or math.isnan(float(accuracy)) \
            or float(accuracy) < 1:
        raise ValueError("%s: accuracy must be a number >= 1 (+inf: the exact sum), got %r" % (what, accuracy))
    return float(accuracy)


def winding_depth(n_faces):
    """THE rule of depth=None, shared with the device (wn_auto_depth): the smallest depth with 8 * 4^depth >= n_faces, at most
    WINDING_MAX_DEPTH -- a surface meets about 4^depth of the 8^depth leaf cells, so a leaf holds about eight triangles.  Chosen from
    the depth sweep of tools/mesh_winding_bench.py (deeper trees answer faster up to the cap; the build grows with the 8^depth
    cells); the constant 8 itself and the cap are not measured against alternatives."""
    d = 0
    while d < WINDING_MAX_DEPTH and (8 << (2 * d)) < int(n_faces):
        d += 1
    return d


def check_winding_depth(depth, n_faces, what="winding_tree"):
    if depth is None:
        return winding_depth(n_faces)
    if isinstance(depth, bool) or not isinstance(depth, (int, np.integer)) or not 0 <= int(depth) <= WINDING_MAX_DEPTH:
        raise ValueError("%s: depth must be None or an integer in [0, %d], got %r" % (what, WINDING_MAX_DEPTH, depth))
    return int(depth)


def solid_angle_terms(p, a, b, c):
    """The signed solid angle under which the triangle (a, b, c) is seen from p (Van Oosterom & Strackee 1983): float64 (..., 3)
    tensors that broadcast.  With a, b, c the corners minus p: num = a . (b x c), the cross product first and the dot product summed
    from the left; den = (((|a| |b|) |c| + (a.b) |c|) + (b.c) |a|) + (c.a) |b|; the term is 2 atan2(num, den), and 0 where
    num == 0 -- a point in the plane of the face, on the face or at a corner sees it under no angle.  Every operation is rounded on
    its own; only atan2 is a library function.  Positive when the corners run counter-clockwise seen from the far side of p."""
    a, b, c = a - p, b - p, c - p
    crx = b[..., 1] * c[..., 2] - b[..., 2] * c[..., 1]
    cry = b[..., 2] * c[..., 0] - b[..., 0] * c[..., 2]
    crz = b[..., 0] * c[..., 1] - b[..., 1] * c[..., 0]
    num = (a[..., 0] * crx + a[..., 1] * cry) + a[..., 2] * crz
    la, lb, lc = _sqrt_rn(_dot3(a, a)), _sqrt_rn(_dot3(b, b)), _sqrt_rn(_dot3(c, c))
    den = (((la * lb) * lc + _dot3(a, b) * lc) + _dot3(b, c) * la) + _dot3(c, a) * lb
    term = 2.0 * torch.atan2(num, den)
    return torch.where(num == 0, torch.zeros_like(term), term)


def winding_orient(verts, faces):
    """+1 or -1: the sign of the mesh's signed volume, sum det(v0, v1, v2) / 6 in float64; +1 where that is 0 or NaN.  det = v0 .
    (v1 x v2) as in `solid_angle_terms`.  The order of the sum (k_wn_box): 256 partial sums, number t taking the faces t, t + 256,
    ... in ascending order, then p[t] += p[t + s] for s = 128, 64, ..., 1.  -> (orient int, volume float)."""
    T = verts.detach().to(torch.float64)[faces.detach().long()].cpu()
    F = int(T.shape[0])
    if F == 0:
        return 1, 0.0
    v0, v1, v2 = T[:, 0], T[:, 1], T[:, 2]
    crx = v1[:, 1] * v2[:, 2] - v1[:, 2] * v2[:, 1]
    cry = v1[:, 2] * v2[:, 0] - v1[:, 0] * v2[:, 2]
    crz = v1[:, 0] * v2[:, 1] - v1[:, 1] * v2[:, 0]
    det = ((v0[:, 0] * crx + v0[:, 1] * cry) + v0[:, 2] * crz).numpy()
    rows = (F + 255) // 256
    padded = np.zeros(rows * 256, dtype=np.float64)
    padded[:F] = det
    p = np.add.accumulate(padded.reshape(rows, 256), axis=0)[-1].copy()      # strictly sequential down every column
    s = 128
    while s >= 1:
        p[:s] = p[:s] + p[s:2 * s]
        s //= 2
    volume = float(p[0]) / 6.0
    return (-1 if volume < 0 else 1), volume


def _morton3(ix, iy, iz, depth):
    """Bit b of ix, iy, iz -> bits 3b + 2, 3b + 1, 3b of the key."""
    key = np.zeros_like(ix)
    for b in range(depth):
        key |= (((ix >> b) & 1) << (3 * b + 2)) | (((iy >> b) & 1) << (3 * b + 1)) | (((iz >> b) & 1) << (3 * b))
    return key


def _unmorton3(key, depth):
    out = [np.zeros_like(key), np.zeros_like(key), np.zeros_like(key)]
    for b in range(depth):
        for a in range(3):
            out[a] |= ((key >> (3 * b + 2 - a)) & 1) << b
    return out


class WindingTree:
    """The cluster tree of `winding_tree`, on the host.  order (F,) int32: the triangles' ids in list order; tris (F,3,3) float32:
    their corners in list order; first, count, level, skip (N,) int32; nvec (N,3), centroid (N,3), radius (N,), area (N,) float64;
    lo (3,) float64 and side: the cube; depth, n_faces, orient (+1 / -1), volume, valid (False: a used vertex is not finite, every
    winding number is NaN)."""

    FIELDS = ("order", "tris", "first", "count", "level", "skip", "nvec", "centroid", "radius", "area")

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def n_nodes(self):
        return int(self.first.shape[0])


def winding_tree(verts, faces, depth=None):
    """The cluster tree of the fast winding number (Barill et al. 2018) of the mesh verts (V,3) floating point, faces (F,3) integer
    -> WindingTree.  The specification of arah_winding_index_count / _fill (csrc/meshwinding.hpp): the integer tables are equal and
    the float tables equal bit for bit.  float64 on the vertices as given (the device takes them as float32), every operation rounded
    on its own.

    The cube: lo = the minimum over the vertices some face uses, side = the largest of the three extents.  Triangle (a, b, c) has
    the centroid g = ((a + b) + c) / 3 and lies in the leaf cell i = (int) clamp((g - lo) * (2^depth / side), 0, 2^depth - 1) per
    axis (a NaN counts as 0), whose key interleaves the bits of (ix, iy, iz), x highest.  The list orders the triangles by (key, face
    id).  Every non-empty cell of every level 0 .. depth -- the key shifted right by 3 (depth - level) -- is a node; the nodes are
    numbered in depth-first preorder (by first, then level), skip is the number of the next node outside the subtree (N after the
    last).  depth=None is `winding_depth`; depth=0 makes the root the one leaf, the list the face order.

    Per triangle n = ((b - a) x (c - a)) / 2 -- 0.5 times each component of the cross product --, area = |n| summed from the left,
    and area * g.  A leaf sums n, area and area * g over its members in list order, starting from 0; an inner node sums its
    children's sums in child order, starting from 0.  centroid = sum(area g) / sum(area) where the summed area is > 0, else the
    cell's centre lo + (i + 0.5) * (side / 2^level).  radius = sqrt of the largest |corner - centroid|^2 (summed from the left) over
    the corners of the member triangles.  A face id outside [0, V) raises.  The device refuses a mesh that puts more than
    WINDING_MAX_LEAF faces into one leaf cell at depth > 0 (hip.winding_index raises); this specification has no such limit."""
    if not isinstance(verts, torch.Tensor) or verts.dim() != 2 or verts.shape[1] != 3 or not verts.dtype.is_floating_point:
        raise ValueError("winding_tree: verts must be a floating-point (V, 3) tensor")
    if (not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype.is_floating_point
            or faces.dtype == torch.bool):
        raise ValueError("winding_tree: faces must be an integer (F, 3) tensor")
    F, V = int(faces.shape[0]), int(verts.shape[0])
    if F > WINDING_MAX_FACES:
        raise ValueError("winding_tree: at most 2^28 faces")
    depth = check_winding_depth(depth, F)
    fc = faces.detach().long().cpu()
    if F and not bool(((fc >= 0) & (fc < V)).all()):
        raise ValueError("winding_tree: a face names a vertex outside [0, %d)" % V)
    f64, i32 = torch.float64, torch.int32
    v32 = verts.detach().cpu()
    T = v32.to(f64)[fc] if F else torch.zeros((0, 3, 3), dtype=f64)
    orient, volume = winding_orient(v32, fc)
    empty_i = torch.zeros(0, dtype=i32)
    if F == 0:
        return WindingTree(order=empty_i, tris=torch.zeros((0, 3, 3), dtype=torch.float32), first=empty_i, count=empty_i.clone(),
                           level=empty_i.clone(), skip=empty_i.clone(), nvec=torch.zeros((0, 3), dtype=f64),
                           centroid=torch.zeros((0, 3), dtype=f64), radius=torch.zeros(0, dtype=f64), area=torch.zeros(0, dtype=f64),
                           lo=torch.zeros(3, dtype=f64), side=0.0, depth=depth, n_faces=0, orient=1, volume=0.0, valid=True)
    valid = bool(torch.isfinite(T).all())
    flat = T.reshape(-1, 3)
    fin = torch.where(torch.isfinite(flat), flat, torch.full_like(flat, float("nan")))
    lo = torch.from_numpy(np.fmin.reduce(fin.numpy(), axis=0))
    hi = torch.from_numpy(np.fmax.reduce(fin.numpy(), axis=0))
    side = (hi - lo).max()
    a, b, c = T[:, 0], T[:, 1], T[:, 2]
    g = ((a + b) + c) / 3.0
    n_leaf = 1 << depth
    inv = torch.full((), float(n_leaf), dtype=f64) / side
    q = torch.nan_to_num((g - lo) * inv, nan=0.0, posinf=float(n_leaf - 1), neginf=0.0).clamp(0.0, float(n_leaf - 1))
    cell = q.trunc().long().numpy()
    key = _morton3(cell[:, 0], cell[:, 1], cell[:, 2], depth)
    order = np.argsort((key << 32) | np.arange(F, dtype=np.int64), kind="stable")
    sk = key[order]
    # the level at which a triangle of the list starts a node: 0 for the first, depth + 1 where the key repeats
    x = sk[1:] ^ sk[:-1]
    hb = np.where(x > 0, np.floor(np.log2(np.maximum(x, 1))).astype(np.int64), -1)
    h = np.concatenate([[0], np.where(x > 0, depth - hb // 3, depth + 1)]).astype(np.int64)
    prefix = np.concatenate([[0], np.cumsum(depth + 1 - h)]).astype(np.int64)
    N = int(prefix[-1])
    first, count = np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int64)
    level, skip = np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int64)
    cells = np.zeros((N, 3), dtype=np.int64)
    for l in range(depth + 1):
        s = 3 * (depth - l)
        i = np.flatnonzero(h <= l)
        node = prefix[i] + l - h[i]
        end = np.searchsorted(sk, ((sk[i] >> s) + 1) << s, side="left")
        first[node], count[node], level[node], skip[node] = i, end - i, l, prefix[end]
        cx, cy, cz = _unmorton3(sk[i] >> s, l)
        cells[node] = np.stack([cx, cy, cz], axis=1)
    # per triangle, in list order
    to = torch.from_numpy(order)
    a, b, c, g = a[to], b[to], c[to], g[to]
    e1, e2 = b - a, c - a
    nv = torch.stack([0.5 * (e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]), 0.5 * (e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]),
                      0.5 * (e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0])], dim=1)
    ar = _sqrt_rn(_dot3(nv, nv))
    val = torch.cat([nv, ar[:, None], ar[:, None] * g], dim=1)                   # (F, 7)
    sums = torch.zeros((N, 7), dtype=f64)
    leaves = np.flatnonzero(level == depth)
    lf, lc = first[leaves], count[leaves]
    for j in range(int(lc.max())):                                              # list order inside every leaf
        m = lc > j
        rows = torch.from_numpy(leaves[m])
        sums[rows] = sums[rows] + val[torch.from_numpy(lf[m] + j)]
    for l in range(depth - 1, -1, -1):                                          # child order inside every inner node
        nodes = np.flatnonzero(level == l)
        child = nodes + 1
        for _ in range(8):
            m = child < skip[nodes]
            if not m.any():
                break
            rows, ch = torch.from_numpy(nodes[m]), torch.from_numpy(child[m])
            sums[rows] = sums[rows] + sums[ch]
            child = np.where(m, skip[np.minimum(child, N - 1)], child)
    lvl = torch.from_numpy(level)
    width = torch.full((N,), 1.0, dtype=f64) * side / torch.pow(torch.full((N,), 2.0, dtype=f64), lvl.to(f64))
    centre = lo[None, :] + (torch.from_numpy(cells).to(f64) + 0.5) * width[:, None]
    area = sums[:, 3]
    centroid = torch.where((area > 0)[:, None], sums[:, 4:7] / area[:, None], centre)
    r2 = torch.zeros(N, dtype=f64)
    corners = torch.stack([a, b, c], dim=1)                                      # (F,3,3) in list order
    for l in range(depth + 1):
        nodes = np.flatnonzero(level == l)
        owner = torch.from_numpy(np.repeat(nodes, count[nodes]))                  # the node of every triangle of the list at level l
        d = corners - centroid[owner][:, None, :]
        d2 = _dot3(d, d).amax(1)
        r2.scatter_reduce_(0, owner, d2, reduce="amax", include_self=True)
    return WindingTree(order=to.to(i32), tris=v32.to(torch.float32)[fc][to].contiguous(), first=torch.from_numpy(first).to(i32),
                       count=torch.from_numpy(count).to(i32), level=lvl.to(i32), skip=torch.from_numpy(skip).to(i32),
                       nvec=sums[:, 0:3].contiguous(), centroid=centroid.contiguous(), radius=_sqrt_rn(r2), area=area.contiguous(),
                       lo=lo, side=float(side), depth=depth, n_faces=F, orient=orient, volume=volume, valid=valid)


def mesh_winding(tree, points, accuracy=3.0, chunk=256):
    """The generalized winding number of points (P,3) float32 or float64 on the host against a WindingTree -> w (P,) float64,
    n_exact (P,) int32 (triangles summed exactly), n_far (P,) int32 (clusters taken as dipoles).  The specification of
    arah_mesh_winding: the same near / far decisions, bit-equal dipole terms, exact terms that differ by atan2's last bits.

    One accumulator per point, in solid angle, starting from 0.  The walk starts at node 0 and ends at node N.  At a node with
    centroid c, radius r and summed area vector n, d = c - p and d2 = |d|^2 summed from the left: if d2 > accuracy^2 * (r * r) the
    node adds (d . n) / (d2 * sqrt(d2)) and the walk goes to skip; else a leaf adds `solid_angle_terms` of its triangles one by one
    in list order and the walk goes to skip; else the walk goes to the next node.  w = accumulator / (4 pi).  accuracy = +inf takes
    no node as far (inf * 0 is NaN, and no number exceeds a NaN): the exact sum.  A tree that is not valid answers NaN, 0, 0; a NaN
    in a point takes every node as near and ends as NaN.  `chunk` bounds the temporaries; the result does not depend on it."""
    acc = check_accuracy(accuracy, "mesh_winding")
    if not isinstance(tree, WindingTree):
        raise ValueError("mesh_winding: tree must come from winding_tree")
    if (not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3
            or points.dtype not in (torch.float32, torch.float64)):
        raise ValueError("mesh_winding: points must be (P, 3) float32 or float64")
    f64 = torch.float64
    X = points.detach().cpu().to(f64)
    P, N = int(X.shape[0]), tree.n_nodes
    total = torch.zeros(P, dtype=f64)
    n_exact, n_far = torch.zeros(P, dtype=torch.int32), torch.zeros(P, dtype=torch.int32)
    if not tree.valid:
        return torch.full((P,), float("nan"), dtype=f64), n_exact, n_far
    acc2 = acc * acc
    T = tree.tris.to(f64)
    first, count, level, skip = (t.tolist() for t in (tree.first, tree.count, tree.level, tree.skip))
    at = torch.zeros(P, dtype=torch.int64)
    for n in range(N):
        here = torch.nonzero(at == n)[:, 0]
        if here.numel() == 0:
            continue
        p = X[here]
        d = tree.centroid[n][None, :] - p
        d2 = _dot3(d, d)
        r = tree.radius[n]
        far = d2 > acc2 * (r * r)
        fi = here[far]
        if fi.numel():
            df, d2f = d[far], d2[far]
            total[fi] = total[fi] + _dot3(df, tree.nvec[n][None, :].expand_as(df)) / (d2f * _sqrt_rn(d2f))
            n_far[fi] += 1
        if level[n] == tree.depth:
            ni = here[~far]
            if ni.numel():
                pn = X[ni][:, None, :]
                run = total[ni]
                for t0 in range(first[n], first[n] + count[n], chunk):
                    tt = T[t0:min(t0 + chunk, first[n] + count[n])]
                    terms = solid_angle_terms(pn, tt[None, :, 0], tt[None, :, 1], tt[None, :, 2])
                    for j in range(int(terms.shape[1])):
                        run = run + terms[:, j]
                total[ni] = run
                n_exact[ni] += count[n]
            at[here] = skip[n]
        else:
            at[here] = torch.where(far, torch.full_like(here, skip[n]), torch.full_like(here, n + 1))
    return total / WINDING_FOUR_PI, n_exact, n_far


def winding_inside(w, orient):
    """THE rule of the winding number's inside test: orient * w >= 0.5; a NaN is outside."""
    return (float(orient) * w) >= 0.5


def face_normals(tri):
    """Unit right-hand normals of a triangle soup (F,3,3) (pytorch3d Meshes.faces_normals_packed)."""
    n = torch.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], dim=1)
    return n / n.norm(dim=1, keepdim=True).clamp_min(1e-20)


def project_opencv(pts, cam_rot, cam_trans, K):
    """World points (...,3) -> (u, v, depth) with x_cam = R x + t, u = fx X/Z + cx (cameras_from_opencv_projection)."""
    xc = pts @ cam_rot.t() + cam_trans
    z = xc[..., 2]
    u = K[0, 0] * xc[..., 0] / z + K[0, 2]
    v = K[1, 1] * xc[..., 1] / z + K[1, 2]
    return torch.stack([u, v, z], dim=-1)


_LOOKAT = {}   # (device, azimuth, distance) -> (camera position (3,), view axes as columns (3,3)) on the device


def _lookat(device, azim_deg, dist):
    """look_at_view_transform(dist, 0, azim): the camera position and the matrix whose columns are the view axes.  Built once
    per device and view: a tensor made from Python numbers is a blocking host -> device copy, which waits for everything the
    stream has queued -- inside a frame that would be the whole render in front of the mesh branch."""
    key = (device, float(azim_deg), float(dist))
    if key not in _LOOKAT:
        a = math.radians(azim_deg)
        cam = torch.tensor([dist * math.sin(a), 0.0, dist * math.cos(a)])
        z_axis = -cam / cam.norm()
        up = torch.tensor([0.0, 1.0, 0.0])
        x_axis = torch.cross(up, z_axis, dim=0)
        x_axis = x_axis / x_axis.norm()
        y_axis = torch.cross(z_axis, x_axis, dim=0)
        R = torch.stack([x_axis, y_axis, z_axis], dim=1)          # columns = view axes
        _LOOKAT[key] = (cam.to(device), R.to(device))
    return _LOOKAT[key]


def project_lookat(pts, azim_deg, size, dist=2.0, fov_deg=60.0):
    """look_at_view_transform(dist, elev 0, azim) + FoVPerspectiveCameras(fov 60): canonical points -> (u, v, depth).
    pytorch3d's view space has +X left, +Y up, +Z into the screen; NDC (1,1) is the top-left pixel corner."""
    cam, R = _lookat(pts.device, azim_deg, dist)
    xv = (pts - cam) @ R
    f = 1.0 / math.tan(math.radians(fov_deg) / 2.0)
    z = xv[..., 2]
    u = (1.0 - f * xv[..., 0] / z) * size / 2.0
    v = (1.0 - f * xv[..., 1] / z) * size / 2.0
    return torch.stack([u, v, z], dim=-1)


def normal_image(pix_to_face, normals, background):
    """normals (F,3) gathered per pixel, `background` elsewhere, mapped to [0,1] like models/__init__.py:247,278.
    (A gather and a select: boolean-mask indexing would cost a device -> host round trip for the number of pixels.)"""
    fg = (pix_to_face >= 0).unsqueeze(-1)
    img = torch.where(fg, normals[pix_to_face.clamp_min(0)], torch.full((), float(background), device=normals.device))
    return ((img + 1.0) / 2.0).clip(0.0, 1.0).unsqueeze(0)


# Triangle capacity of the device-side extraction per device, and the counts of earlier calls on their way to the host
# (asynchronous copies into pinned memory: nothing here ever waits for the GPU).  A count that turns out to have exceeded
# the capacity raises it for the calls that follow and is reported: that call's mesh was truncated.
_MC_STATE = {}
MC_DEFAULT_CAP = 1 << 20


def _mc_state(dev):
    st = _MC_STATE.get(dev)
    if st is None:
        st = _MC_STATE[dev] = {"cap": MC_DEFAULT_CAP, "pending": [], "free": [], "overflowed": 0, "last_count": None}
    return st


def _mc_poll(st, wait=False):
    import warnings
    keep = []
    for ev, host, cap in st["pending"]:
        if wait:
            ev.synchronize()
        if ev.query():
            n = int(host[0])
            st["last_count"] = n
            st["free"].append((ev, host))
            if n <= cap and not st["overflowed"]:
                # every frame pushes the whole buffer through un-normalisation, skinning, projection and three rasterisations:
                # size it for the level set this subject actually has (twice the last count, a power of two, never above the
                # default; one overflow pins the raised capacity for good)
                st["cap"] = min(MC_DEFAULT_CAP, max(1 << 16, 1 << int(math.ceil(math.log2(2.0 * max(n, 1))))))
            if n > cap:
                st["overflowed"] += 1
                st["cap"] = max(st["cap"], 1 << int(math.ceil(math.log2(1.5 * n))))
                warnings.warn("canonical mesh: the level set has %d triangles, the device buffer held %d -- that frame's mesh was "
                              "truncated; capacity raised to %d for the following frames" % (n, cap, st["cap"]))
        else:
            keep.append((ev, host, cap))
    st["pending"] = keep


def mesh_counts(device, wait=True):
    """(triangles of the last finished extraction on `device`, number of truncated extractions so far); wait=True drains the
    outstanding count copies first (tests, end of a sequence)."""
    st = _mc_state(torch.device(device))
    _mc_poll(st, wait=wait)
    return st["last_count"], st["overflowed"]


def canonical_mesh_outputs(frame, ws, inputs, rasterize_fn=None, n_side=256, image_size=512, tri=None, want_tri=True):
    """The three normal maps of the gen_cano_mesh branch + the canonical triangle soup (normalised coordinates).
    frame: packed hip.Frame of the current pose; inputs: the model's input dict (coord_min/max, center, trans,
    cam_rot, cam_trans, intrinsics).  tri: a triangle soup to use instead of meshing the SDF (fixture F18 injects the mesh
    the reference's own branch was run on).  want_tri=False (the model entry): the soup is not returned and the call makes
    no device -> host round trip at all -- the mesh lives in a fixed-capacity buffer whose tail is degenerate triangles, its
    size stays on the device (hip.marching_cubes, hip.skin_lbs_counted); want_tri=True trims the soup to its size, which
    waits for the GPU."""
    from . import hip
    rasterize_fn = rasterize_fn or hip.rasterize
    with torch.no_grad():
        tri, posed, n_dev = skinned_mesh(frame, ws, inputs, n_side, tri)
        F = tri.shape[0]
        cam_rot, cam_trans, K = inputs["cam_rot"][0], inputs["cam_trans"][0], inputs["intrinsics"][0]
        p2f = rasterize_fn(project_opencv(posed, cam_rot, cam_trans, K), image_size, image_size)
        n_posed = -face_normals(posed)                                                   # models/__init__.py:243
        out = {"output_normal": normal_image(p2f, n_posed @ cam_rot.t(), -1.0)}
        n_cano = face_normals(tri)                                                       # un-negated, :274
        for key, azim in (("normal_cano_front", 0.0), ("normal_cano_back", 180.0)):
            p2f = rasterize_fn(project_lookat(tri, azim, image_size), image_size, image_size, z_near=1.0)
            out[key] = normal_image(p2f, n_cano, 0.0)
        if not want_tri:
            return out, None
        if n_dev is not None:
            tri = tri[:min(int(n_dev.item()), F)]
    return out, tri


def skinned_mesh(frame, ws, inputs, n_side=256, tri=None, cap=None):
    """The canonical level set and its forward-skinned image, the reference's points_bar mesh (models/__init__.py:209-227):
    -> (tri (F,3,3) in [-1,1]^3 normalised canonical, posed (F,3,3) world metres, n_dev (1,) int32 device count of the level set or
    None when `tri` was given).  The soup lives in a fixed-capacity buffer whose tail is degenerate triangles (zeros in `tri`,
    the translation in `posed`); no host round trip.  cap=None: the gen_cano_mesh branch's adaptive capacity (and its overflow
    bookkeeping); an explicit cap leaves that state alone, the caller compares n_dev with it."""
    from . import hip, training
    with torch.no_grad():
        n_dev = None
        if tri is None:
            sdf = canonical_lattice(frame, ws, n_side)
            if cap is not None:
                tri, n_dev = hip.marching_cubes(sdf, 0.0, cap)
            else:
                st = _mc_state(sdf.device)
                _mc_poll(st)
                tri, n_dev = hip.marching_cubes(sdf, 0.0, st["cap"])                     # (cap,3,3) in [-1,1]^3, zero tail
                ev, host = st["free"].pop() if st["free"] else (torch.cuda.Event(), torch.empty(1, dtype=torch.int32).pin_memory())
                host.copy_(n_dev, non_blocking=True)
                ev.record()
                st["pending"].append((ev, host, st["cap"]))
        F = tri.shape[0]
        cmin, cmax, center = inputs["coord_min"][:1], inputs["coord_max"][:1], inputs["center"][:1]
        x_hat = training.unnormalize_canonical_points(tri.reshape(1, -1, 3), cmin, cmax, center)[0]
        if n_dev is None:
            _, x_bar, _ = hip.skin_lbs(frame, ws, x_hat)
        else:
            x_bar = hip.skin_lbs_counted(frame, ws, x_hat, n_dev, per_item=3)            # zero beyond the mesh: degenerate
        posed = (x_bar + inputs["trans"].reshape(1, 3)).reshape(F, 3, 3)
    return tri, posed, n_dev


def canonical_lattice(frame, ws, n_side=256):
    """The canonical SDF lattice the mesh branch extracts from: only where the level set can pass (csrc/tier.hpp: same
    triangles as the full lattice, ~6 % of its 16.8 M evaluations); ARAH_MESH_BAND=0 or n_side < 33: every lattice point, like
    sdf_meshing.py:44-57."""
    from . import hip
    if n_side >= 33 and os.environ.get("ARAH_MESH_BAND", "1") != "0":
        return hip.sdf_grid_band(frame, ws, n_side)[0]
    return hip.sdf_grid(frame, ws, n_side)


def skinned_indexed_mesh(frame, ws, inputs, n_side=256, vert_cap=MC_DEFAULT_VERT_CAP, face_cap=None):
    """`skinned_mesh` as an indexed mesh: the canonical level set's V vertices are skinned, not its 3 F corners.  -> (verts
    (vert_cap,3) normalised canonical, posed (vert_cap,3) world metres, faces (face_cap,3) int32, counts (2,) int32 on the
    device).  Rows beyond the counts: zeros in verts and faces, the translation in posed.  No host round trip."""
    from . import hip, training
    with torch.no_grad():
        sdf = canonical_lattice(frame, ws, n_side)
        verts, faces, counts = hip.marching_cubes_indexed(sdf, 0.0, vert_cap, MC_DEFAULT_CAP if face_cap is None else face_cap)
        cmin, cmax, center = inputs["coord_min"][:1], inputs["coord_max"][:1], inputs["center"][:1]
        x_hat = training.unnormalize_canonical_points(verts.reshape(1, -1, 3), cmin, cmax, center)[0]
        x_bar = hip.skin_lbs_counted(frame, ws, x_hat, counts[:1], per_item=1)
        posed = x_bar + inputs["trans"].reshape(1, 3)
    return verts, posed, faces, counts
