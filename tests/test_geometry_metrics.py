"""Geometry scores of a mesh against a ground-truth mesh (DESIGN.md "Geometry metrics on the device"): the float64 numpy
restatement of the definition and its closed-form checks, geometry.load_mesh, and on the GPU the indexed exact closest-triangle
query (hip.mesh_index / hip.mesh_closest) held to hip.mesh_query bit for bit, geometry.mesh_metrics held to the restatement,
MetaAvatarRender.geometry_metrics and `validate --geometry`."""
import json
import os
import struct

import numpy as np
import pytest
import torch

from conftest import get_model, golden
from oracle.mesh_oracle import point_mesh_np

gpu = pytest.mark.gpu
KEYS = ("accuracy", "completeness", "chamfer_l1", "chamfer_l2", "normal_consistency", "hausdorff_ab", "hausdorff_ba")
F32 = 2.0 ** -24   # relative rounding of a float32 coordinate


# ---------------------------------------------------------------------------------------------------- the restatement
def kept_faces_np(tris):
    """Faces whose float64 cross product is not exactly the zero vector."""
    t = np.asarray(tris, np.float32).astype(np.float64)
    return (np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]) != 0).any(-1)


def face_normals_np(tris):
    t = np.asarray(tris, np.float32).astype(np.float64)
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    return n / np.sqrt((n * n).sum(-1))[:, None]


def brute_closest(tris, pts):
    """(d2, face) by the oracle the existing suite pins: every triangle for every point, lowest index on ties."""
    tris = np.asarray(tris, np.float32)
    d2, face, _, _ = point_mesh_np(tris.reshape(-1, 3), np.arange(tris.shape[0] * 3).reshape(-1, 3), np.asarray(pts, np.float32))
    return d2, face


def restate_per_sample(tris_x, pts_x, face_x, tris_y, closest=brute_closest):
    """Per sample of X (points pts_x on faces face_x) against Y: distance d and normal term c."""
    d2, g = closest(tris_y, pts_x)
    nx, ny = face_normals_np(tris_x)[np.asarray(face_x)], face_normals_np(tris_y)[np.asarray(g)]
    return np.sqrt(d2), d2, np.abs((nx * ny).sum(-1))


def restate_metrics(tris_a, pts_a, face_a, tris_b, pts_b, face_b, closest=brute_closest):
    """The definition, in float64 numpy, on GIVEN samples; both meshes without their dropped faces."""
    d_ab, d2_ab, c_ab = restate_per_sample(tris_a, pts_a, face_a, tris_b, closest)
    d_ba, d2_ba, c_ba = restate_per_sample(tris_b, pts_b, face_b, tris_a, closest)
    return {"accuracy": d_ab.mean(), "completeness": d_ba.mean(), "chamfer_l1": 0.5 * (d_ab.mean() + d_ba.mean()),
            "chamfer_l2": 0.5 * (d2_ab.mean() + d2_ba.mean()), "normal_consistency": 0.5 * (c_ab.mean() + c_ba.mean()),
            "hausdorff_ab": d_ab.max(), "hausdorff_ba": d_ba.max(), "n_a": len(d_ab), "n_b": len(d_ba)}


def sample_np(tris, n, rng, faces=None):
    """Area-weighted samples (float32 points, their faces); `faces`: draw from these faces only."""
    t = np.asarray(tris, np.float32).astype(np.float64)
    area = 0.5 * np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=-1)
    if faces is not None:
        w = np.zeros_like(area)
        w[faces] = area[faces]
        area = w
    fi = rng.choice(len(t), n, p=area / area.sum())
    r = rng.rand(n, 2)
    flip = r.sum(1) > 1
    r[flip] = 1 - r[flip]
    p = t[fi, 0] + r[:, :1] * (t[fi, 1] - t[fi, 0]) + r[:, 1:] * (t[fi, 2] - t[fi, 0])
    return p.astype(np.float32), fi


def icosphere(level, radius=1.0, centre=(0.0, 0.0, 0.0)):
    g = (1 + 5 ** 0.5) / 2
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1),
         (-g, 0, -1), (-g, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                w = v[i] + v[j]
                v.append(w / np.linalg.norm(w))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    verts = (np.array(v) * radius + np.array(centre)).astype(np.float32)
    return verts[np.array(f)]   # (F,3,3) float32


def sphere_bracket(t1, r1, t2, r2):
    """[r2 cos(phi) - r1, r2 - r1 cos(phi)] for two concentric icospheres, phi the largest angular radius of a face of either
    (from the meshes, float64), widened by the float32 rounding of the vertices."""
    cos_phi = 1.0
    for t, r in ((t1, r1), (t2, r2)):
        n = face_normals_np(t)
        cos_phi = min(cos_phi, float(np.abs((n * t[:, 0].astype(np.float64)).sum(-1)).min()) / r)
    slack = 8 * F32 * r2
    return r2 * cos_phi - r1 - slack, r2 - r1 * cos_phi + slack


def flat_patch(n=8, half=1.0):
    """An n x n grid of quads in the plane z = 0 over [-half, half]^2 (dyadic coordinates), two triangles each."""
    xs = np.linspace(-half, half, n + 1)
    tris = []
    for i in range(n):
        for j in range(n):
            p00, p10, p01, p11 = (xs[i], xs[j], 0), (xs[i + 1], xs[j], 0), (xs[i], xs[j + 1], 0), (xs[i + 1], xs[j + 1], 0)
            tris += [(p00, p10, p11), (p00, p11, p01)]
    return np.array(tris, np.float32)


# ---------------------------------------------------------------------------------------------------------- CPU tests
# The four test_restatement_* tests check the RESTATEMENT above (the yardstick the GPU tests hold the feature to) against
# closed forms, as the feature's issue asks; they use nothing of the feature and so pass without it.  Every other test in this
# file needs the feature.
def test_restatement_mesh_against_itself():
    tris = icosphere(2, 0.75, (0.25, -0.5, 1.0))
    rng = np.random.RandomState(0)
    p, f = sample_np(tris, 300, rng)
    q, g = sample_np(tris, 300, rng)
    r = restate_metrics(tris, p, f, tris, q, g)
    # a float32 sample is its face's point rounded per coordinate (three roundings of values <= the largest coordinate)
    tol = np.sqrt(3) * 4 * F32 * np.abs(tris).max()
    assert r["hausdorff_ab"] <= tol and r["hausdorff_ba"] <= tol and r["chamfer_l1"] <= tol
    assert abs(r["normal_consistency"] - 1.0) <= 1e-12
    assert r["n_a"] == r["n_b"] == 300


def test_restatement_translated_copy_of_a_flat_patch():
    patch = flat_patch()
    mesh = np.concatenate([patch, icosphere(1, 0.5, (0.0, 0.0, 3.0))])
    t = 0.0625
    moved = (mesh + np.array([0, 0, t], np.float32)).astype(np.float32)
    rng = np.random.RandomState(1)
    p, f = sample_np(mesh, 400, rng, faces=np.arange(len(patch)))
    inner = (np.abs(p[:, :2]) <= 1.0 - 2 * t).all(1)     # the point above it is still on the copy's patch
    p, f = p[inner], f[inner]
    assert len(p) > 200
    d, _, c = restate_per_sample(mesh, p, f, moved)
    assert np.abs(d - t).max() <= 1e-12 and np.abs(c - 1.0).max() <= 1e-12
    d, _, c = restate_per_sample(moved, p + np.array([0, 0, t], np.float32), f, mesh)
    assert np.abs(d - t).max() <= 1e-12 and np.abs(c - 1.0).max() <= 1e-12


def test_restatement_concentric_icospheres():
    r1, r2 = 0.8, 1.0
    a, b = icosphere(2, r1), icosphere(3, r2)
    lo, hi = sphere_bracket(a, r1, b, r2)
    assert 0 < lo < r2 - r1 < hi
    rng = np.random.RandomState(2)
    p, f = sample_np(a, 300, rng)
    q, g = sample_np(b, 300, rng)
    d_ab, _, c_ab = restate_per_sample(a, p, f, b)
    d_ba, _, c_ba = restate_per_sample(b, q, g, a)
    assert lo <= d_ab.min() and d_ab.max() <= hi and lo <= d_ba.min() and d_ba.max() <= hi
    assert c_ab.min() > 0.9 and c_ba.min() > 0.9
    r = restate_metrics(a, p, f, b, q, g)
    assert lo <= r["accuracy"] <= hi and lo <= r["completeness"] <= hi and r["chamfer_l1"] == 0.5 * (r["accuracy"] + r["completeness"])
    assert lo * lo <= r["chamfer_l2"] <= hi * hi


def test_restatement_drops_exactly_degenerate_faces():
    tris = icosphere(1)
    bad = tris.copy()
    bad[3, 1] = bad[3, 0]                               # two corners equal
    bad[7] = np.outer([0, 1, 2], [0.5, 0.25, 0.125]).astype(np.float32)   # three corners on a line (dyadic: exactly)
    keep = kept_faces_np(bad)
    assert keep.sum() == len(tris) - 2 and not keep[3] and not keep[7]


def _write_ply(path, verts, faces, binary, extra_vertex_props=False, quad=False):
    verts, faces = np.asarray(verts, np.float32), np.asarray(faces)
    head = ["ply", "format %s 1.0" % ("binary_little_endian" if binary else "ascii"), "comment written by the test",
            "element vertex %d" % len(verts), "property float x", "property float y", "property float z"]
    if extra_vertex_props:
        head += ["property uchar red", "property double quality"]
    head += ["element face %d" % len(faces), "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        for k, v in enumerate(verts):
            if binary:
                f.write(struct.pack("<3f", *v) + (struct.pack("<Bd", k % 256, 0.5 * k) if extra_vertex_props else b""))
            else:
                f.write((" ".join(repr(float(x)) for x in v) + (" %d %r" % (k % 256, 0.5 * k) if extra_vertex_props else "")
                         + "\n").encode("ascii"))
        for k, face in enumerate(faces):
            row = list(face) + ([int(face[0])] if quad and k == 1 else [])
            if binary:
                f.write(struct.pack("<B%di" % len(row), len(row), *row))
            else:
                f.write((" ".join(str(int(x)) for x in [len(row)] + row) + "\n").encode("ascii"))


def test_load_mesh_round_trips_and_rejections(tmp_path):
    from arah_release_amd import geometry
    tris = icosphere(1, 0.5, (0.1, 0.2, 0.3))
    verts, inv = np.unique(tris.reshape(-1, 3), axis=0, return_inverse=True)
    faces = inv.reshape(-1, 3)
    np.savez(tmp_path / "m.npz", vertices=verts, faces=faces)
    cases = [tmp_path / "m.npz"]
    for binary in (False, True):
        for extra in (False, True):
            p = tmp_path / ("m_%d_%d.ply" % (binary, extra))
            _write_ply(p, verts, faces, binary, extra_vertex_props=extra)
            cases.append(p)
    for p in cases:
        v, f = geometry.load_mesh(p)
        assert v.dtype == torch.float32 and f.dtype == torch.int64
        np.testing.assert_array_equal(v.numpy(), verts)
        np.testing.assert_array_equal(f.numpy(), faces)
    # rejections
    np.savez(tmp_path / "nokey.npz", verts=verts, faces=faces)
    with pytest.raises(ValueError, match="vertices"):
        geometry.load_mesh(tmp_path / "nokey.npz")
    np.savez(tmp_path / "quads.npz", vertices=verts, faces=np.zeros((4, 4), np.int64))
    with pytest.raises(ValueError):
        geometry.load_mesh(tmp_path / "quads.npz")
    np.savez(tmp_path / "range.npz", vertices=verts, faces=faces + len(verts))
    with pytest.raises(ValueError):
        geometry.load_mesh(tmp_path / "range.npz")
    for binary in (False, True):
        _write_ply(tmp_path / "quad.ply", verts, faces, binary, quad=True)
        with pytest.raises(ValueError, match="triangle"):
            geometry.load_mesh(tmp_path / "quad.ply")
    (tmp_path / "big.ply").write_bytes(b"ply\nformat binary_big_endian 1.0\nelement vertex 0\nend_header\n")
    with pytest.raises(ValueError):
        geometry.load_mesh(tmp_path / "big.ply")
    (tmp_path / "m.obj").write_text("v 0 0 0\n")
    with pytest.raises(ValueError):
        geometry.load_mesh(tmp_path / "m.obj")


def test_mesh_metrics_argument_errors():
    from arah_release_amd import geometry
    good = torch.from_numpy(icosphere(0))
    for bad in (torch.zeros(4, 3), torch.zeros(4, 3, 2), torch.zeros(0, 3, 3), (torch.zeros(5, 3), torch.zeros(0, 3, dtype=torch.int64)),
                (torch.zeros(5, 2), torch.zeros(2, 3, dtype=torch.int64)), (torch.zeros(5, 3), torch.zeros(2, 4, dtype=torch.int64)),
                (torch.zeros(5, 3), torch.zeros(2, 3))):
        with pytest.raises(ValueError):
            geometry.mesh_metrics(bad, good)
        with pytest.raises(ValueError):
            geometry.mesh_metrics(good, bad)
    for n in (0, -3, 2.5):
        with pytest.raises(ValueError):
            geometry.mesh_metrics(good, good, n_samples=n)
    with pytest.raises(ValueError):   # host-resident meshes: the scores run on the HIP kernels
        geometry.mesh_metrics(good, good, n_samples=10)


# ---------------------------------------------------------------------------------------------------------- GPU tests
DEV = "cuda:0"


def _f10_tris(dev):
    g = golden("f10_mesh_contains.npz")
    return torch.from_numpy(g["verts"].astype(np.float32)[g["faces"]]).to(dev).contiguous()


def _query_both(hip, tris, pts):
    """(indexed result, brute-force result) on the same soup."""
    verts = tris.reshape(-1, 3).contiguous()
    faces = torch.arange(verts.shape[0], dtype=torch.int32, device=tris.device).reshape(-1, 3)
    d2, face, closest, _ = hip.mesh_closest(hip.mesh_index(tris), pts)
    rd2, rface, rclosest, _, _ = hip.mesh_query(verts, faces, pts)
    return (d2, face, closest), (rd2, rface, rclosest)


def _assert_same(got, want, what):
    for g, w, name in zip(got, want, ("d2", "face", "closest")):
        np.testing.assert_array_equal(g.cpu().numpy(), w.cpu().numpy(), err_msg="%s: %s" % (what, name))


def _query_sets(tris, other, seed):
    """Points that exercise a mesh's index: samples of another mesh (as they are and moved onto this mesh), the mesh's own
    vertices and edge midpoints (ties between the faces that share them), uniform points in 3 x the bounding box, and 64
    points 5 to 10 box diagonals away."""
    from arah_release_amd import data
    dev = tris.device
    gen = torch.Generator(device=dev).manual_seed(seed)
    lo, hi = tris.reshape(-1, 3).min(0).values, tris.reshape(-1, 3).max(0).values
    mid, diag = 0.5 * (lo + hi), (hi - lo).norm()
    o = other.reshape(-1, 3)
    samples, _ = data.sample_surface(o, torch.arange(o.shape[0], device=dev).reshape(-1, 3), 2000, generator=gen)
    sel = torch.randperm(tris.shape[0], device=dev, generator=gen)[:1500]
    corners = tris[sel].reshape(-1, 3)
    edges = (0.5 * (tris[sel] + tris[sel].roll(1, 1))).reshape(-1, 3)
    box = mid + (torch.rand(2000, 3, device=dev, generator=gen) - 0.5) * 3.0 * (hi - lo)
    d = torch.randn(64, 3, device=dev, generator=gen)
    far = mid + d / d.norm(dim=1, keepdim=True) * diag * (5.0 + 5.0 * torch.rand(64, 1, device=dev, generator=gen))
    return {"other's samples": samples, "other's samples, recentred": samples - 0.5 * (o.min(0).values + o.max(0).values) + mid,
            "own vertices": corners, "edge midpoints": edges, "3x box": box, "far": far}


@pytest.fixture(scope="module")
def posed(scene):
    """The synthetic subject's posed meshes at two resolutions."""
    dev = torch.device(DEV)
    model, _ = get_model("zju377_mono", dev)
    model.eval()
    inputs = scene.make_inputs(32, 32, frame_idx=0, device=dev)
    with torch.no_grad():
        m128 = model.posed_mesh(inputs, n_side=128)
    return {"model": model, "inputs": inputs, "m128": m128}


@gpu
def test_mesh_closest_equals_mesh_query(posed):
    from arah_release_amd import geometry, hip
    dev = torch.device(DEV)
    smpl, lattice = _f10_tris(dev), posed["m128"]["tris"].contiguous()
    assert lattice.shape[0] > 5000
    for name, tris, other in (("f10", smpl, lattice), ("posed 128", lattice, smpl)):
        index = hip.mesh_index(tris)
        head = index.header()
        print("%s: %d faces, grid %s, cell %.4f m, %d references, %d on the big list" % (name, tris.shape[0], head["n"], head["h"],
                                                                                         head["n_refs"], head["n_big"]))
        assert head["status"] == 0 and head["n_refs"] <= 8 * tris.shape[0] and head["n_big"] <= tris.shape[0]
        for what, pts in _query_sets(tris, other, seed=3).items():
            pts = pts.float().contiguous()
            got, want = _query_both(hip, tris, pts)
            _assert_same(got, want, "%s, %s" % (name, what))
            _, _, _, tested = hip.mesh_closest(index, pts, want_closest=False, want_tested=True)
            print("   %-28s %5d points: tests per query mean %.1f max %d of %d faces" % (what, pts.shape[0], tested.float().mean().item(),
                                                                                        int(tested.max()), tris.shape[0]))
    # duplicated triangles: the lowest index wins
    gen = torch.Generator(device=dev).manual_seed(4)
    dup = torch.cat([smpl, smpl[torch.randperm(smpl.shape[0], device=dev, generator=gen)[:4000]]]).contiguous()
    pts = _query_sets(smpl, lattice, seed=5)
    for what in ("own vertices", "edge midpoints", "3x box"):
        got, want = _query_both(hip, dup, pts[what].float().contiguous())
        _assert_same(got, want, "duplicated, %s" % what)
        assert int(got[1].max()) < smpl.shape[0]
    # exactly degenerate faces leave by the rule of the definition
    bad = smpl.clone()
    sel = torch.randperm(smpl.shape[0], device=dev, generator=gen)[:500]
    bad[sel[:250], 1] = bad[sel[:250], 0]
    bad[sel[250:]] = bad[sel[250:], :1]
    keep = torch.from_numpy(kept_faces_np(bad.cpu().numpy())).to(dev)
    assert int(keep.sum()) == smpl.shape[0] - 500
    soup, n_kept, sample_faces = geometry.drop_degenerate(bad)
    assert int(n_kept) == int(keep.sum()) and torch.equal(soup[:int(n_kept)], bad[keep])
    assert bool((sample_faces[int(n_kept):] == 0).all()) and torch.equal(soup[int(n_kept):], soup[int(n_kept) - 1:int(n_kept)].expand(500, 3, 3))
    for what in ("own vertices", "3x box", "far"):
        p = pts[what].float().contiguous()
        d2, face, closest, _ = hip.mesh_closest(hip.mesh_index(soup), p)
        _, want = _query_both(hip, bad[keep].contiguous(), p)
        _assert_same((d2, face, closest), want, "degenerate faces dropped, %s" % what)


@gpu
def test_mesh_closest_big_triangles_over_a_dense_patch():
    """A few box-sized triangles over a dense patch: they overlap more cells than a triangle is referenced from and go to the
    list every query walks; results still equal the brute force."""
    from arah_release_amd import hip
    dev = torch.device(DEV)
    dense = torch.from_numpy(flat_patch(64, 0.25)).to(dev)
    big = torch.tensor([[[-2, -2, 0.5], [2, -2, 0.5], [0, 2, -0.5]], [[-2, 2, -1], [2, 2, 1], [0, -2, 0.25]],
                        [[-2, 0, -2], [2, 0, -2], [0, 0.5, 2]]], dtype=torch.float32, device=dev)
    tris = torch.cat([big[:1], dense, big[1:]]).contiguous()
    head = hip.mesh_index(tris).header()
    assert head["n_big"] == 3 and head["n_refs"] >= dense.shape[0]
    gen = torch.Generator(device=dev).manual_seed(6)
    pts = torch.cat([(torch.rand(3000, 3, device=dev, generator=gen) - 0.5) * 5.0,
                     (torch.rand(3000, 3, device=dev, generator=gen) - 0.5) * torch.tensor([0.6, 0.6, 0.1], device=dev),
                     tris.reshape(-1, 3)[::7]]).contiguous()
    got, want = _query_both(hip, tris, pts)
    _assert_same(got, want, "big triangles")
    assert int((got[1] == 0).sum()) > 0 and int(((got[1] > 0) & (got[1] <= dense.shape[0])).sum()) > 0
    # finite float32 coordinates up to the format's largest are in the domain
    huge = torch.tensor([[[3.3e38, 0, 0], [0, 3.3e38, 0], [0, 0, -3.3e38]], [[-3.4e38, 1e38, 0], [0, -3.4e38, 1e38], [1e38, 0, 3.4e38]]],
                        dtype=torch.float32, device=dev)
    far = ((torch.rand(500, 3, device=dev, generator=gen) - 0.5) * 3.0e38 * 2.0).contiguous()   # (6e38 is not a float32)
    assert bool(torch.isfinite(far).all())
    assert hip.mesh_index(huge).header()["status"] == 0
    got, want = _query_both(hip, huge, far)
    _assert_same(got, want, "coordinates near the largest float32")
    assert bool(torch.isfinite(got[0]).all())
    # one triangle, and a mesh of one point
    for soup in (big[:1].contiguous(), big[:1, :1].expand(1, 3, 3).contiguous()):
        got, want = _query_both(hip, soup, pts[:500].contiguous())
        np.testing.assert_array_equal(got[1].cpu().numpy(), want[1].cpu().numpy())
        np.testing.assert_array_equal(got[0].cpu().numpy(), want[0].cpu().numpy())


@gpu
def test_mesh_closest_order_shapes_builds_and_streams(posed):
    from arah_release_amd import hip
    dev = torch.device(DEV)
    tris = posed["m128"]["tris"].contiguous()
    sets = _query_sets(tris, _f10_tris(dev), seed=7)
    pts = torch.cat([sets["other's samples, recentred"], sets["own vertices"], sets["3x box"], sets["far"]]).float().contiguous()
    assert pts.shape[0] > 4097
    index = hip.mesh_index(tris)
    full = hip.mesh_closest(index, pts, want_tested=True)
    perm = torch.randperm(pts.shape[0], device=dev, generator=torch.Generator(device=dev).manual_seed(8))
    shuffled = hip.mesh_closest(index, pts[perm].contiguous(), want_tested=True)
    for a, b in zip(full, shuffled):
        assert torch.equal(a[perm], b)
    for n in (0, 1, 63, 64, 65, 4097):
        part = hip.mesh_closest(index, pts[:n].contiguous(), want_tested=True)
        for a, b in zip(full, part):
            assert b.shape[0] == n and torch.equal(a[:n], b)
    again = hip.mesh_closest(hip.mesh_index(tris.clone()), pts, want_tested=True)
    for a, b in zip(full, again):
        assert torch.equal(a, b)
    # a second stream, other work in flight on the first
    side = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    x = torch.randn(4096, 4096, device=dev)
    for _ in range(8):
        x = (x @ x).clamp(-1, 1)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        other = hip.mesh_closest(hip.mesh_index(tris), pts, want_tested=True)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    for a, b in zip(full, other):
        assert torch.equal(a, b)
    assert bool(torch.isfinite(x).all())
    # what the wrappers refuse
    with pytest.raises(ValueError):
        hip.mesh_index(tris.double())
    with pytest.raises(ValueError):
        hip.mesh_index(tris[:0])
    with pytest.raises(ValueError):
        hip.mesh_closest(index, pts.double())
    with pytest.raises(ValueError):
        hip.mesh_closest(index, pts[:, :2])


def _gpu_closest(tris, pts):
    """The restatement's distance source on the GPU: hip.mesh_query, every triangle for every point."""
    from arah_release_amd import hip
    t = torch.from_numpy(np.ascontiguousarray(tris, np.float32)).to(DEV)
    p = torch.from_numpy(np.ascontiguousarray(pts, np.float32)).to(DEV)
    faces = torch.arange(t.shape[0] * 3, dtype=torch.int32, device=DEV).reshape(-1, 3)
    d2, face, _, _, _ = hip.mesh_query(t.reshape(-1, 3).contiguous(), faces, p)
    return d2.cpu().numpy(), face.cpu().numpy().astype(np.int64)


def _restate_call(res):
    """The restatement on the samples a mesh_metrics call drew (its debug return)."""
    s = res["samples"]
    ka, kb = int(s["n_faces_a"]), int(s["n_faces_b"])
    a, b = s["tris_a"][:ka].cpu().numpy(), s["tris_b"][:kb].cpu().numpy()
    fa, fb = s["face_a"].cpu().numpy(), s["face_b"].cpu().numpy()
    assert fa.max() < ka and fb.max() < kb
    return restate_metrics(a, s["points_a"].cpu().numpy(), fa, b, s["points_b"].cpu().numpy(), fb, closest=_gpu_closest), a, b


@gpu
def test_mesh_metrics_against_the_restatement():
    from arah_release_amd import geometry
    dev = torch.device(DEV)
    a = _f10_tris(dev)
    gen = torch.Generator(device=dev).manual_seed(9)
    # the ground truth: the same body, its vertices moved by up to 1 cm, shifted by 2 cm, with some faces made degenerate
    g = golden("f10_mesh_contains.npz")
    verts = torch.from_numpy(g["verts"].astype(np.float32)).to(dev)
    verts_b = verts + (torch.rand(verts.shape, device=dev, generator=gen) - 0.5) * 0.02 + torch.tensor([0.02, 0.0, 0.0], device=dev)
    faces = torch.from_numpy(g["faces"].astype(np.int64)).to(dev)
    faces_b = faces.clone()
    faces_b[::97, 1] = faces_b[::97, 0]
    res = geometry.mesh_metrics(a, (verts_b, faces_b), n_samples=6000, seed=11, return_samples=True)
    assert res["n_a"] == res["n_b"] == 6000
    for k in KEYS:
        assert res[k].dim() == 0 and res[k].dtype == torch.float64 and res[k].is_cuda, k
    want, ta, tb = _restate_call(res)
    assert ta.shape[0] == a.shape[0] and tb.shape[0] == faces.shape[0] - len(range(0, faces.shape[0], 97))
    bound = max(np.abs(ta).max(), np.abs(tb).max()) ** 2
    for k in KEYS:
        got = float(res[k])
        tol = 64 * 2.0 ** -53 * (abs(want[k]) + bound)
        print("%-20s %.17g restated %.17g  |diff| %.3g  tol %.3g" % (k, got, want[k], abs(got - want[k]), tol))
    for k in KEYS:
        assert abs(float(res[k]) - want[k]) <= 64 * 2.0 ** -53 * (abs(want[k]) + bound), k
    assert 0.001 < want["accuracy"] < 0.03 and 0.5 < want["normal_consistency"] <= 1.0
    # a face index out of range never reaches the device as one: the scores are NaN
    wild = faces_b.clone()
    wild[5, 2] = verts_b.shape[0]
    bad = geometry.mesh_metrics(a, (verts_b, wild), n_samples=100, seed=0)
    assert all(bool(torch.isnan(bad[k])) for k in KEYS)
    # (verts, faces) pairs and soups are the same mesh
    pair = geometry.mesh_metrics((verts, faces), (verts_b, faces_b), n_samples=6000, seed=11)
    for k in KEYS:
        assert torch.equal(pair[k], res[k]), k


@gpu
def test_mesh_metrics_determinism_and_brackets():
    from arah_release_amd import geometry
    dev = torch.device(DEV)
    r1, r2 = 0.8, 1.0
    a_np, b_np = icosphere(4, r1), icosphere(5, r2)
    lo, hi = sphere_bracket(a_np, r1, b_np, r2)
    a, b = torch.from_numpy(a_np).to(dev), torch.from_numpy(b_np).to(dev)
    first = geometry.mesh_metrics(a, b, n_samples=20000, seed=0, return_samples=True)
    again = geometry.mesh_metrics(a, b, n_samples=20000, seed=0, return_samples=True)
    other = geometry.mesh_metrics(a, b, n_samples=20000, seed=1, return_samples=True)
    for k in KEYS:
        assert torch.equal(first[k], again[k]), k
    assert torch.equal(first["samples"]["points_a"], again["samples"]["points_a"])
    assert not torch.equal(first["samples"]["points_a"], other["samples"]["points_a"])
    assert not torch.equal(first["samples"]["points_b"], other["samples"]["points_b"])
    assert any(not torch.equal(first[k], other[k]) for k in KEYS)
    for r in (first, other):
        print({k: float(r[k]) for k in KEYS}, "bracket", lo, hi)
        for k in ("accuracy", "completeness", "chamfer_l1", "hausdorff_ab", "hausdorff_ba"):
            assert lo <= float(r[k]) <= hi, k
        assert lo * lo <= float(r["chamfer_l2"]) <= hi * hi
        d_ab, d_ba = r["samples"]["d2_ab"].sqrt(), r["samples"]["d2_ba"].sqrt()
        assert lo <= float(d_ab.min()) and lo <= float(d_ba.min())
        assert 0.99 < float(r["normal_consistency"]) <= 1.0
    # nothing is copied to the host and the stream is never waited for
    torch.cuda.synchronize(dev)
    torch.cuda.set_sync_debug_mode("error")
    try:
        quiet = geometry.mesh_metrics(a, b, n_samples=20000, seed=0)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for k in KEYS:
        assert torch.equal(first[k], quiet[k]), k
    # a mesh against itself: the samples lie on it up to their float32 rounding
    same = geometry.mesh_metrics(b, b, n_samples=20000, seed=2)
    tol = np.sqrt(3) * 4 * F32 * r2
    assert float(same["hausdorff_ab"]) <= tol and float(same["hausdorff_ba"]) <= tol and float(same["chamfer_l1"]) <= tol


@gpu
def test_geometry_metrics_on_the_synthetic_subject(posed):
    model, inputs = posed["model"], posed["inputs"]
    with torch.no_grad():
        m256 = model.posed_mesh(inputs, n_side=256)
        own = model.geometry_metrics(inputs, m256["tris"], n_side=256, n_samples=50000, seed=0)
        coarse = model.geometry_metrics(inputs, posed["m128"]["tris"], n_side=256, n_samples=50000, seed=0)
    assert own["n_tris"] == m256["n_tris"] and own["n_a"] == own["n_b"] == 50000
    tol = np.sqrt(3) * 4 * F32 * float(m256["tris"].abs().max())
    print("own mesh:", {k: float(own[k]) for k in KEYS}, "tolerance", tol)
    assert float(own["hausdorff_ab"]) <= tol and float(own["hausdorff_ba"]) <= tol and float(own["chamfer_l1"]) <= tol
    assert float(own["normal_consistency"]) > 0.99
    cell = float(posed["m128"]["box"][3]) / 127.0
    print("128 mesh:", {k: float(coarse[k]) for k in KEYS}, "coarse cell diagonal", np.sqrt(3) * cell)
    assert 0.0 < float(coarse["accuracy"]) < np.sqrt(3) * cell and 0.0 < float(coarse["completeness"]) < np.sqrt(3) * cell
    verts = posed["m128"]["tris"].reshape(-1, 3)
    pair = model.geometry_metrics(inputs, (verts, torch.arange(verts.shape[0], device=verts.device).reshape(-1, 3)), n_side=256,
                                  n_samples=50000, seed=0)
    assert all(torch.equal(pair[k], coarse[k]) for k in KEYS)
    cpu_inputs = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in inputs.items()}
    with pytest.raises(ValueError):
        model.geometry_metrics(cpu_inputs, m256["tris"])
    model.train()
    try:
        with pytest.raises(ValueError):
            model.geometry_metrics(inputs, m256["tris"])
    finally:
        model.eval()


@gpu
def test_validate_with_geometry(tmp_path, scene, monkeypatch):
    """python -m arah_release_amd.validate --geometry DIR on the synthetic capture of the validation tests, the ground truth
    written from posed_mesh for two of its three frames (one .npz, one binary .ply)."""
    import yaml
    from test_validation import _capture_cfg, _fake_samples, _write_capture
    from arah_release_amd import config, data, smpl, train, validate
    dev = torch.device(DEV)
    body = smpl.BodyModel.synthetic(scene)
    monkeypatch.setattr(data, "training_samples", _fake_samples)
    n_frames, size = 3, 256
    faces = np.zeros((1, 3), np.int32)
    _write_capture(tmp_path / "data", scene, n_frames=n_frames, size=size, focal=300.0, full_masks=True)
    cfg = _capture_cfg(tmp_path)
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(cfg))
    argv = [str(tmp_path / "cfg.yaml"), "--default-config", str(tmp_path / "cfg.yaml")]
    train_ds = data.get_capture_dataset("train", cfg, body=body, faces=faces)
    val_ds = data.get_capture_dataset("val", cfg, body=body, faces=faces)
    lm = config.get_model(cfg, dataset=train_ds, mode="val", body_model=body)
    own = lm.model.state_dict()
    lm.model.load_state_dict({k: v for k, v in config.synthetic_state_dict(cfg).items()
                              if k not in own or own[k].shape == v.shape}, strict=False)
    train.save_checkpoint(str(tmp_path / "out" / "checkpoints" / "last.ckpt"), lm, lm.configure_optimizers(), epoch=1, global_step=n_frames)
    lm = lm.to(dev).eval()
    gt_dir = tmp_path / "gt"
    gt_dir.mkdir()
    coords = 0.0
    for i in (0, 2):
        with torch.no_grad():
            mesh = lm.model.posed_mesh(lm.compose_inputs(val_ds.validation_item(i, dev), eval=True), n_side=128)
        verts = mesh["tris"].reshape(-1, 3).cpu().numpy()
        coords = max(coords, float(np.abs(verts).max()))
        tri_faces = np.arange(len(verts)).reshape(-1, 3)
        stem = os.path.splitext(os.path.basename(val_ds.data[i]["model_file"]))[0]
        if i == 0:
            np.savez(gt_dir / (stem + ".npz"), vertices=verts, faces=tri_faces)
        else:
            _write_ply(gt_dir / (stem + ".ply"), verts, tri_faces, binary=True)
    lines = []
    plain = validate.main(argv, body=body, faces=faces, log=lines.append)
    assert set(json.loads(lines[-1])) == {"n", "n_psnr_inf", "psnr", "ssim", "seconds_per_frame", "world", "data_range", "mode"}
    assert all(set(f) == {"frame", "status", "psnr", "ssim"} for f in json.load(open(tmp_path / "out" / "validation.json"))["frames"])
    res = validate.main(argv + ["--geometry", str(gt_dir), "--geometry-n-side", "128", "--geometry-samples", "20000"], body=body,
                        faces=faces, log=lines.append)
    line = json.loads(lines[-1])
    print("validate --geometry:", lines[-1])
    assert set(line) == set(json.loads(lines[-2])) | set(KEYS) | {"n_geometry"}
    assert line["n"] == n_frames and line["n_geometry"] == 2
    assert line["psnr"] == plain["psnr"] and line["ssim"] == plain["ssim"]
    tol = np.sqrt(3) * 4 * F32 * coords     # the ground truth IS the posed mesh: distances are the samples' float32 rounding
    assert 0.0 <= line["chamfer_l1"] <= tol and line["hausdorff_ab"] <= tol and line["hausdorff_ba"] <= tol
    assert line["normal_consistency"] > 0.99
    saved = json.load(open(tmp_path / "out" / "validation.json"))
    scored = [f for f in saved["frames"] if "chamfer_l1" in f]
    assert [f["frame"] for f in scored] == [0, 2] and "chamfer_l1" not in saved["frames"][1]
    assert np.mean([f["chamfer_l1"] for f in scored]) == pytest.approx(line["chamfer_l1"], abs=1e-18)
    # no frame has a ground truth: the means are null, the line is still strict JSON
    (tmp_path / "empty").mkdir()
    validate.main(argv + ["--geometry", str(tmp_path / "empty")], body=body, faces=faces, log=lines.append)

    def no_constant(name):
        raise AssertionError("%s in the JSON line" % name)
    none = json.loads(lines[-1], parse_constant=no_constant)
    assert none["n_geometry"] == 0 and all(none[k] is None for k in KEYS) and none["psnr"] == plain["psnr"]
    with pytest.raises(FileNotFoundError):
        validate.main(argv + ["--geometry", str(tmp_path / "nowhere")], body=body, faces=faces, log=lines.append)
