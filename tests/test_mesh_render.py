"""Indexed meshes drawn: meshing.mesh_rasterize / interpolate_attributes (the rule) against a scalar restatement, the properties
the rule is there for (watertight along shared edges, perspective-correct), the kernels hip.mesh_rasterize / hip.mesh_interpolate
against the rule bit for bit, and the public entries geometry.render_mesh and MetaAvatarRender.render_mesh."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from conftest import get_model

gpu = pytest.mark.gpu
DEV = "cuda:0"
f32, f64 = np.float32, np.float64
CULLS = ("none", "back", "front")


# ---- the rule once more, in scalar loops: one rounding per operation (numpy float32 / float64 scalars) -----------------------------
def _edges(c, px, py):
    (x0, y0, _), (x1, y1, _), (x2, y2, _) = c
    return ((x1 - px) * (y2 - py) - (x2 - px) * (y1 - py), (x2 - px) * (y0 - py) - (x0 - px) * (y2 - py),
            (x0 - px) * (y1 - py) - (x1 - px) * (y0 - py))


def restate_rasterize(verts, faces, H, W, z_near=1e-4, cull="none"):
    verts, faces = np.asarray(verts, f32), np.asarray(faces, np.int64)
    V, zn = len(verts), f32(z_near)
    best = {}
    with np.errstate(all="ignore"):
        for f, ids in enumerate(faces):
            if not all(0 <= int(k) < V for k in ids):
                continue
            c = [tuple(f32(t) for t in verts[int(k)]) for k in ids]
            if not all(p[2] > zn and np.isfinite(p[2]) for p in c):
                continue
            (x0, y0, z0), (x1, y1, z1), (x2, y2, z2) = c
            area2 = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)
            if not np.isfinite(area2) or area2 == 0 or (cull == "back" and area2 < 0) or (cull == "front" and area2 > 0):
                continue
            xs, ys = (x0, x1, x2), (y0, y1, y2)
            for i in range(H):
                for j in range(W):
                    px, py = f32(j) + f32(0.5), f32(i) + f32(0.5)
                    if not (min(xs) <= px <= max(xs) and min(ys) <= py <= max(ys)):        # the closed bounding box
                        continue
                    e0, e1, e2 = _edges(c, px, py)
                    inside = (e0 >= 0 and e1 >= 0 and e2 >= 0) if area2 > 0 else (e0 <= 0 and e1 <= 0 and e2 <= 0)
                    s = (e0 + e1) + e2
                    if not inside or s == 0:
                        continue
                    z = f32(1.0) / (((e0 / z0 + e1 / z1) + e2 / z2) / s)
                    if not (np.isfinite(z) and z > 0):
                        continue
                    key = (int(np.array(z, f32).view(np.uint32)) << 32) | f
                    if (i, j) not in best or key < best[(i, j)][0]:
                        best[(i, j)] = (key, (e0, e1, e2), (z0, z1, z2))
    p2f = np.full((H, W), -1, np.int32)
    depth = np.full((H, W), -1.0, f32)
    bary = np.full((H, W, 3), -1.0, f32)
    for (i, j), (key, e, z) in best.items():
        p2f[i, j] = key & 0xffffffff
        depth[i, j] = np.array(key >> 32, np.uint32).view(f32)
        E = [f64(t) for t in e]
        S = (E[0] + E[1]) + E[2]
        p = [(E[k] / S) / f64(z[k]) for k in range(3)]
        P = (p[0] + p[1]) + p[2]
        bary[i, j] = [f32(p[k] / P) for k in range(3)]
    return p2f, depth, bary


def restate_interpolate(p2f, bary, faces, attr, background):
    faces, attr = np.asarray(faces, np.int64), np.asarray(attr, f32)
    H, W = p2f.shape
    out = np.full((H, W, attr.shape[1]), f32(background), f32)
    with np.errstate(all="ignore"):
        for i in range(H):
            for j in range(W):
                f = int(p2f[i, j])
                if not 0 <= f < len(faces) or not all(0 <= int(k) < len(attr) for k in faces[f]):
                    continue
                b = [f64(t) for t in bary[i, j]]
                for c in range(attr.shape[1]):
                    a = [f64(attr[int(k), c]) for k in faces[f]]
                    out[i, j, c] = f32((b[0] * a[0] + b[1] * a[1]) + b[2] * a[2])
    return out


def bits(t):
    t = t.detach().cpu().contiguous() if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t))
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def assert_same(got, want, what=""):
    for name, g, w in zip(("pix_to_face", "depth", "bary"), got, want):
        g, w = bits(g), bits(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        n_bad = int((g != w).sum())
        assert n_bad == 0, "%s %s: %d of %d values differ" % (what, name, n_bad, g.numel())


# ---- meshes ----------------------------------------------------------------------------------------------------------------------
def handmade():
    """12 x 12: two overlapping faces, one face twice (the lower id wins the tie), one behind z_near, one with a NaN vertex, one with
    an id out of range, one with a repeated id, one of each orientation."""
    verts = torch.tensor([[1.0, 1.0, 2.0], [10.5, 1.5, 2.5], [2.0, 10.0, 3.0],        # 0-2
                          [11.0, 11.0, 1.5], [0.5, 6.5, 2.2], [6.5, 0.5, 2.7],          # 3-5
                          [3.0, 3.0, -1.0], [9.0, 3.0, 1.0], [6.0, 9.0, 1.0],           # 6-8: 6 is behind
                          [float("nan"), 2.0, 1.0], [4.0, 4.0, 5e-5], [7.5, 7.5, 0.9]], dtype=torch.float32)
    faces = torch.tensor([[0, 1, 2], [3, 2, 1], [4, 5, 3], [3, 2, 1], [6, 7, 8], [9, 7, 8], [0, 1, 12], [0, -1, 2], [0, 0, 2],
                          [10, 7, 8], [11, 8, 7], [2, 1, 0]], dtype=torch.int64)
    return verts, faces


def random_set(F=600, H=96, W=128, seed=5):
    """The construction of test_meshing.test_rasterize_against_oracle, indexed: small faces scattered over and around the image."""
    g = torch.Generator().manual_seed(seed)
    c = torch.rand(F, 1, 2, generator=g) * torch.tensor([W, H]) * 1.2 - torch.tensor([W, H]) * 0.1
    uv = c + (torch.rand(F, 3, 2, generator=g) - 0.5) * 14
    z = 1.0 + torch.rand(F, 3, 1, generator=g) * 3
    z[:7] = -0.5                                                          # behind the camera: dropped
    verts = torch.cat([uv, z], dim=-1).float().reshape(-1, 3)
    return verts, torch.arange(3 * F).reshape(F, 3)


def with_large(at, H=96, W=128):
    """random_set with three faces put in at the ids at, at + 1, at + 2: two that cover the whole image (one behind most of the small
    faces, one tilted through them and it, of opposite orientations) and one whose bounding box reaches 1e5 pixels beyond the image."""
    verts, faces = random_set(600, H, W)
    V = verts.shape[0]
    big = torch.tensor([[-5.0, -5.0, 4.2], [2.0 * W + 10, -5.0, 4.4], [-5.0, 2.0 * H + 10, 4.6],
                        [-7.0, -6.0, 2.0], [-7.0, 2.0 * H + 20, 9.0], [2.0 * W + 20, -6.0, 9.5],
                        [-1.0e5, 40.0, 3.0], [1.0e5, 60.0, 3.2], [40.0, 1.0e5, 3.1]])
    extra = torch.arange(V, V + 9).reshape(3, 3)
    return torch.cat([verts, big]), torch.cat([faces[:at], extra, faces[at:]])


def grid_mesh(n, seed, half):
    """A jittered n x n tessellation of [6,58] x [5,59] on a tilted plane (1 / z is linear in the pixel coordinates), random diagonals,
    one orientation; half: the vertices rounded to half-integers, so that pixel centres fall exactly on vertices and edges."""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.linspace(6.0, 58.0, n), np.linspace(5.0, 59.0, n), indexing="xy")
    step = np.array([52.0, 54.0]) / (n - 1)
    jit = (rng.random((n, n, 2)) - 0.5) * 0.6 * step
    jit[0, :, 1] = jit[-1, :, 1] = 0.0                                    # the border stays on the rectangle
    jit[:, 0, 0] = jit[:, -1, 0] = 0.0
    jit[0, 0] = jit[0, -1] = jit[-1, 0] = jit[-1, -1] = 0.0
    x, y = gx + jit[..., 0], gy + jit[..., 1]
    if half:
        x, y = np.round(x * 2.0) / 2.0, np.round(y * 2.0) / 2.0
        x[:, 0], x[:, -1], y[0], y[-1] = 6.0, 58.0, 5.0, 59.0
    z = 1.0 / (0.45 - 0.002 * x - 0.003 * y)
    verts = torch.from_numpy(np.stack([x, y, z], -1).reshape(-1, 3)).float()
    faces = []
    for r in range(n - 1):
        for c in range(n - 1):
            a, b, d, e = r * n + c, r * n + c + 1, (r + 1) * n + c, (r + 1) * n + c + 1
            faces += [[a, b, e], [a, e, d]] if rng.random() < 0.5 else [[a, b, d], [b, e, d]]
    return verts, torch.tensor(faces, dtype=torch.int64)


GRIDS = [(n, s, half) for s, n in enumerate((5, 6, 8, 11, 13, 17, 23, 29, 33, 40)) for half in (False, True)]
_SPEC = {}


def spec(name, make, H, W, cull="none", z_near=1e-4):
    """The rule's result for a named mesh, computed once on the host and shared."""
    from arah_release_amd import meshing
    key = (name, H, W, cull, z_near)
    if key not in _SPEC:
        verts, faces = make()
        _SPEC[key] = (verts, faces, meshing.mesh_rasterize(verts, faces, H, W, z_near=z_near, cull=cull))
    return _SPEC[key]


# ---- CPU: the rule -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cull", CULLS)
def test_rule_equals_its_restatement_on_the_handmade_faces(cull):
    from arah_release_amd import meshing
    verts, faces = handmade()
    got = meshing.mesh_rasterize(verts, faces, 12, 12, cull=cull)
    want = restate_rasterize(verts.numpy(), faces.numpy(), 12, 12, cull=cull)
    assert_same(got, want, cull)
    p2f = got[0]
    assert got[0].dtype == torch.int32 and got[1].dtype == torch.float32 and got[2].shape == (12, 12, 3)
    drawn = set(p2f[p2f >= 0].tolist())
    assert drawn and not drawn & {3, 4, 5, 6, 7, 8, 9}                     # the tie goes to face 1, the invalid ones draw nothing
    # faces 0, 1, 2 and 10 have area2 > 0; 11 is 0 reversed (the same plane, its depths rounded differently); 3 is 1 once more
    assert drawn <= ({0, 1, 2, 10, 11} if cull == "none" else {0, 1, 2, 10} if cull == "back" else {11})
    assert {0, 1, 10} <= drawn or cull == "front"
    if cull == "none":
        assert bool(((p2f >= 0) == (got[1] > 0)).all()) and bool((got[2][p2f < 0] == -1).all())
        on = got[2][p2f >= 0]
        assert float((on.sum(1) - 1).abs().max()) < 1e-6 and float(on.min()) >= 0.0


@pytest.mark.parametrize("seed", range(4))
def test_rule_equals_its_restatement_on_random_faces(seed):
    from arah_release_amd import meshing
    H, W = (12, 12) if seed % 2 else (7, 11)
    verts, faces = random_set(24, H, W, seed=seed)
    if seed >= 2:
        verts[:, :2] = torch.round(verts[:, :2] * 2) / 2                  # vertices and edges on pixel centres
    faces = torch.cat([faces, faces[5:8]])                               # exact ties
    cull = CULLS[seed % 3]
    got = meshing.mesh_rasterize(verts, faces, H, W, z_near=0.5, cull=cull)
    assert_same(got, restate_rasterize(verts.numpy(), faces.numpy(), H, W, z_near=0.5, cull=cull), "seed %d" % seed)
    assert int((got[0] >= 0).sum()) > H * W // 8


def test_interpolation_equals_its_restatement():
    from arah_release_amd import meshing
    verts, faces = handmade()
    p2f, _, bary = meshing.mesh_rasterize(verts, faces, 12, 12)
    g = torch.Generator().manual_seed(1)
    for n_ch, background in ((1, 0.0), (3, -1.0), (5, 0.25)):
        attr = (torch.rand(verts.shape[0], n_ch, generator=g) * 4 - 2).float()
        got = meshing.interpolate_attributes(p2f, bary, faces, attr, background=background)
        want = restate_interpolate(p2f.numpy(), bary.numpy(), faces.numpy(), attr.numpy(), background)
        assert got.dtype == torch.float32 and torch.equal(bits(got), bits(want))
        assert bool((got[p2f < 0] == background).all())
    # a pix_to_face that names no face of this mesh, or a face with an id out of range, is background
    odd = p2f.clone()
    odd[0, 0], odd[0, 1], odd[0, 2] = 99, 6, 7
    got = meshing.interpolate_attributes(odd, bary, faces, attr, background=9.0)
    assert bool((got[0, :3] == 9.0).all())
    assert torch.equal(bits(got), bits(restate_interpolate(odd.numpy(), bary.numpy(), faces.numpy(), attr.numpy(), 9.0)))


@pytest.mark.parametrize("n,seed,half", GRIDS)
def test_rule_is_watertight_on_jittered_grids(n, seed, half):
    """Every pixel centre inside the tessellated rectangle [6,58] x [5,59] is covered, none outside is: 0 violations."""
    H = W = 64
    _, faces, (p2f, depth, bary) = spec("grid%d-%d-%d" % (n, seed, half), lambda: grid_mesh(n, seed, half), H, W)
    assert faces.shape[0] == 2 * (n - 1) ** 2
    inside = torch.zeros(H, W, dtype=torch.bool)
    inside[5:59, 6:58] = True                                             # centres j + 0.5 in [6,58], i + 0.5 in [5,59]
    covered = p2f >= 0
    assert int((inside & ~covered).sum()) == 0 and int((covered & ~inside).sum()) == 0
    # on the plane 1 / z = 0.45 - 0.002 x - 0.003 y, whichever face took the pixel
    jj, ii = torch.meshgrid(torch.arange(W) + 0.5, torch.arange(H) + 0.5, indexing="xy")
    plane = 1.0 / (0.45 - 0.002 * jj - 0.003 * ii)
    assert float(((depth - plane).abs() / plane)[covered].max()) < 1e-5


def test_barycentrics_and_depth_are_perspective_correct():
    """One triangle through K = [[60,0,32],[0,60,32],[0,0,1]] at 64 x 64: the world corners interpolated with bary re-project onto the
    pixel's own centre within 1e-3 px (screen-space barycentrics miss by up to 29 px), and depth is the re-projected z within 1e-5."""
    from arah_release_amd import meshing
    world = torch.tensor([[-1.2, -1.0, 1.2], [2.5, -0.8, 4.0], [-0.5, 2.0, 2.5]])
    K = torch.tensor([[60.0, 0.0, 32.0], [0.0, 60.0, 32.0], [0.0, 0.0, 1.0]])
    uvz = meshing.project_opencv(world, torch.eye(3), torch.zeros(3), K)
    p2f, depth, bary = meshing.mesh_rasterize(uvz, torch.tensor([[0, 1, 2]]), 64, 64)
    on = p2f >= 0
    assert int(on.sum()) > 500
    pt = bary[on].double() @ world.double()
    u, v = 60.0 * pt[:, 0] / pt[:, 2] + 32.0, 60.0 * pt[:, 1] / pt[:, 2] + 32.0
    ii, jj = torch.nonzero(on, as_tuple=True)
    miss = torch.maximum((u - (jj + 0.5)).abs(), (v - (ii + 0.5)).abs())
    print("re-projection misses the centre by at most %.3g px" % float(miss.max()))
    assert float(miss.max()) < 1e-3
    assert float(((depth[on].double() - pt[:, 2]).abs() / pt[:, 2]).max()) < 1e-5
    # the sign a face seen from its right-hand-normal side has under project_opencv: negative
    normal = torch.cross(world[1] - world[0], world[2] - world[0], dim=0)
    x, y = uvz[:, 0], uvz[:, 1]
    area2 = (x[1] - x[0]) * (y[2] - y[0]) - (x[2] - x[0]) * (y[1] - y[0])
    assert float((normal * world.mean(0)).sum()) * float(area2) > 0       # normal away from the camera <=> area2 > 0
    assert int((meshing.mesh_rasterize(uvz, torch.tensor([[0, 1, 2]]), 64, 64, cull="back" if area2 < 0 else "front")[0] >= 0).sum()) == 0


def test_render_mesh_on_the_host_and_its_argument_checks():
    from arah_release_amd import geometry, meshing
    verts, faces = grid_mesh(6, 3, False)
    world = torch.stack([(verts[:, 0] - 32) / 60 * verts[:, 2], (verts[:, 1] - 32) / 60 * verts[:, 2], verts[:, 2]], 1)
    cam = {"cam_rot": torch.eye(3), "cam_trans": torch.zeros(3), "K": torch.tensor([[60.0, 0, 32], [0, 60.0, 32], [0, 0, 1]])}
    colour = torch.rand(verts.shape[0], 3, generator=torch.Generator().manual_seed(2))
    res = geometry.render_mesh(world, faces, 64, 64, camera=cam, attributes={"colour": colour, "vertex_normal": True,
                                                                             "face_normal": True}, background=-2.0)
    assert set(res) == {"pix_to_face", "depth", "bary", "mask", "colour", "vertex_normal", "face_normal"}
    mask = res["mask"]
    assert mask.dtype == torch.bool and 2000 < int(mask.sum()) < 64 * 64 and torch.equal(mask, res["pix_to_face"] >= 0)
    uvz = geometry.project_mesh(world, cam, 64, 64)
    assert float((uvz - verts).abs().max()) < 1e-4
    assert_same((res["pix_to_face"], res["depth"], res["bary"]), meshing.mesh_rasterize(uvz, faces, 64, 64))
    assert torch.equal(res["colour"], meshing.interpolate_attributes(res["pix_to_face"], res["bary"], faces, colour, background=-2.0))
    assert bool((res["colour"][~mask] == -2.0).all()) and bool((res["face_normal"][~mask] == -2.0).all())
    flat = res["face_normal"][mask]
    assert float((flat.norm(dim=1) - 1).abs().max()) < 1e-6 and res["vertex_normal"].shape == (64, 64, 3)
    # a look-at view of the same call; a mesh behind the camera draws nothing
    look = geometry.render_mesh((world - world.mean(0)) * 0.2, faces, 48, 64, camera={"azim": 0.0, "dist": 2.5})
    assert 0 < int(look["mask"].sum()) < 48 * 64
    # "at" moves the camera with the point it looks at: the mesh moved by the same vector looks the same
    small, shift = (world - world.mean(0)) * 0.2, torch.tensor([0.25, -0.5, 0.125])
    moved = geometry.render_mesh(small + shift, faces, 48, 64, camera={"azim": 0.0, "dist": 2.5, "at": shift})
    assert int((moved["mask"] != look["mask"]).sum()) <= 2 and int(moved["mask"].sum()) > 0
    assert torch.equal(moved["bary"], geometry.render_mesh(small + shift, faces, 48, 64, camera={"azim": 0.0, "dist": 2.5, "at": (0.25, -0.5, 0.125)})["bary"])
    assert int(geometry.render_mesh(-world, faces, 64, 64, camera=cam)["mask"].sum()) == 0
    bad = [dict(verts=world[:, :2]), dict(verts=world.long()), dict(faces=faces.float()), dict(faces=faces[:, :2]), dict(camera=None),
           dict(camera={}), dict(camera={"cam_rot": torch.eye(3), "K": cam["K"]}), dict(camera=dict(cam, azim=0.0)),
           dict(camera={"dist": 2.0}), dict(camera={"azim": 0.0, "K": cam["K"]}), dict(camera={"azim": "front"}), dict(camera={"azim": 0.0, "at": (0.0, 1.0)}),
           dict(camera={"azim": 0.0, "at": torch.zeros(3, dtype=torch.int64)}), dict(camera={"at": (0.0, 0.0, 0.0)}),
           dict(camera=dict(cam, cam_trans=torch.zeros(4))), dict(cull="both"), dict(height=0), dict(width=2.5),
           dict(attributes={"colour": colour[:-1]}), dict(attributes={"colour": colour[:, 0]}), dict(attributes={"colour": True}),
           dict(attributes={"wide": torch.zeros(verts.shape[0], 33)}), dict(attributes={"depth": colour})]
    for kw in bad:
        args = dict(verts=world, faces=faces, height=64, width=64, camera=cam)
        args.update(kw)
        with pytest.raises(ValueError):
            geometry.render_mesh(**args)
    with pytest.raises(ValueError):
        meshing.mesh_rasterize(verts, faces, 64, 64, cull="sideways")
    with pytest.raises(ValueError):
        meshing.mesh_rasterize(verts.double(), faces, 64, 64)


def test_surface_centroid_does_not_depend_on_the_tessellation():
    from arah_release_amd import geometry
    verts, faces = grid_mesh(5, 1, False)
    flat = torch.cat([verts[:, :2], torch.zeros(verts.shape[0], 1)], 1)      # the rectangle [6,58] x [5,59], however it is cut
    for n, seed in ((5, 1), (17, 2), (40, 3)):
        v, f = grid_mesh(n, seed, False)
        c = geometry.surface_centroid(torch.cat([v[:, :2], torch.zeros(v.shape[0], 1)], 1), f)
        assert c.dtype == torch.float32 and float((c - torch.tensor([32.0, 32.0, 0.0])).abs().max()) < 1e-4
    # invalid faces and corners that are not numbers are left out; no area: the origin
    bad = torch.cat([faces, torch.tensor([[0, 1, 99], [0, 1, flat.shape[0]]])])
    withnan = torch.cat([flat, torch.tensor([[float("nan"), 0.0, 0.0]])])
    assert torch.equal(geometry.surface_centroid(withnan, bad), geometry.surface_centroid(flat, faces))
    assert torch.equal(geometry.surface_centroid(flat, faces[:0]), torch.zeros(3)) and torch.equal(geometry.surface_centroid(flat[:0], faces), torch.zeros(3))


# ---- GPU: the kernels against the rule ----------------------------------------------------------------------------------------------
def kernel(verts, faces, H, W, **kw):
    from arah_release_amd import hip
    return hip.mesh_rasterize(verts.to(DEV), faces.to(DEV), H, W, **kw)


@gpu
def test_kernel_equals_the_rule_on_the_same_device_tensors():
    """600 small faces at 96 x 128: the kernel against the rule running on the same GPU tensors, and that against the rule on the
    host; the three cull modes."""
    from arah_release_amd import meshing
    for cull in CULLS:
        verts, faces, want = spec("random600", random_set, 96, 128, cull=cull)
        dv, df = verts.to(DEV), faces.to(DEV)
        on_device = meshing.mesh_rasterize(dv, df, 96, 128, cull=cull)
        assert all(t.device.type == "cuda" for t in on_device)
        assert_same(on_device, want, "the rule, device against host, cull=%s" % cull)
        assert_same(kernel(verts, faces, 96, 128, cull=cull), on_device, "cull=%s" % cull)
    assert float((want[0] >= 0).float().mean()) > 0.2


@gpu
@pytest.mark.parametrize("at", (0, 63, 64, 300))
def test_kernel_draws_large_and_small_faces_of_one_wave(at):
    """Two image-covering faces and one whose bounding box reaches 1e5 px beyond the image, among 600 small ones, from face id `at`
    on: in the first lanes of a wave, across a wave boundary, at the start of one and in the middle.  Twice: the same bits."""
    verts, faces, want = spec("large%d" % at, lambda: with_large(at), 96, 128)
    assert bool((want[0] >= 0).all()) and {at, at + 1, at + 2} <= set(want[0].unique().tolist())
    got = kernel(verts, faces, 96, 128)
    assert_same(got, want, "at %d" % at)
    assert_same(kernel(verts, faces, 96, 128), got, "the second run")
    # every way of sharing the faces out -- lanes only, waves only, one workgroup a face, 64 a face, a mixture -- draws the same image
    big = 1 << 30
    for thresholds in ((big, big, big), (0, big, big), (0, 0, big), (0, 0, 0), (4, 32, 64)):
        assert_same(kernel(verts, faces, 96, 128, thresholds=thresholds), want, "thresholds %r" % (thresholds,))


@gpu
def test_kernel_on_small_meshes_and_images():
    from arah_release_amd import hip, meshing
    verts, faces = random_set(257, 64, 64, seed=9)
    for F in (0, 1, 63, 64, 65, 257):
        for H, W in ((1, 1), (37, 53), (64, 64)):
            want = meshing.mesh_rasterize(verts, faces[:F], H, W)
            assert_same(kernel(verts, faces[:F], H, W), want, "F %d at %d x %d" % (F, H, W))
            # a list holds H W ids: at 1 x 1 with every face sent to one, all but one find it full
            assert_same(kernel(verts, faces[:F], H, W, thresholds=(0, 0, 0)), want, "F %d at %d x %d, all huge" % (F, H, W))
            assert_same(kernel(verts, faces[:F], H, W, thresholds=(0, 0, 1 << 30)), want, "F %d at %d x %d, all medium" % (F, H, W))
    none = kernel(verts[:0], faces, 37, 53)                               # V = 0: every id is out of range
    assert_same(none, meshing.mesh_rasterize(verts[:0], faces, 37, 53), "V = 0")
    assert bool((none[0] == -1).all()) and bool((none[1] == -1).all()) and bool((none[2] == -1).all())
    for cull in CULLS:                                                     # the invalid faces
        hv, hf = handmade()
        assert_same(kernel(hv, hf, 12, 12, cull=cull), spec("handmade", handmade, 12, 12, cull=cull)[2], "handmade %s" % cull)
    for n, seed, half in ((40, 9, True), (17, 5, True)):                   # pixel centres exactly on vertices and edges
        gv, gf, want = spec("grid%d-%d-%d" % (n, seed, half), lambda: grid_mesh(n, seed, half), 64, 64)
        assert_same(kernel(gv, gf, 64, 64), want, "grid %d" % n)
    # bad arguments
    lib = hip.load_library()
    dv, df = verts.to(DEV), faces.to(torch.int32).to(DEV)
    keys = torch.empty(64 * 64, dtype=torch.int64, device=DEV)
    out = (torch.empty(64, 64, dtype=torch.int32, device=DEV), torch.empty(64, 64, device=DEV), torch.empty(64, 64, 3, device=DEV))
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(V=dv.shape[0], F=df.shape[0], H=64, W=64, cull=0, v=dv, f=df, k=keys, o=out):
        return lib.arah_mesh_rasterize(v if v is None else p(v), C.c_int64(V), f if f is None else p(f), C.c_int64(F), C.c_int32(H),
                                       C.c_int32(W), C.c_float(1e-4), C.c_int32(cull), k if k is None else p(k),
                                       *(t if t is None else p(t) for t in o), hip._stream(torch.device(DEV)))
    assert call() == 0
    for kw in (dict(V=-1), dict(F=-1), dict(H=0), dict(W=-3), dict(H=1 << 16, W=1 << 15), dict(cull=3), dict(cull=-1), dict(v=None),
               dict(f=None), dict(k=None), dict(o=(None, out[1], out[2])), dict(o=(out[0], None, out[2])), dict(o=(out[0], out[1], None)),
               dict(F=1 << 31)):
        assert call(**kw) == -1, kw
    assert call(F=0, f=None) == 0 and call(V=0, v=None) == 0
    torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize("n_ch", (1, 3, 4, 24))
def test_interpolation_kernel_equals_the_rule(n_ch):
    from arah_release_amd import hip, meshing
    verts, faces, (p2f, _, bary) = spec("large64", lambda: with_large(64), 96, 128)
    attr = (torch.rand(verts.shape[0], n_ch, generator=torch.Generator().manual_seed(n_ch)) * 4 - 2).float()
    want = meshing.interpolate_attributes(p2f, bary, faces, attr, background=0.5)
    got = hip.mesh_interpolate(p2f.to(DEV), bary.to(DEV), faces.to(DEV), attr.to(DEV), background=0.5)
    assert got.shape == (96, 128, n_ch) and torch.equal(bits(got), bits(want))
    odd = p2f.clone()                                                      # names no face: background
    odd[0, :4] = torch.tensor([-1, faces.shape[0], 2 ** 31 - 1, -7], dtype=torch.int32)
    want = meshing.interpolate_attributes(odd, bary, faces, attr)
    assert torch.equal(bits(hip.mesh_interpolate(odd.to(DEV), bary.to(DEV), faces.to(DEV), attr.to(DEV))), bits(want))
    with pytest.raises(ValueError):
        hip.mesh_interpolate(p2f.to(DEV), bary.to(DEV), faces.to(DEV), torch.zeros(verts.shape[0], 33, device=DEV))


@gpu
def test_public_call_on_the_host_equals_the_one_on_the_device():
    from arah_release_amd import geometry
    verts, faces = with_large(64)
    K = torch.tensor([[70.0, 0, 64], [0, 75.0, 48], [0, 0, 1]])
    rot = torch.tensor([[0.96, 0.0, 0.28], [0.0, 1.0, 0.0], [-0.28, 0.0, 0.96]])
    cam = {"cam_rot": rot, "cam_trans": torch.tensor([0.1, -0.2, 0.3]), "K": K}
    cam_space = torch.stack([(verts[:, 0] - 64) / 70 * verts[:, 2], (verts[:, 1] - 48) / 75 * verts[:, 2], verts[:, 2]], 1)
    world = (cam_space - cam["cam_trans"]) @ rot                          # x_cam = R x + t
    attrs = {"colour": torch.rand(verts.shape[0], 3, generator=torch.Generator().manual_seed(4)), "vertex_normal": True,
             "face_normal": True}
    for camera in (cam, {"azim": 180.0, "dist": 6.0, "fov": 70.0}, {"azim": 30.0, "dist": 6.0, "at": torch.tensor([0.5, -0.25, 1.0])}):
        for cull in ("none", "front"):
            host = geometry.render_mesh(world, faces, 96, 128, camera=camera, attributes=attrs, cull=cull, z_near=0.3, background=-1.0)
            dev = geometry.render_mesh(world.to(DEV), faces.to(DEV), 96, 128, attributes={k: v if v is True else v.to(DEV) for k, v in attrs.items()},
                                       camera={k: v.to(DEV) if torch.is_tensor(v) else v for k, v in camera.items()}, cull=cull,
                                       z_near=0.3, background=-1.0)
            assert set(host) == set(dev) and int(host["mask"].sum()) > (1000 if "K" in camera else 0)
            for k in host:
                assert dev[k].device.type == "cuda" and host[k].dtype == dev[k].dtype
                assert torch.equal(bits(host[k]), bits(dev[k])), (k, cull, sorted(camera))


# ---- GPU: the model's entry ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def subject(scene):
    dev = torch.device(DEV)
    model, _ = get_model("zju377_mono", dev)
    model.eval()
    return model, scene.make_inputs(64, 64, frame_idx=0, device=dev)


@gpu
def test_model_renders_its_posed_and_canonical_mesh(subject):
    from arah_release_amd import geometry, meshing
    model, inputs = subject
    H = W = 64
    with torch.no_grad():
        res = model.render_mesh(inputs, height=H, width=W, n_side=64, smooth=2)
    mesh, mask = res["mesh"], res["mask"]
    assert {"pix_to_face", "depth", "bary", "mask", "color", "vertex_normal", "mesh"} == set(res)
    assert {"verts", "faces", "verts_posed", "color"} <= set(mesh) and mesh["n_tris"] > 1000
    n_on = int(mask.sum())
    print("posed mask: %d of %d pixels" % (n_on, H * W))
    assert 0 < n_on < H * W
    colour = res["color"]
    # values of the colour network lie in [0, 1]; the three float32 weights sum to at most 1 + 3 * 2^-24
    assert bool(torch.isfinite(colour).all()) and float(colour[mask].min()) >= 0.0 and float(colour[mask].max()) <= 1.0 + 1e-6
    assert bool((colour[~mask] == 0.0).all()) and bool((res["vertex_normal"][~mask] == 0.0).all())
    # the interpolant of unit normals is shorter than 1 inside a face: unit length AFTER renormalising it, and not far from it before
    n = res["vertex_normal"][mask]
    length = n.norm(dim=1)
    assert float(length.min()) > 0.0 and float(length.max()) <= 1.0 + 1e-6
    assert float(((n / length[:, None]).norm(dim=1) - 1).abs().max()) < 1e-3
    posed_normals = geometry.vertex_normals(mesh["verts_posed"], mesh["faces"])
    assert torch.equal(res["vertex_normal"], geometry.render_mesh(
        mesh["verts_posed"], mesh["faces"], H, W, attributes={"n": posed_normals},
        camera={"cam_rot": inputs["cam_rot"][0], "cam_trans": inputs["cam_trans"][0].reshape(3), "K": inputs["intrinsics"][0]})["n"])
    # the posed vertices interpolated and re-projected land on the pixel's own centre
    pt = meshing.interpolate_attributes(res["pix_to_face"], res["bary"], mesh["faces"], mesh["verts_posed"].contiguous())
    uvz = meshing.project_opencv(pt[mask].double(), inputs["cam_rot"][0].double(), inputs["cam_trans"][0].reshape(3).double(),
                                 inputs["intrinsics"][0].double())
    ii, jj = torch.nonzero(mask, as_tuple=True)
    miss = torch.maximum((uvz[:, 0] - (jj + 0.5)).abs(), (uvz[:, 1] - (ii + 0.5)).abs())
    print("re-projection misses the centre by at most %.3g px" % float(miss.max()))
    assert float(miss.max()) < 1e-2
    assert float(((uvz[:, 2] - res["depth"][mask].double()).abs() / uvz[:, 2]).max()) < 1e-4
    with torch.no_grad():
        front = model.render_mesh(inputs, height=H, width=W, n_side=64, space="canonical", attributes=("face_normal", "normal"))
    assert front["face_normal"].shape == (H, W, 3) and front["normal"].shape == (H, W, 3) and 0 < int(front["mask"].sum()) < H * W
    assert "verts_posed" not in front["mesh"]
    for kw in (dict(space="world"), dict(attributes=("albedo",)), dict(view={"azim": 0}), dict(space="canonical", view={"K": 1})):
        with pytest.raises(ValueError):
            model.render_mesh(inputs, height=H, width=W, n_side=64, **kw)


def _canonical_masks(subject, **view):
    model, inputs = subject
    with torch.no_grad():
        front = model.render_mesh(inputs, height=64, width=64, n_side=64, smooth=2, space="canonical", view=dict(view, azim=0), attributes=())
        back = model.render_mesh(inputs, height=64, width=64, n_side=64, smooth=2, space="canonical", view=dict(view, azim=180), attributes=())
    a, b = front["mask"], back["mask"].flip(1)
    n_a, n_b = int(a.sum()), int(b.sum())
    print("canonical masks %r: front %d, back %d pixels, %d differ after mirroring" % (view, n_a, n_b, int((a != b).sum())))
    return n_a, n_b


@gpu
def test_canonical_front_and_back_masks_agree_from_far_away(subject):
    """The same framing from 20 x the distance (dist 40, tan(fov / 2) = tan(30 degrees) / 20): with the body at z in [-0.06, 0.29] the
    areas differ by at most (40.29 / 39.71)^2 - 1 = 3 % through perspective; the rest of the 5 % is for the pixels of the outline."""
    fov = 2.0 * math.degrees(math.atan(math.tan(math.radians(30.0)) / 20.0))
    n_a, n_b = _canonical_masks(subject, dist=40.0, fov=fov)
    assert 0 < n_a < 64 * 64 and abs(n_a - n_b) <= 0.05 * n_a


@gpu
def test_canonical_front_and_back_masks_have_equal_area(subject):
    """The default look-at view (dist 2, fov 60 degrees) from the front and from the back: mirrored masks of equal area within 5 %.
    The view looks at the centroid of the mesh's surface.  Measured on an MI355X: front 501, back 485 pixels of 64 x 64 (3.2 %), 28
    differ after mirroring.  A camera that looks at the origin instead, as the gen_cano_mesh maps do, sees 542 and 446 (18 %): the
    subject's normalised canonical body lies at z in [-0.06, 0.29], nearer to the front camera, and a silhouette's area goes with
    1 / depth^2; one that looks at the centre of the bounding box sees 471 and 509 (8 %), because what reaches z = 0.29 is little
    of the body."""
    n_a, n_b = _canonical_masks(subject)
    assert 0 < n_a < 64 * 64 and abs(n_a - n_b) <= 0.05 * n_a
