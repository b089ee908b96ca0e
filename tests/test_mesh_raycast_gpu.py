"""Casting rays against meshes on the device (csrc/meshray.hpp, DESIGN.md "Casting rays against meshes on the device"): the kernel
behind hip.mesh_raycast equals the specification meshing.mesh_raycast ON THE SAME DEVICE TENSORS bit for bit -- t, face and bary of
the first hit; mode "any" gives hit == (the specification's face >= 0) -- whatever the index's order of references, and the entries
of `geometry` and of the model built on it.  The cases and the host-side helpers are those of test_mesh_raycast.py."""
import math

import pytest
import torch

from conftest import get_model
from test_mesh_raycast import (DEPTH_TOL, F32, INF, NAN, T, assert_same, case_tensors, handmade_cases, in_plane_scene, random_scene,
                               raster_against_rays, sphere_rays, uv_sphere)

gpu = pytest.mark.gpu
DEV = "cuda"


def check(tris, o, d, index=None, what="", **kw):
    """kernel == specification on the device tensors, both modes; -> (the specification's result, the index)"""
    from arah_release_amd import hip, meshing
    tris, o, d = tris.to(DEV), o.to(DEV), d.to(DEV)
    index = hip.mesh_index(tris) if index is None else index
    spec = meshing.mesh_raycast(tris, o, d, **kw)
    got = hip.mesh_raycast(index, o, d, want_tested=True, **kw)
    assert_same(got, spec, what)
    hit, tested_any = hip.mesh_raycast(index, o, d, mode="any", want_tested=True, **kw)
    assert hit.dtype == torch.bool and torch.equal(hit, spec[1] >= 0), (what, "any")
    assert got[3].dtype == torch.int32 and bool((got[3] >= 0).all()) and bool((tested_any >= 0).all())
    return spec, index


@gpu
def test_kernel_equals_the_specification_on_the_handmade_set():
    from arah_release_amd import hip
    for case in handmade_cases():
        tris, o, d, kw = case_tensors(case)
        if case[0] == "nan_vertex":
            # an index cannot be built over a corner that is not finite: its status is 1 and EVERY ray misses, where the
            # specification only drops the faces concerned (test_an_index_with_status_1_misses_everything)
            continue
        spec, index = check(tris, o, d, what=case[0], **kw)
        assert index.header()["status"] == 0


@gpu
def test_kernel_equals_the_specification_on_rays_in_the_planes_of_faces():
    """Rays in the plane of a face, far beside it: det is rounding noise there.  All faces at once, and every seventh face alone
    (F = 1: one cell, and the ray usually misses the box)."""
    tris, o, d = in_plane_scene()
    for kw in ({"t_min": -INF}, {}, {"cull": "back", "t_min": -INF}):
        spec, _ = check(tris, o, d, what="in-plane " + str(kw), **kw)
        assert int((spec[1] >= 0).sum()) > 100
    per = o.shape[0] // tris.shape[0]
    for f in range(0, tris.shape[0], 7):
        check(tris[f:f + 1], o[f * per:(f + 1) * per], d[f * per:(f + 1) * per], what="in-plane, face %d alone" % f, t_min=-INF)


@gpu
def test_an_index_with_status_1_misses_everything():
    from arah_release_amd import hip
    case = [c for c in handmade_cases() if c[0] == "nan_vertex"][0]
    tris, o, d, kw = case_tensors(case, DEV)
    index = hip.mesh_index(tris)
    assert index.header()["status"] == 1
    t, face, bary, tested = hip.mesh_raycast(index, o, d, want_tested=True)
    assert bool((face == -1).all()) and bool(torch.isinf(t).all()) and bool((t > 0).all()) and bool((bary == 0).all())
    assert bool((tested == 0).all())
    assert not bool(hip.mesh_raycast(index, o, d, mode="any")[0].any())


def box_rays(hdr, n=4096, seed=1):
    """rays about the box of an index: origins inside, outside, 10^3 diagonals away, rays that miss the box, rays that graze a face
    of the box (they lie in the plane of the face)"""
    g = torch.Generator().manual_seed(seed)
    lo, hi = torch.tensor(hdr["lo"], dtype=torch.float64), torch.tensor(hdr["hi"], dtype=torch.float64)
    size, diag = hi - lo, float((hi - lo).norm())
    rnd = lambda *shape: torch.rand(*shape, generator=g, dtype=torch.float64)
    q = n // 8
    o, d = [], []
    # inside, any direction
    o.append(lo + rnd(2 * q, 3) * size)
    d.append(torch.randn(2 * q, 3, generator=g, dtype=torch.float64))
    # outside (on a shell 1 to 2 diagonals from the centre), aimed at a point of the box
    centre = 0.5 * (lo + hi)
    out = torch.randn(2 * q, 3, generator=g, dtype=torch.float64)
    out = centre + out / out.norm(dim=1, keepdim=True) * diag * (1.0 + rnd(2 * q, 1))
    o.append(out)
    d.append(lo + rnd(2 * q, 3) * size - out)
    # 10^3 diagonals away, aimed at the box; unit directions, so t is about 10^3 diagonals
    far = torch.randn(q, 3, generator=g, dtype=torch.float64)
    far = centre + far / far.norm(dim=1, keepdim=True) * diag * 1e3
    aim = lo + rnd(q, 3) * size - far
    o.append(far)
    d.append(aim / aim.norm(dim=1, keepdim=True))
    # rays that miss the box: outside and pointing away from the centre, or parallel to a face beside it
    away = torch.randn(q, 3, generator=g, dtype=torch.float64)
    away = away / away.norm(dim=1, keepdim=True)
    o.append(centre + away * diag)
    d.append(away + 0.3 * torch.randn(q, 3, generator=g, dtype=torch.float64))
    miss_from, miss_to = 5 * q, 6 * q
    # rays in the plane of a face of the box: one coordinate exactly lo or hi, no motion along it
    axis = torch.randint(0, 3, (2 * q,), generator=g)
    top = torch.randint(0, 2, (2 * q,), generator=g).bool()
    og = lo + (rnd(2 * q, 3) * 1.5 - 0.25) * size
    dg = torch.randn(2 * q, 3, generator=g, dtype=torch.float64)
    rows = torch.arange(2 * q)
    og[rows, axis] = torch.where(top, hi[axis], lo[axis])
    dg[rows, axis] = 0.0
    o.append(og)
    d.append(dg)
    return torch.cat(o).to(F32), torch.cat(d).to(F32), (miss_from, miss_to)


@pytest.fixture(scope="module")
def random_index():
    from arah_release_amd import hip
    tris = random_scene(600, 8, seed=0)[0].to(DEV)
    return tris, hip.mesh_index(tris)


@gpu
def test_kernel_equals_the_specification_on_random_faces(random_index):
    from arah_release_amd import hip
    tris, index = random_index
    hdr = index.header()
    assert hdr["status"] == 0 and hdr["n_refs"] > 600
    o, d, (m0, m1) = box_rays(hdr)
    assert o.shape[0] == 4096
    spec, _ = check(tris, o, d, index=index, what="random")
    share = float((spec[1] >= 0).float().mean())
    print("random faces: %.3f of the rays hit, grid %s, n_big %d" % (share, hdr["n"], hdr["n_big"]))
    assert 0.2 < share < 0.9
    # a ray that misses the box tests the big list and nothing else
    tested = hip.mesh_raycast(index, o.to(DEV), d.to(DEV), want_tested=True)[3]
    assert bool((spec[1][m0:m1] < 0).all()) and bool((tested[m0:m1] == hdr["n_big"]).all())
    # all three cull values, and windows of t that exclude the nearest face of many rays: the second has to be found
    t_first = spec[0][torch.isfinite(spec[0])]
    median = float(t_first.median())
    for kw in ({"cull": "back"}, {"cull": "front"}, {"t_min": median}, {"t_min": median, "t_max": 4.0 * median, "cull": "back"},
               {"t_max": median}, {"t_min": -INF}):
        s2, _ = check(tris, o, d, index=index, what=str(kw), **kw)
        if "t_min" in kw and kw["t_min"] > 0:
            moved = (spec[1] >= 0) & (spec[0] < median) & (s2[1] >= 0)
            assert int(moved.sum()) > 20, kw                       # rays whose nearest face is outside the window and which hit another


@gpu
def test_kernel_equals_the_specification_with_a_big_list():
    from arah_release_amd import hip
    tris = random_scene(600, 8, seed=0)[0]
    span = T([[[-1.2, -1.2, -1.1], [1.2, -1.1, 1.2], [-1.1, 1.2, 1.15]], [[1.2, 1.2, -1.2], [-1.2, 1.1, 1.2], [1.1, -1.2, 0.3]]])
    tris = torch.cat([tris[:300], span, tris[300:]]).to(DEV)
    index = hip.mesh_index(tris)
    hdr = index.header()
    assert hdr["n_big"] > 0
    o, d, (m0, m1) = box_rays(hdr, n=2048, seed=2)
    spec, _ = check(tris, o, d, index=index, what="big list")
    assert int(((spec[1] == 300) | (spec[1] == 301)).sum()) > 50
    tested = hip.mesh_raycast(index, o.to(DEV), d.to(DEV), want_tested=True)[3]
    assert bool((tested[m0:m1] == hdr["n_big"]).all())
    check(tris, o, d, index=index, what="big list, window", t_min=0.5, t_max=2.0, cull="front")


@gpu
def test_kernel_equals_the_specification_on_the_jittered_spheres():
    misses = 0
    for k in range(6):
        verts, faces, o, d = sphere_rays(k)
        spec, index = check(verts[faces], o, d, what="sphere %d" % k)
        misses += int((spec[1] < 0).sum())
        assert index.header()["n"][0] > 4
    assert misses == 0


@gpu
def test_kernel_equals_the_specification_on_a_fine_grid():
    """A shell of 36 480 small faces: a grid of some 30 cells a side, nearly all of them empty -- the walk crosses many slabs, jumps
    through the empty space by the distance transform, and ends on the best t long before the far side."""
    from arah_release_amd import hip
    verts, faces = uv_sphere(192, 96, jitter=0.01, seed=7)
    tris = verts[faces].to(DEV)
    index = hip.mesh_index(tris)
    hdr = index.header()
    print("fine grid: %s cells, %d references, n_big %d" % (hdr["n"], hdr["n_refs"], hdr["n_big"]))
    assert min(hdr["n"]) >= 24
    o, d, _ = box_rays(hdr, n=4096, seed=9)
    spec, _ = check(tris, o, d, index=index, what="fine grid")
    assert 0.3 < float((spec[1] >= 0).float().mean()) < 0.9       # the scene is neither empty nor a wall
    tested = hip.mesh_raycast(index, o.to(DEV), d.to(DEV), want_tested=True)[3]
    print("fine grid: mean tested %.1f, max %d of %d faces" % (float(tested.float().mean()), int(tested.max()), tris.shape[0]))
    assert float(tested.float().mean()) < tris.shape[0] / 20        # an index, not a list
    for kw in ({"t_min": 0.9, "cull": "front"}, {"t_min": 0.5, "t_max": 1.7, "cull": "back"}):
        check(tris, o, d, index=index, what="fine grid " + str(kw), **kw)
    # from the centre and from far outside through the vertices: every ray meets a shared vertex
    centre = torch.zeros(verts.shape[0], 3)
    check(tris, torch.cat([centre, verts * 3.0]), torch.cat([verts, -verts]), index=index, what="fine grid, vertices")


@gpu
def test_rays_in_cell_boundaries_and_through_cell_corners(random_index):
    tris, index = random_index
    hdr = index.header()
    lo, h, n = torch.tensor(hdr["lo"], dtype=torch.float64), hdr["h"], hdr["n"]
    o, d = [], []
    ks = lambda a: sorted({0, 1, 2, n[a] // 2, n[a] - 1, n[a]})
    for axis in range(3):                                   # along `axis`, lying in boundary planes of both other axes
        a, b = (axis + 1) % 3, (axis + 2) % 3
        for ka in ks(a):
            for kb in ks(b):
                for sign in (1.0, -1.0):
                    p = lo.clone()
                    p[a], p[b] = lo[a] + ka * h, lo[b] + kb * h
                    p[axis] = lo[axis] - h if sign > 0 else lo[axis] + (n[axis] + 1) * h
                    e = torch.zeros(3, dtype=torch.float64)
                    e[axis] = sign
                    o.append(p)
                    d.append(e)
                    e2 = e.clone()                          # ... and in the plane of one axis only, slanted in the other
                    e2[b] = 0.37 * sign
                    o.append(p)
                    d.append(e2)
    for kx in ks(0):                                        # through cell corners along (1,1,1) and its mirror images
        for ky in ks(1):
            for kz in ks(2):
                corner = lo + torch.tensor([kx, ky, kz], dtype=torch.float64) * h
                for e in ([1.0, 1.0, 1.0], [-1.0, -1.0, -1.0], [1.0, -1.0, 1.0]):
                    e = torch.tensor(e, dtype=torch.float64)
                    o.append(corner - 2.5 * h * e)
                    d.append(e)
    o, d = torch.stack(o).to(F32), torch.stack(d).to(F32)
    spec, _ = check(tris, o, d, index=index, what="cell boundaries")
    print("cell boundaries: %d rays, %d hit" % (o.shape[0], int((spec[1] >= 0).sum())))
    assert int((spec[1] >= 0).sum()) > o.shape[0] // 10
    check(tris, o, d, index=index, what="cell boundaries, culled", cull="back")


@gpu
def test_one_face_and_the_ray_counts_around_a_wave(random_index):
    from arah_release_amd import hip
    tri = T([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]])
    g = torch.Generator().manual_seed(5)
    o = torch.cat([torch.rand(200, 2, generator=g) * 1.4 - 0.2, torch.ones(200, 1)], dim=1)
    d = torch.cat([torch.randn(200, 2, generator=g) * 0.2, -torch.ones(200, 1)], dim=1)
    spec, index = check(tri, o, d, what="F = 1")
    assert index.header()["n_cells"] >= 1 and 20 < int((spec[1] == 0).sum()) < 200
    tris, index = random_index
    o, d, _ = box_rays(index.header(), n=128, seed=3)
    for R in (0, 1, 63, 64, 65):
        spec, _ = check(tris, o[:R], d[:R], index=index, what="R = %d" % R)
        assert spec[0].shape == (R,)
    for wg in (64, 128, 256):                               # the workgroup size changes nothing
        got = hip.mesh_raycast(index, o.to(DEV), d.to(DEV), workgroup=wg)
        assert_same(got, hip.mesh_raycast(index, o.to(DEV), d.to(DEV)), "workgroup %d" % wg)


@gpu
def test_argument_checks_on_the_device(random_index):
    from arah_release_amd import hip
    tris, index = random_index
    o, d = torch.zeros(4, 3, device=DEV), torch.ones(4, 3, device=DEV)
    bad = [lambda: hip.mesh_raycast(tris, o, d), lambda: hip.mesh_raycast(index, o.cpu(), d), lambda: hip.mesh_raycast(index, o, d[:3]),
           lambda: hip.mesh_raycast(index, o.double(), d), lambda: hip.mesh_raycast(index, o, d, mode="all"),
           lambda: hip.mesh_raycast(index, o, d, cull="both"), lambda: hip.mesh_raycast(index, o, d, t_min=NAN),
           lambda: hip.mesh_raycast(index, o, d, workgroup=32)]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail("call %d was accepted" % k)


# ---- geometry on the device against geometry on the host -------------------------------------------------------------------------
def dented_sphere():
    verts, faces = uv_sphere()
    verts = verts.clone()
    verts[100] *= 1.0 / 3.0
    return verts, faces


@gpu
def test_cast_rays_and_ambient_occlusion_equal_the_host():
    from arah_release_amd import geometry, hip, meshing
    verts, faces = dented_sphere()
    _, _, o, d = sphere_rays(0)
    o = torch.cat([o, o[:500] * 0.0 + T([0.0, 0.0, 3.0])])          # ... and from outside
    d = torch.cat([d, -d[:500] + T([0.0, 0.0, -3.0])])
    colour = torch.rand(verts.shape[0], 5, generator=torch.Generator().manual_seed(3))
    attrs = {"colour": colour, "vertex_normal": True}
    host = geometry.cast_rays((verts, faces), o, d, attributes=attrs, cull="back")
    index = hip.mesh_index(verts[faces].to(DEV))
    for idx in (None, index):
        dev = geometry.cast_rays((verts.to(DEV), faces.to(DEV)), o.to(DEV), d.to(DEV), attributes={"colour": colour.to(DEV), "vertex_normal": True},
                                 cull="back", index=idx)
        assert set(dev) == set(host)
        for k in host:
            assert dev[k].is_cuda and dev[k].dtype == host[k].dtype and dev[k].shape == host[k].shape, k
            assert_same((dev[k],), (host[k],), k)
    assert 0 < int(host["hit"].sum()) < o.shape[0]
    R = o.shape[0]
    for name, a in (("colour", colour), ("vertex_normal", geometry.vertex_normals(verts, faces))):
        want = meshing.interpolate_attributes(host["face"].reshape(1, R), host["bary"].float().reshape(1, R, 3), faces, a)[0]
        assert_same((dev[name],), (want,), name)
    assert torch.equal(geometry.occluded((verts.to(DEV), faces.to(DEV)), o.to(DEV), d.to(DEV), 0.0, 1.0).cpu(),
                       geometry.occluded((verts, faces), o, d, 0.0, 1.0))
    for kw in ({}, {"n_rays": 16, "seed": 4, "radius": 0.5}):
        ao_host = geometry.ambient_occlusion(verts, faces, **kw)
        ao_dev = geometry.ambient_occlusion(verts.to(DEV), faces.to(DEV), **kw)
        assert ao_dev.is_cuda and torch.equal(ao_dev.cpu(), ao_host), kw
        assert float(ao_host[100]) < 1.0 and float(ao_host.max()) == 1.0
    eye = T([0.5, -2.0, 2.5])
    assert torch.equal(geometry.vertex_visibility(verts.to(DEV), faces.to(DEV), eye.to(DEV)).cpu(), geometry.vertex_visibility(verts, faces, eye))


# ---- the model's entries ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def subject(scene):
    dev = torch.device(DEV)
    model, _ = get_model("zju377_mono", dev)
    model.eval()
    return model, scene.make_inputs(64, 64, frame_idx=0, device=dev)


@gpu
def test_model_casts_the_frames_rays_and_agrees_with_its_render(subject):
    from arah_release_amd import geometry
    model, inputs = subject
    H = W = 64
    with torch.no_grad():
        own = model.cast_rays(inputs, n_side=64, attributes=("color", "vertex_normal"))
        n = inputs["ray_dirs"][0].reshape(-1, 3).shape[0]
        assert own["t"].shape == (n,) and own["hit"].shape == (n,) and own["color"].shape == (n, 3) and own["vertex_normal"].shape == (n, 3)
        assert 0 < int(own["hit"].sum()) <= n and "mesh" in own
        camera = {"cam_rot": inputs["cam_rot"][0], "cam_trans": inputs["cam_trans"][0].reshape(3), "K": inputs["intrinsics"][0]}
        cast = model.cast_rays(inputs, rays=geometry.camera_rays(camera, H, W), n_side=64)
        raster = model.render_mesh(inputs, H, W, n_side=64, attributes=("ambient_occlusion",))
    assert torch.equal(cast["mesh"]["verts_posed"], raster["mesh"]["verts_posed"])
    cpu = lambda r: {k: v.cpu() for k, v in r.items() if isinstance(v, torch.Tensor)}
    bad, err, n_same, n_both = raster_against_rays(cpu(raster), cpu(cast), H, W)
    print("model: %d interior pixels, %d with the same face, largest |depth - t| %.3g, %d disagree" % (n_both, n_same, err, bad))
    assert n_both > 50 and n_same > 0.8 * n_both
    assert bad == 0
    assert err <= DEPTH_TOL
    ao = raster["ambient_occlusion"]
    assert ao.shape == (H, W, 1) and ao.dtype == F32 and bool(((ao >= 0) & (ao <= 1)).all())
    assert bool((ao[~raster["mask"]] == 0).all()) and float(ao.max()) > 0.5
    with pytest.raises(ValueError):
        model.cast_rays(inputs, n_side=64, attributes=("face_normal",))
    with pytest.raises(ValueError):
        model.cast_rays(inputs, rays=(inputs["ray_dirs"][0],), n_side=64)
