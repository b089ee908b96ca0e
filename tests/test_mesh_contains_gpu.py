"""Point-in-mesh for large meshes, on the device: arah_mesh_contains and arah_mesh_contains_grid (csrc/meshcontains.hpp) against the
specification meshing.mesh_contains bit for bit, edge sizes through the C entry, geometry.mesh_iou bracketed by counts of radii,
MetaAvatarRender.geometry_metrics(iou=N) and `validate --geometry-iou`."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from conftest import get_model
from test_geometry_metrics import icosphere
from test_mesh_contains import cube, f10, indexed

gpu = pytest.mark.gpu
DEV = "cuda:0"


def _points_around(verts, n, seed):
    """n float64 points in the mesh's box widened by a tenth, with a few that no box holds."""
    lo, hi = verts.double().amin(0), verts.double().amax(0)
    gen = torch.Generator().manual_seed(seed)
    pts = lo - 0.1 * (hi - lo) + torch.rand(n, 3, generator=gen, dtype=torch.float64) * 1.2 * (hi - lo)
    nan = float("nan")
    pts[:6] = torch.tensor([[nan, 0, 0], [0, nan, 0], [0, 0, nan], [1e30, 0, 0], [0, -1e30, 0], [float("inf"), 0, 0]], dtype=torch.float64)
    pts[6] = hi                      # q = resolution - 0.5 on every axis
    pts[7] = lo
    return pts


def _cases():
    verts, faces, points, _ = f10()
    out = {}
    for res in (512, 64, 8, 2):
        out["f10_%d" % res] = (verts, faces, points, res, res == 512)
    v, f = indexed(icosphere(2))
    gen = torch.Generator().manual_seed(0)
    out["icosphere"] = (v, f, torch.rand(20000, 3, generator=gen, dtype=torch.float64) * 2.2 - 1.1, 512, True)
    # two triangles over the whole xy extent: 512 x 512 cells each, the several-workgroups path of the build
    lo, hi = verts.amin(0), verts.amax(0)
    mid = float(lo[2] + hi[2]) / 2
    sheet = torch.tensor([[lo[0], lo[1], mid], [hi[0], lo[1], mid], [hi[0], hi[1], mid], [lo[0], hi[1], mid]], dtype=torch.float32)
    n = verts.shape[0]
    out["f10_sheet"] = (torch.cat([verts, sheet]), torch.cat([faces, torch.tensor([[n, n + 1, n + 2], [n, n + 2, n + 3]], dtype=torch.int32)]),
                        _points_around(verts, 6000, 1), 512, False)
    # a medium rectangle (workgroup path: 100 x 100 cells) and a wave one (20 x 20) beside the small ones
    ex = (hi - lo)
    def patch(frac):
        a = lo + 0.3 * ex
        b = a + torch.tensor([frac, 0.0, 0.0]) * ex
        c = a + torch.tensor([0.0, frac, 0.1]) * ex
        return torch.stack([a, b, c]).to(torch.float32)
    extra = torch.cat([patch(100 / 511), patch(20 / 511)])
    out["f10_patches"] = (torch.cat([verts, extra]), torch.cat([faces, torch.tensor([[n, n + 1, n + 2], [n + 3, n + 4, n + 5]], dtype=torch.int32)]),
                          _points_around(verts, 6000, 2), 512, False)
    # zero-area and vertical faces: the cube's walls are vertical; faces that repeat a vertex or lie on a line have no area
    cv, cf = cube(3.0)
    cv = torch.cat([cv, torch.tensor([[1.0, 1.0, 1.0], [2.0, 2.0, 2.0], [1.5, 1.5, 1.5]])])
    cf = torch.cat([cf, torch.tensor([[0, 0, 7], [8, 8, 8], [8, 10, 9], [1, 8, 1]], dtype=torch.int32)])
    out["degenerate_faces"] = (cv, cf, _points_around(cv, 3000, 3), 16, False)
    # the class edges and the remainder of the parts: six triangles in the unit cube whose rectangles hold exactly EDGE_CELLS cells
    ev, ef = cube(1.0)
    for k, (w, h) in enumerate(EDGE_RECTS):           # cell k of an axis has its centre at k / 511: the rectangle starts at cell 7 + k
        x0, y0, x1, y1 = (7 + k) / 511, (9 + k) / 511, (7 + k + w - 1) / 511, (9 + k + h - 1) / 511
        n = ev.shape[0]
        ev = torch.cat([ev, torch.tensor([[x0, y0, 0.25], [x1, y0, 0.5], [x0, y1, 0.75]])])
        ef = torch.cat([ef, torch.tensor([[n, n + 1, n + 2]], dtype=torch.int32)])
    assert rect_cells(ev, ef, 512)[12:] == list(EDGE_CELLS)
    out["class_edges"] = (ev, ef, _points_around(ev, 6000, 4), 512, False)
    return out


EDGE_RECTS = ((4, 4), (1, 17), (16, 32), (19, 27), (128, 256), (99, 331))     # 32769 = 99 x 331 is no multiple of the 64 parts
EDGE_CELLS = (16, 17, 512, 513, 32768, 32769)                                 # lane | wave | wave | medium | medium | huge


def rect_cells(verts, faces, res):
    """The cells of every face's clipped rectangle, by the rule's own rescaling (meshing.mesh_contains), on the host."""
    tri = verts.double()[faces.long()]
    lo, hi = tri.reshape(-1, 3).amin(0), tri.reshape(-1, 3).amax(0)
    scale = torch.full_like(lo, float(res - 1)) / (hi - lo)
    tri = scale * tri + (0.5 - scale * lo)
    r0 = tri[:, :, :2].amin(1).trunc().long().clamp(0, res - 1)
    r1 = tri[:, :, :2].amax(1).trunc().long().clamp(0, res - 1)
    return ((r1 - r0 + 1).prod(1)).tolist()


@pytest.fixture(scope="module")
def cases():
    """name -> the mesh and the points on the device, the specification's answer there (computed once), the index."""
    from arah_release_amd import hip, meshing
    dev = torch.device(DEV)
    out = {}
    for name, (v, f, p, res, brute) in _cases().items():
        v, f, p = v.to(dev), f.to(dev), p.to(dev)
        out[name] = {"verts": v, "faces": f, "points": p, "resolution": res, "brute": brute,
                     "spec": meshing.mesh_contains(v, f, p, res), "index": hip.contains_index(v, f, res)}
    return out


def _same(got, want, what):
    for g, w, field in zip(got, want, ("inside", "ambiguous", "tested")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, field)
        bad = torch.nonzero(g != w)[:, 0]
        assert bad.numel() == 0, "%s: %s differs at %d rows, first %s" % (what, field, bad.numel(), bad[:5].tolist())


CASES = ("f10_512", "f10_64", "f10_8", "f10_2", "icosphere", "f10_sheet", "f10_patches", "degenerate_faces", "class_edges")


# ------------------------------------------------------------------------------------------ 7. kernel == specification
@gpu
@pytest.mark.parametrize("name", CASES)
def test_kernel_equals_the_specification(cases, name):
    from arah_release_amd import hip, meshing
    c = cases[name]
    got = hip.mesh_contains(c["index"], c["points"], want_ambiguous=True, want_tested=True)
    _same(got, c["spec"], name)
    print("%s: %d references, inside %d, ambiguous %d, tested mean %.2f max %d" % (
        name, c["index"].n_refs, int(got[0].sum()), int(got[1].sum()), float(got[2].double().mean()), int(got[2].max())))
    assert c["index"].valid and c["index"].n_refs > 0
    # the optional outputs may be left out, float32 points are their float64 values
    alone = hip.mesh_contains(c["index"], c["points"])
    assert torch.equal(alone[0], got[0]) and alone[1] is None and alone[2] is None
    p32 = c["points"][:2000].float()
    _same(hip.mesh_contains(c["index"], p32, True, True), hip.mesh_contains(c["index"], p32.double(), True, True), name + " float32")
    _same(hip.mesh_contains(c["index"], p32, True, True), meshing.mesh_contains(c["verts"], c["faces"], p32, c["resolution"]), name + " f32 spec")
    if c["brute"]:     # where the host tests showed the specification and the brute force to agree
        if c["resolution"] == 512:
            assert torch.equal(hip.mesh_query(c["verts"], c["faces"], c["points"][:4096])[4], got[0][:4096])
    head = hip._contains_header(c["index"].buf)
    assert head["n_refs"] == c["index"].n_refs and head["n_faces"] == c["faces"].shape[0] and head["status"] == 0
    if name == "f10_sheet":
        assert head["n_huge"] == 2 and int(got[2][got[2] > 0].min()) >= 2
    if name == "f10_patches":
        assert head["n_med"] == 1 and head["n_huge"] == 0
    if name == "f10_2":
        assert head["n_huge"] == 0 and int(got[2].max()) == 1554
    if name == "class_edges":
        # the cube's four cap triangles cover all 512 x 512 cells, its eight wall triangles one row of 512; lane and wave classes
        # have no counter: that every cell of every rectangle was visited once is the reference count
        cells = rect_cells(c["verts"].cpu(), c["faces"].cpu(), 512)
        assert cells[:12] == [512 * 512] * 4 + [512] * 8
        assert head["n_med"] == sum(512 < n <= 1 << 15 for n in cells) == 2
        assert head["n_huge"] == sum(n > 1 << 15 for n in cells) == 5
        assert c["index"].n_refs == sum(cells)
    assert int(c["index"].refs.min()) >= 0 and int(c["index"].refs.max()) < c["faces"].shape[0]


@gpu
def test_degenerate_meshes_on_the_device(cases):
    from arah_release_amd import geometry, hip
    c = cases["f10_64"]
    v, f, p = c["verts"], c["faces"], c["points"]
    flat = v.clone()
    flat[:, 1] = 0.25
    poisoned = v.clone()
    poisoned[int(f[0, 0])] = float("nan")
    bad_id = f.clone()
    bad_id[5, 2] = v.shape[0]
    for vv, ff in ((v, f[:0]), (flat, f), (poisoned, f), (v, bad_id)):
        index = hip.contains_index(vv, ff, 64)
        assert not index.valid and index.n_refs == 0
        inside, ambiguous, tested = hip.mesh_contains(index, p, True, True)
        assert not bool(inside.any()) and not bool(ambiguous.any()) and int(tested.abs().sum()) == 0
        occ, amb = hip.mesh_contains_grid(index, p[:7, 0].float(), p[:5, 1].float(), p[:70, 2].float())
        assert not bool(occ.any()) and int(amb) == 0
    # the geometry layer: a soup or a pair, an index built earlier
    inside = geometry.mesh_contains((v, f), p, resolution=64)
    assert torch.equal(inside, c["spec"][0])
    both = geometry.mesh_contains((v, f), p, resolution=64, index=c["index"], return_ambiguous=True)
    assert torch.equal(both[0], c["spec"][0]) and torch.equal(both[1], c["spec"][1])
    assert torch.equal(geometry.mesh_contains(v[f.long()], p, resolution=64), c["spec"][0])
    with pytest.raises(ValueError):
        geometry.mesh_contains((v, f), p, resolution=512, index=c["index"])


# ------------------------------------------------------------------------------------------ 8. edge sizes
@gpu
def test_edge_sizes_through_the_c_entry(cases):
    from arah_release_amd import hip
    lib = hip.load_library()
    c = cases["f10_64"]
    index, dev = c["index"], torch.device(DEV)
    pad = 96
    for P in (0, 1, 63, 64, 65, 257):
        for dtype in (torch.float64, torch.float32):
            pts = torch.full((P + pad, 3), float("nan"), dtype=dtype, device=dev)
            pts[:P] = c["points"][100:100 + P].to(dtype)
            inside = torch.full((P + pad,), 0xAB, dtype=torch.uint8, device=dev)
            ambiguous = torch.full((P + pad,), 0xCD, dtype=torch.uint8, device=dev)
            tested = torch.full((P + pad,), -7, dtype=torch.int32, device=dev)
            with hip._on_device(dev):
                rc = lib.arah_mesh_contains(*index._head(), hip._ptr(pts), C.c_int32(1 if dtype == torch.float64 else 0), C.c_int32(P),
                                            hip._ptr(inside), hip._ptr(ambiguous), hip._ptr(tested), hip._stream())
            assert rc == 0, (P, rc)
            assert bool((inside[P:] == 0xAB).all()) and bool((ambiguous[P:] == 0xCD).all()) and bool((tested[P:] == -7).all()), P
            if dtype == torch.float64:
                want = [x[100:100 + P] for x in c["spec"]]
                _same((inside[:P].bool(), ambiguous[:P].bool(), tested[:P]), want, "P = %d" % P)
    with hip._on_device(dev):   # P = 0 with no buffers at all; a negative count; too many references
        assert lib.arah_mesh_contains(*index._head(), None, C.c_int32(1), C.c_int32(0), None, None, None, hip._stream()) == 0
        assert lib.arah_mesh_contains(*index._head(), None, C.c_int32(1), C.c_int32(-1), None, None, None, hip._stream()) == -1
        assert lib.arah_contains_index_fill(hip._ptr(index.buf), C.c_size_t(index.buf.numel()), C.c_int32(index.n_faces),
                                            C.c_int32(index.resolution), None, C.c_int64(2 ** 31), hip._stream()) == -6
        assert lib.arah_contains_index_fill(hip._ptr(index.buf), C.c_size_t(index.buf.numel() - 256), C.c_int32(index.n_faces),
                                            C.c_int32(index.resolution), hip._ptr(index.refs), C.c_int64(index.n_refs), hip._stream()) == -3
    # the index built twice gives equal answers (the order of the ids inside a cell may differ)
    again = hip.contains_index(c["verts"], c["faces"], 64)
    assert again.n_refs == index.n_refs
    _same(hip.mesh_contains(again, c["points"], True, True), c["spec"], "second index")
    assert torch.equal(torch.sort(again.refs).values, torch.sort(index.refs).values)


# ------------------------------------------------------------------------------------------ 9. the lattice kernel
@gpu
@pytest.mark.parametrize("dims", [(1, 1, 1), (5, 3, 70), (33, 17, 65), (2, 1, 4100)])
def test_grid_equals_the_point_kernel(cases, dims):
    from arah_release_amd import geometry, hip
    for name in ("f10_512", "f10_2"):
        c = cases[name]
        lo, hi = c["verts"].amin(0).cpu(), c["verts"].amax(0).cpu()
        # from a fifth of the extent before the box to a fifth behind it: coordinates outside the box on every axis (not for one cell)
        axes = [torch.linspace(float(lo[a] - 0.2 * (hi[a] - lo[a])), float(hi[a] + 0.2 * (hi[a] - lo[a])), dims[a])
                if dims[a] > 1 else ((lo[a] + hi[a]) / 2).reshape(1) for a in range(3)]
        axes = [x.float().to(DEV).contiguous() for x in axes]
        occ, amb = hip.mesh_contains_grid(c["index"], *axes)
        assert occ.shape == dims and occ.dtype == torch.bool and amb.dtype == torch.int64
        grid = torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1).reshape(-1, 3).contiguous()
        inside, ambiguous, _ = hip.mesh_contains(c["index"], grid, want_ambiguous=True)
        assert torch.equal(occ.reshape(-1), inside), (name, dims)
        assert int(amb) == int(ambiguous.sum()), (name, dims)
        if dims == (33, 17, 65):
            assert int(occ.sum()) > 0 and not bool(occ.all())
    c = cases["f10_512"]
    vox = geometry.voxelize((c["verts"], c["faces"]), dims=dims, padding=0.01, index=c["index"])
    grid = torch.stack(torch.meshgrid(vox["xs"], vox["ys"], vox["zs"], indexing="ij"), dim=-1).reshape(-1, 3).contiguous()
    assert torch.equal(vox["occupancy"].reshape(-1), hip.mesh_contains(c["index"], grid)[0]) and vox["occupancy"].shape == dims


# ------------------------------------------------------------------------------------------ 10. IoU of concentric icospheres
@gpu
def test_iou_of_concentric_icospheres_is_bracketed_by_radii():
    """Sphere of radius R as icosphere(2): every point with |p| < 0.98 R is inside (the inscribed radius is 0.9822 R), every point
    with |p| > R (1 + 2^-20) outside (the vertices are float32 roundings of points at distance R).  With A of radius 0.8 inside B
    of radius 1 (0.8 < 0.98): n_both = n_a, n_either = n_b, and all four counts lie between counts of the same samples' radii."""
    from arah_release_amd import geometry, meshing
    dev = torch.device(DEV)
    a, b = torch.from_numpy(icosphere(2, radius=0.8)).to(dev), torch.from_numpy(icosphere(2, radius=1.0)).to(dev)
    n = 100000
    res = geometry.mesh_iou(a, b, n_points=n, seed=1, return_points=True)
    r = res["points"].double().norm(dim=1)
    up = 1.0 + 2.0 ** -20
    lo_a, hi_a = int((r < 0.8 * 0.98).sum()), int((r <= 0.8 * up).sum())
    lo_b, hi_b = int((r < 0.98).sum()), int((r <= up).sum())
    n_a, n_b, n_both, n_either = (int(res[k]) for k in ("n_a", "n_b", "n_both", "n_either"))
    print("iou %.6f  n_a %d in [%d, %d]  n_b %d in [%d, %d]" % (float(res["iou"]), n_a, lo_a, hi_a, n_b, lo_b, hi_b))
    assert lo_a <= n_a <= hi_a and lo_b <= n_b <= hi_b and n_both == n_a and n_either == n_b
    assert lo_a / hi_b <= float(res["iou"]) <= hi_a / lo_b and float(res["iou"]) == n_both / n_either
    assert 0.45 < float(res["iou"]) < 0.56 and lo_a > 10000           # (0.8)^3 = 0.512 for the balls
    assert int(res["ambiguous_a"]) == 0 and int(res["ambiguous_b"]) == 0 and res["n_points"] == n
    assert float(res["volume_b"]) == n_b / n * 8.0 and float(res["volume_a"]) == n_a / n * 8.0      # the union's box is [-1, 1]^3
    for mesh, key in ((a, "inside_a"), (b, "inside_b")):
        v, f = mesh.reshape(-1, 3), torch.arange(mesh.shape[0] * 3, dtype=torch.int32, device=dev).reshape(-1, 3)
        assert torch.equal(res[key], meshing.mesh_contains(v, f, res["points"], 512)[0])
    again = geometry.mesh_iou(a, b, n_points=n, seed=1)
    assert all(torch.equal(torch.as_tensor(again[k]), torch.as_tensor(res[k])) for k in geometry.IOU_KEYS)
    other = geometry.mesh_iou(a, b, n_points=n, seed=2)
    assert int(other["n_a"]) != n_a


# ------------------------------------------------------------------------------------------ 11. model level
@gpu
def test_geometry_metrics_with_iou(scene):
    dev = torch.device(DEV)
    model, _ = get_model("zju377_mono", dev)
    model.eval()
    inputs = scene.make_inputs(32, 32, frame_idx=0, device=dev)
    with torch.no_grad():
        tris = model.posed_mesh(inputs, n_side=64)["tris"]
        plain = model.geometry_metrics(inputs, tris, n_side=64, n_samples=20000)
        own = model.geometry_metrics(inputs, tris, n_side=64, n_samples=20000, iou=20000)
        extent = tris.reshape(-1, 3).amax(0) - tris.reshape(-1, 3).amin(0)
        moved = model.geometry_metrics(inputs, tris + extent, n_side=64, n_samples=20000, iou=20000)
    new = {"iou"} | {"iou_" + k for k in ("n_a", "n_b", "n_both", "n_either", "ambiguous_a", "ambiguous_b", "volume_a", "volume_b", "n_points")}
    assert set(own) == set(plain) | new and not new & set(plain)
    assert all(torch.equal(torch.as_tensor(own[k]), torch.as_tensor(plain[k])) for k in plain)
    print("iou of the posed mesh with itself: %r, %d of %d points inside, %d ambiguous" % (
        float(own["iou"]), int(own["iou_n_a"]), own["iou_n_points"], int(own["iou_ambiguous_a"])))
    assert float(own["iou"]) == 1.0 and int(own["iou_n_a"]) == int(own["iou_n_both"]) > 100 and own["iou_n_points"] == 20000
    assert float(moved["iou"]) == 0.0 and int(moved["iou_n_both"]) == 0 and int(moved["iou_n_a"]) > 20 and int(moved["iou_n_b"]) > 20
    with pytest.raises(ValueError):
        model.geometry_metrics(inputs, tris.reshape(-1, 3), n_side=64, n_samples=20000, iou=1000)      # a scan has no volume


@gpu
def test_validate_with_geometry_iou(tmp_path, scene, monkeypatch):
    """validate --geometry DIR --geometry-iou N: one frame against its own posed mesh, one against a scan, one without ground truth."""
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
    for i in (0, 2):
        with torch.no_grad():
            mesh = lm.model.posed_mesh(lm.compose_inputs(val_ds.validation_item(i, dev), eval=True), n_side=64)
        verts = mesh["tris"].reshape(-1, 3).cpu().numpy()
        stem = os.path.splitext(os.path.basename(val_ds.data[i]["model_file"]))[0]
        if i == 0:
            np.savez(gt_dir / (stem + ".npz"), vertices=verts, faces=np.arange(len(verts)).reshape(-1, 3))
        else:
            np.savez(gt_dir / (stem + ".npz"), points=verts)
    lines = []
    common = ["--geometry", str(gt_dir), "--geometry-n-side", "64", "--geometry-samples", "5000"]
    validate.main(argv + common, body=body, faces=faces, log=lines.append)
    without = json.loads(lines[-1])
    frames_without = json.load(open(tmp_path / "out" / "validation.json"))["frames"]
    validate.main(argv + common + ["--geometry-iou", "5000"], body=body, faces=faces, log=lines.append)
    line = json.loads(lines[-1])
    print("validate --geometry-iou:", lines[-1])
    assert set(line) == set(without) | {"iou"} and "iou" not in without
    assert line["iou"] == 1.0 and line["n_geometry"] == 2
    assert all(line[k] == without[k] for k in without if k != "seconds_per_frame")
    frames = json.load(open(tmp_path / "out" / "validation.json"))["frames"]
    assert set(frames[0]) == set(frames_without[0]) | {"iou"} and frames[0]["iou"] == 1.0
    assert set(frames[2]) == set(frames_without[2]) and set(frames[1]) == set(frames_without[1]) and "iou" not in frames[2]
    with pytest.raises(ValueError):
        validate.main(argv + ["--geometry-iou", "5000"], body=body, faces=faces, log=lines.append)
