"""Generalized winding numbers on the device (DESIGN.md "Winding numbers on the device"): arah_winding_index_count / _fill against
the specification meshing.winding_tree table by table, arah_mesh_winding and arah_mesh_winding_grid (csrc/meshwinding.hpp) against
meshing.mesh_winding walking the device's own tables, the C entries on the test's own buffers, geometry.* with rule="winding",
MetaAvatarRender.geometry_metrics(inside="winding") and `validate --geometry-inside winding`."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from conftest import get_model
from test_mesh_contains import cube, f10
from test_mesh_sdf_gpu import _axes, _meshes, _same_bits

gpu = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")
NAMES = ("f10", "icosphere", "f10_open", "f10_zero_area", "f10_sheet", "cube")
DEPTHS = (0, 2, None)
ACCURACIES = (2.0, 3.0, INF)
DIMS = ((1, 1, 1), (5, 3, 70), (33, 17, 65))
# per exactly summed triangle: a term is at most 2 pi, w = sum / (4 pi) moves by at most 1/2 per term, and 2^-48 allows 16 ulp of
# it to the two atan2s (the device's and the host's); everything else of a term is correctly rounded on both sides
TERM_BOUND = 2.0 ** -48


def _mesh(name):
    if name == "cube":
        return cube()
    return _meshes()[name]


def _points(verts, faces):
    """2 000 seeded points in 1.5 x the bounds, the mesh's own vertices and its face centroids, float32."""
    lo, hi = verts.double().amin(0), verts.double().amax(0)
    mid, half = 0.5 * (lo + hi), 0.75 * (hi - lo)
    gen = torch.Generator().manual_seed(20)
    rnd = mid + (2.0 * torch.rand(2000, 3, dtype=torch.float64, generator=gen) - 1.0) * half
    tri = verts.double()[faces.long()]
    return torch.cat([rnd, verts.double(), tri.mean(1)]).to(torch.float32).contiguous()


_BUILT = {}


def _built(name, depth):
    """(index on the device, its tables as a host tree, the points) of one mesh at one depth, once."""
    key = (name, depth)
    if key not in _BUILT:
        from arah_release_amd import hip
        verts, faces = _mesh(name)
        index = hip.winding_index(verts.to(DEV), faces.to(DEV), depth)
        _BUILT[key] = (index, index.tree(), _points(verts, faces))
    return _BUILT[key]


@gpu
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("name", NAMES)
def test_build_equals_the_specification(name, depth):
    from arah_release_amd import meshing
    verts, faces = _mesh(name)
    index, got, _ = _built(name, depth)
    want = meshing.winding_tree(verts, faces, depth)
    assert index.depth == want.depth == meshing.check_winding_depth(depth, faces.shape[0])
    assert index.n_nodes == want.n_nodes and index.orient == want.orient and index.valid and want.valid
    assert index.side == want.side and index.lo == tuple(want.lo.tolist())
    assert np.float64(index.volume).tobytes() == np.float64(want.volume).tobytes()
    for field in ("order", "first", "count", "level", "skip"):
        assert torch.equal(getattr(got, field), getattr(want, field)), (name, depth, field)
    for field in ("tris", "nvec", "centroid", "radius", "area"):
        _same_bits(getattr(got, field), getattr(want, field), "%s depth %s: %s" % (name, depth, field))
    # the tree's own invariants: every triangle once, preorder, skips that close their subtrees
    assert sorted(got.order.tolist()) == list(range(faces.shape[0]))
    assert int(got.count[0]) == faces.shape[0] and int(got.skip[0]) == got.n_nodes
    assert bool((got.skip > torch.arange(got.n_nodes)).all())
    assert int(got.count[got.level == got.depth].sum()) == faces.shape[0]


@gpu
@pytest.mark.parametrize("accuracy", ACCURACIES)
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("name", NAMES)
def test_query_equals_the_specification_on_the_same_tables(name, depth, accuracy):
    from arah_release_amd import hip, meshing
    index, tree, pts = _built(name, depth)
    want_w, want_exact, want_far = meshing.mesh_winding(tree, pts, accuracy)
    w, inside, n_exact, n_far = hip.mesh_winding(index, pts.to(DEV), accuracy, want_counts=True)
    w, inside, n_exact, n_far = w.cpu(), inside.cpu(), n_exact.cpu(), n_far.cpu()
    assert w.dtype == torch.float64 and inside.dtype == torch.bool and n_exact.dtype == torch.int32 and n_far.dtype == torch.int32
    assert torch.equal(n_exact, want_exact) and torch.equal(n_far, want_far), (name, depth, accuracy)
    assert bool(((n_exact + n_far) >= 1).all())
    if accuracy == INF:
        assert bool((n_exact == tree.n_faces).all()) and bool((n_far == 0).all())
    assert bool(torch.isfinite(w).all()) and bool(torch.isfinite(want_w).all())
    diff, bound = (w - want_w).abs(), n_exact.double() * TERM_BOUND
    worst = float((diff / bound.clamp(min=TERM_BOUND)).max())
    print("%s depth %s accuracy %s: max |dw| = %.3g, %.3g of the bound; mean n_exact %.1f, n_far %.1f"
          % (name, depth, accuracy, float(diff.max()), worst, float(n_exact.double().mean()), float(n_far.double().mean())))
    assert bool((diff <= bound).all()), (name, depth, accuracy, float(diff.max()), worst)
    only_far = n_exact == 0
    _same_bits(w[only_far], want_w[only_far], "dipoles only")
    decided = (tree.orient * want_w - 0.5).abs() > bound
    assert torch.equal(inside[decided], meshing.winding_inside(want_w, tree.orient)[decided])
    # without the counts, and once more: the same bits
    again, inside2, none_a, none_b = hip.mesh_winding(index, pts.to(DEV), accuracy)
    assert none_a is None and none_b is None and torch.equal(inside2.cpu(), inside)
    _same_bits(again.cpu(), w, "two runs")


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_lattice_kernel_equals_the_point_kernel(name):
    from arah_release_amd import hip
    verts, _ = _mesh(name)
    lo, hi = verts.double().amin(0) - 0.05, verts.double().amax(0) + 0.05
    for depth in DEPTHS:
        index = _built(name, depth)[0]
        for dims in DIMS:
            axes, _ = _axes(lo, hi, dims, torch.device(DEV))
            grid = torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1).reshape(-1, 3).contiguous()
            for accuracy in ACCURACIES:
                w, occ, n_exact, n_far = hip.mesh_winding_grid(index, *axes, accuracy, want_counts=True)
                pw, pin, pe, pf = hip.mesh_winding(index, grid, accuracy, want_counts=True)
                assert tuple(w.shape) == dims and occ.dtype == torch.bool
                _same_bits(w.reshape(-1), pw, "%s %s %s %s" % (name, depth, dims, accuracy))
                assert torch.equal(occ.reshape(-1), pin) and torch.equal(n_exact.reshape(-1), pe) and torch.equal(n_far.reshape(-1), pf)
                w2, occ2, none_a, none_b = hip.mesh_winding_grid(index, *axes, accuracy)
                assert none_a is None and none_b is None and torch.equal(occ2, occ)
                _same_bits(w2, w, "two runs")


@gpu
def test_smallest_shapes_on_the_device():
    from arah_release_amd import hip, meshing
    dev = torch.device(DEV)
    pts = _points(*cube()).to(dev)
    # F = 0: no node, w = 0, nothing inside
    empty = hip.winding_index(torch.zeros(0, 3, device=dev), torch.zeros(0, 3, dtype=torch.int32, device=dev))
    assert empty.n_nodes == 0 and empty.n_faces == 0 and empty.orient == 1
    w, inside, n_exact, n_far = hip.mesh_winding(empty, pts, 3.0, want_counts=True)
    assert bool((w == 0).all()) and not bool(inside.any()) and not bool(n_exact.any()) and not bool(n_far.any())
    verts, faces = (x.to(dev) for x in cube())
    for depth in (0, meshing.WINDING_MAX_DEPTH):
        index = hip.winding_index(verts, faces, depth)
        tree = index.tree()
        for P in (0, 1, 65):
            w, inside, n_exact, n_far = hip.mesh_winding(index, pts[:P], INF, want_counts=True)
            assert tuple(w.shape) == (P,) and bool((n_exact == 12).all())
            want, _, _ = meshing.mesh_winding(tree, pts[:P].cpu(), INF)
            assert bool(((w.cpu() - want).abs() <= 12 * TERM_BOUND).all())
    # a vertex that is not finite: every winding number is NaN, nothing is inside
    bad = verts.clone()
    bad[3, 1] = float("nan")
    index = hip.winding_index(bad, faces)
    assert not index.valid
    w, inside, _, _ = hip.mesh_winding(index, pts)
    assert bool(torch.isnan(w).all()) and not bool(inside.any())
    # a point that is not finite
    index = hip.winding_index(verts, faces)
    nanp = pts[:3].clone()
    nanp[1, 2] = float("nan")
    w, inside, _, _ = hip.mesh_winding(index, nanp)
    assert bool(torch.isnan(w[1])) and not bool(inside[1]) and bool(torch.isfinite(w[[0, 2]]).all())
    # a face id outside [0, V), an index of another kind, a bad accuracy
    with pytest.raises(ValueError):
        hip.winding_index(verts, torch.tensor([[0, 1, 8]], dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        hip.mesh_winding(hip.contains_index(verts, faces, 64), pts)
    for accuracy in (0.5, float("nan"), "3"):
        with pytest.raises(ValueError):
            hip.mesh_winding(index, pts, accuracy)


@gpu
def test_an_index_from_another_mesh_is_refused():
    """The index of the cube handed in with F10, an index of F10 at another depth than the one asked for, and an index of another
    kind: every entry of geometry that takes index= refuses them."""
    from arah_release_amd import geometry, hip
    dev = torch.device(DEV)
    verts, faces, points, _ = f10()
    verts, faces, points = verts.to(torch.float32).to(dev), faces.to(dev), points.to(torch.float32).to(dev)[:100].contiguous()
    cv, cf = (x.to(dev) for x in cube())
    of_cube = hip.winding_index(cv, cf)
    own = hip.winding_index(verts, faces, 3)
    same_faces = hip.winding_index(torch.cat([verts, verts[:1]]), faces, 3)             # the same F, another V
    parity = hip.contains_index(verts, faces, 64)
    mesh = (verts, faces)
    for index in (of_cube, same_faces, parity, object()):
        for call in (lambda: geometry.winding_number(mesh, points, index=index),
                     lambda: geometry.mesh_contains(mesh, points, rule="winding", index=index),
                     lambda: geometry.mesh_sdf(mesh, points, rule="winding", contains_index=index),
                     lambda: geometry.voxelize(mesh, dims=(3, 4, 5), rule="winding", index=index),
                     lambda: geometry.mesh_sdf_grid(mesh, dims=(3, 4, 5), rule="winding", index=index)):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(ValueError):
        geometry.winding_number(mesh, points, depth=4, index=own)                       # built at depth 3
    with pytest.raises(ValueError):
        geometry.winding_number((cv, cf), points, index=own)
    # its own index is taken, with the depth it was built at or without one, and answers like a fresh one
    fresh = geometry.winding_number(mesh, points, depth=3)
    for kw in ({"index": own}, {"index": own, "depth": 3}):
        _same_bits(geometry.winding_number(mesh, points, **kw), fresh, "the mesh's own index")
    auto = hip.winding_index(verts, faces)                                               # the depth of the calls that build their own
    assert torch.equal(geometry.mesh_contains(mesh, points, rule="winding", index=auto), geometry.mesh_contains(mesh, points, rule="winding"))
    vox = geometry.voxelize(mesh, dims=(3, 4, 5), rule="winding", index=auto)
    _same_bits(vox["winding"], geometry.voxelize(mesh, dims=(3, 4, 5), rule="winding")["winding"], "voxelize with the mesh's own index")


@gpu
def test_a_leaf_cell_with_too_many_faces_is_refused():
    """Ranking a cell's faces is quadratic in the cell: more than WINDING_MAX_LEAF faces in one leaf cell at depth > 0 raise; the same
    mesh at depth 0, where nothing is ranked, and a mesh just at the limit build."""
    from arah_release_amd import hip, meshing
    dev = torch.device(DEV)
    n = meshing.WINDING_MAX_LEAF + 1
    gen = torch.Generator().manual_seed(5)
    lump = torch.rand(3 * n, 3, generator=gen) * 0.01                                      # n small triangles in one corner ...
    far = torch.tensor([[10.0, 10, 10], [10, 11, 10], [11, 10, 10]])                         # ... and one far away
    verts = torch.cat([lump, far]).to(dev)
    faces = torch.arange(3 * n + 3, dtype=torch.int32, device=dev).reshape(-1, 3)
    with pytest.raises(ValueError):
        hip.winding_index(verts, faces, 2)
    with pytest.raises(ValueError):
        hip.winding_index(verts, faces)
    flat = hip.winding_index(verts, faces, 0)
    assert flat.valid and flat.n_nodes == 1 and torch.equal(flat.order.cpu(), torch.arange(n + 1, dtype=torch.int32))
    at_limit = hip.winding_index(verts[3:], faces[:-1], 2)                                  # WINDING_MAX_LEAF faces in the cell
    leaves = at_limit.node_i[at_limit.node_i[:, 2] == 2, 1].cpu()
    assert at_limit.valid and sorted(leaves.tolist()) == [1, meshing.WINDING_MAX_LEAF]
    order = at_limit.order.cpu()
    assert torch.equal(order[:-1], torch.arange(meshing.WINDING_MAX_LEAF, dtype=torch.int32)) or torch.equal(
        order[1:], torch.arange(meshing.WINDING_MAX_LEAF, dtype=torch.int32))               # by face id inside the cell


@gpu
def test_c_entries_on_the_tests_own_buffers():
    from arah_release_amd import hip
    lib = hip.load_library()
    dev = torch.device(DEV)
    BADARG, WORKSPACE, OVERFLOW = (next(k for k, v in hip._ERRORS.items() if v == name)
                                   for name in ("ARAH_E_BADARG", "ARAH_E_WORKSPACE", "ARAH_E_OVERFLOW"))
    verts, faces = (x.to(dev) for x in cube())
    index = hip.winding_index(verts, faces, 2)
    pts = _points(*cube()).to(dev)[:65].contiguous()
    P = int(pts.shape[0])
    w = torch.full((P + 8,), -7.0, dtype=torch.float64, device=dev)
    head = index._head()

    def query(accuracy, n_pts=P, head=head):
        return lib.arah_mesh_winding(*head, hip._ptr(pts), C.c_int32(n_pts), C.c_double(accuracy), hip._ptr(w), None, None, None,
                                     hip._stream(dev))

    with hip._on_device(dev):
        assert query(3.0) == 0
        torch.cuda.synchronize()
        assert bool((w[P:] == -7.0).all()) and bool((w[:P] != -7.0).all())          # rows past P are never written
        assert [query(0.5), query(float("nan")), query(-2.0), query(0.0), query(3.0, n_pts=-1)] == [BADARG] * 5
        assert query(INF) == 0 and query(1.0) == 0 and query(3.0, n_pts=0) == 0
        over = list(head)
        over[7] = C.c_int64(2 ** 31)
        assert query(3.0, head=tuple(over)) == OVERFLOW
        short = list(head)
        short[1] = C.c_size_t(index.buf.numel() - 256)
        assert query(3.0, head=tuple(short)) == WORKSPACE
        size = lib.arah_winding_index_bytes
        assert size(C.c_int32(12), C.c_int32(8)) == 0 and size(C.c_int32(-1), C.c_int32(2)) == 0 and size(C.c_int32(12), C.c_int32(-2)) == 0
        assert size(C.c_int32(12), C.c_int32(-1)) == size(C.c_int32(12), C.c_int32(1))    # 8 < 12 <= 32: the rule gives depth 1
        axes = [torch.linspace(-0.2, 1.2, n, device=dev) for n in (3, 4, 5)]
        wg = torch.empty(3, 4, 5, dtype=torch.float64, device=dev)

        def lattice(accuracy, nz=5):
            return lib.arah_mesh_winding_grid(*head, hip._ptr(axes[0]), C.c_int32(3), hip._ptr(axes[1]), C.c_int32(4), hip._ptr(axes[2]),
                                              C.c_int32(nz), C.c_double(accuracy), hip._ptr(wg), None, None, None, hip._stream(dev))

        assert lattice(3.0) == 0
        assert lattice(0.5) == BADARG and lattice(3.0, nz=0) == BADARG
        assert lib.arah_winding_index_fill(*head[:5], None, None, C.c_int64(2 ** 31), hip._stream(dev)) == OVERFLOW
        assert lib.arah_winding_index_count(hip._ptr(verts), C.c_int32(8), hip._ptr(faces), C.c_int32(12), C.c_int32(9), hip._ptr(index.buf),
                                            C.c_size_t(index.buf.numel()), hip._ptr(index.order), hip._ptr(index.tris),
                                            hip._stream(dev)) == BADARG
    torch.cuda.synchronize()
    want = hip.mesh_winding_grid(index, *axes, 3.0)[0]
    _same_bits(wg, want, "the C entry on the test's own buffers")


@gpu
def test_geometry_with_the_winding_rule_equals_the_host_path():
    from arah_release_amd import geometry
    verts, faces, points, contains = f10()
    verts, points = verts.to(torch.float32), points.to(torch.float32)
    dev = torch.device(DEV)
    open_faces = _meshes()["f10_open"][1]
    w_host, e_host, f_host = geometry.winding_number((verts, open_faces), points, return_counts=True)
    w_dev, e_dev, f_dev = geometry.winding_number((verts.to(dev), open_faces.to(dev)), points.to(dev), return_counts=True)
    assert torch.equal(e_dev.cpu(), e_host) and torch.equal(f_dev.cpu(), f_host)
    assert bool(((w_dev.cpu() - w_host).abs() <= e_host.double() * TERM_BOUND).all())
    in_host, amb = geometry.mesh_contains((verts, open_faces), points, rule="winding", return_ambiguous=True)
    in_dev = geometry.mesh_contains((verts.to(dev), open_faces.to(dev)), points.to(dev), rule="winding")
    decided = (w_host.abs() - 0.5).abs() > 1e-9
    assert not bool(amb.any()) and torch.equal(in_dev.cpu()[decided], in_host[decided])
    agree = float((in_dev.cpu() == torch.from_numpy(contains)).double().mean())
    print("f10_open, rule='winding' against the closed mesh's contains: %.4f" % agree)
    assert agree >= 0.99
    # the dicts gain "winding"; the default calls keep their keys
    sdf = geometry.mesh_sdf((verts.to(dev), open_faces.to(dev)), points.to(dev), rule="winding")
    assert set(sdf) == set(geometry.SDF_KEYS) | {"winding"} and not bool(sdf["ambiguous"].any())
    assert torch.equal(sdf["inside"].cpu()[decided], in_host[decided]) and bool(((sdf["sdf"] < 0) == sdf["inside"])[sdf["d2"] > 0].all())
    assert set(geometry.mesh_sdf((verts.to(dev), faces.to(dev)), points.to(dev)[:10])) == set(geometry.SDF_KEYS)
    vox_dev = geometry.voxelize((verts.to(dev), open_faces.to(dev)), dims=(9, 7, 11), rule="winding", padding=0.05)
    vox_host = geometry.voxelize((verts, open_faces), dims=(9, 7, 11), rule="winding", padding=0.05)
    assert int(vox_dev["ambiguous"]) == 0 and tuple(vox_dev["winding"].shape) == (9, 7, 11)
    sure = (vox_host["winding"].abs() - 0.5).abs() > 1e-9
    assert torch.equal(vox_dev["occupancy"].cpu()[sure], vox_host["occupancy"][sure])
    field = geometry.mesh_sdf_grid((verts.to(dev), open_faces.to(dev)), dims=(9, 7, 11), padding=0.05, rule="winding")
    assert torch.equal(field["inside"], vox_dev["occupancy"]) and "winding" in field and int(field["ambiguous"]) == 0
    iou = geometry.mesh_iou((verts.to(dev), faces.to(dev)), (verts.to(dev), open_faces.to(dev)), n_points=20000, rule="winding")
    print("mesh_iou(closed F10, f10_open, rule='winding') = %.4f" % float(iou["iou"]))
    assert set(iou) == set(geometry.IOU_KEYS) | {"n_points", "winding"} and int(iou["ambiguous_a"]) == 0 and int(iou["ambiguous_b"]) == 0
    assert 0.9 <= float(iou["iou"]) <= 1.0
    for fn in (lambda: geometry.mesh_contains((verts, faces), points, rule="crossing"),
               lambda: geometry.mesh_iou((verts, faces), (verts, faces), rule=None),
               lambda: geometry.mesh_contains((verts, faces), points, rule="winding", accuracy=0.5)):
        with pytest.raises(ValueError):
            fn()


@gpu
def test_remesh_repairs_an_open_mesh():
    from arah_release_amd import geometry
    dev = torch.device(DEV)
    verts, faces = (x.to(dev) for x in _meshes()["f10_open"])
    topo = geometry.mesh_topology(verts, faces)
    assert not topo["watertight"]
    out_v, out_f = geometry.remesh((verts, faces), n_side=32, rule="winding")
    topo = geometry.mesh_topology(out_v, out_f)
    print("remesh(f10_open, n_side=32, rule='winding'): %d vertices, %d faces, %s" % (out_v.shape[0], out_f.shape[0], topo))
    assert topo["watertight"] and topo["euler"] == 2


@gpu
def test_geometry_metrics_with_the_winding_rule(scene):
    dev = torch.device(DEV)
    model, _ = get_model("zju377_mono", dev)
    model.eval()
    inputs = scene.make_inputs(32, 32, frame_idx=0, device=dev)
    with torch.no_grad():
        tris = model.posed_mesh(inputs, n_side=64)["tris"]
        open_tris = tris[torch.arange(tris.shape[0], device=dev) % 3 != 0].contiguous()          # a third of the faces removed
        parity = model.geometry_metrics(inputs, tris, n_side=64, n_samples=20000, iou=5000, sdf=5000)
        explicit = model.geometry_metrics(inputs, tris, n_side=64, n_samples=20000, iou=5000, sdf=5000, inside="parity")
        winding = model.geometry_metrics(inputs, tris, n_side=64, n_samples=20000, iou=5000, sdf=5000, inside="winding")
        opened = model.geometry_metrics(inputs, open_tris, n_side=64, n_samples=20000, iou=5000, sdf=5000, inside="winding")
    assert set(winding) == set(parity) == set(explicit)
    assert all(torch.equal(torch.as_tensor(explicit[k]), torch.as_tensor(parity[k])) for k in parity)
    print("posed 64^3 mesh against itself: iou parity %.4f, winding %.4f; against itself with a third of the faces removed, winding: "
          "iou %.4f, sdf_sign %.4f (closed: %.4f)" % (float(parity["iou"]), float(winding["iou"]), float(opened["iou"]),
                                                      float(opened["sdf_sign"]), float(winding["sdf_sign"])))
    for res in (winding, opened):
        assert int(res["iou_ambiguous_a"]) == 0 and int(res["iou_ambiguous_b"]) == 0 and int(res["sdf_ambiguous"]) == 0
        assert 0.0 <= float(res["iou"]) <= 1.0 and 0.0 <= float(res["sdf_sign"]) <= 1.0 and np.isfinite(float(res["sdf_l1"]))
    assert float(winding["iou"]) == 1.0          # the same soup twice: the same winding numbers
    with pytest.raises(ValueError):
        model.geometry_metrics(inputs, tris, n_side=64, n_samples=20000, iou=100, inside="crossing")


@gpu
def test_validate_with_geometry_inside_winding(tmp_path, scene, monkeypatch):
    """validate --geometry DIR --geometry-iou N --geometry-sdf N --geometry-inside winding: one frame against its own posed mesh, one
    against a scan, one without ground truth."""
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
    common = ["--geometry", str(gt_dir), "--geometry-n-side", "64", "--geometry-samples", "5000", "--geometry-iou", "5000",
              "--geometry-sdf", "5000", "--geometry-sdf-band", "0.04"]
    validate.main(argv + common, body=body, faces=faces, log=lines.append)
    parity = json.loads(lines[-1])
    validate.main(argv + common + ["--geometry-inside", "parity"], body=body, faces=faces, log=lines.append)
    explicit = json.loads(lines[-1])
    validate.main(argv + common + ["--geometry-inside", "winding"], body=body, faces=faces, log=lines.append)
    line = json.loads(lines[-1])
    print("validate --geometry-inside winding:", lines[-1])
    assert "geometry_inside" not in parity and set(explicit) == set(parity)
    assert all(explicit[k] == parity[k] for k in parity if k != "seconds_per_frame")
    assert set(line) == set(parity) | {"geometry_inside"} and line["geometry_inside"] == "winding"
    assert line["iou"] == 1.0 and 0.0 <= line["sdf_sign"] <= 1.0 and 0.0 <= line["sdf_l1"] < 2.0 * 0.04 and line["n_geometry"] == 2
    unchanged = [k for k in parity if k not in ("seconds_per_frame", "iou", "sdf_l1", "sdf_sign")]
    assert all(line[k] == parity[k] for k in unchanged)
    with pytest.raises(ValueError):
        validate.main(argv + ["--geometry-inside", "winding"], body=body, faces=faces, log=lines.append)
    with pytest.raises(SystemExit):
        validate.main(argv + common + ["--geometry-inside", "crossing"], body=body, faces=faces, log=lines.append)
