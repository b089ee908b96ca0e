"""The kernels behind geometry.isotropic_remesh against their tensor specifications, bit for bit: the tangential step
(arah_mesh_tangential) and the bounded collapse round (arah_mesh_collapse_round_bounded), round after round until none is applied;
the whole remesher on device tensors against the same call on the host; smooth_mesh(method="tangential"); empty inputs; and the
model's posed_mesh with isotropic=."""
import numpy as np
import pytest
import torch

from test_mesh_collapse import same_bits as collapse_same_bits
from test_mesh_flip import mesh
from test_mesh_isotropic import edge_bounds, remeshed

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MESHES = ("octahedron", "flat_bipyramid", "sheet", "three_faces", "misoriented", "nan_vertex", "bad_ids", "open_sphere", "bicone40",
          "jgrid9_0", "jgrid33_1", "sphere33", "f10")


def bits(t):
    t = t.cpu()
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64) if t.dtype == torch.float64 else t


@pytest.mark.parametrize("name", MESHES)
def test_tangential_kernel_is_the_specification(name):
    from arah_release_amd import geometry, hip, meshing
    verts, faces = mesh(name)
    dv, df = verts.to(DEV), faces.to(DEV)
    v, d = verts, dv
    for step, lamb in enumerate((0.5, 1.0, 0.3)):                                 # three steps, each from the one before
        ns, dns = meshing.vertex_normals(v, faces)[0], hip.vertex_normals(d, df)[0]
        assert torch.equal(bits(dns), bits(ns))
        v, d = meshing.mesh_tangential_step(v, faces, ns, lamb), hip.mesh_tangential_step(d, df, dns, lamb)
        assert d.dtype == torch.float32 and torch.equal(bits(d), bits(v)), (name, step)
    got = geometry.smooth_mesh(dv, df, iterations=2, method="tangential")
    assert got.is_cuda and torch.equal(bits(got), bits(geometry.smooth_mesh(verts, faces, iterations=2, method="tangential")))


@pytest.mark.parametrize("name", MESHES)
def test_bounded_collapse_rounds_are_the_specification_until_none_is_applied(name):
    from arah_release_amd import hip, meshing
    verts, faces = mesh(name)
    short2, long2 = edge_bounds(name)
    v, f, dv, df = verts, faces, verts.to(DEV), faces.to(DEV).to(torch.int32)
    applied = []
    for _ in range(32):
        want = meshing.mesh_collapse_round(v, f, 10 ** 6, details=True, short_len2=short2, long_len2=long2)
        got = hip.mesh_collapse_round(dv, df, 10 ** 6, details=True, short_len2=short2, long_len2=long2)
        collapse_same_bits(got, want, (name, "round", len(applied)), n=8)
        c = dict(zip(meshing.COLLAPSE_BOUNDED_COUNTS, want[4].tolist()))
        applied.append(c["applied"])
        if c["applied"] == 0:
            break
        v, f = want[0][:c["n_verts"]], want[1][:c["n_faces"]].long()
        dv, df = got[0][:c["n_verts"]], got[1][:c["n_faces"]]
    assert applied[-1] == 0 and (name not in ("sphere33", "f10", "open_sphere") or (sum(applied) > 0 and c["not_short"] > 0))
    # one bound alone, and none: the existing entry, twelve counts
    for kw in ({"short_len2": short2}, {"long_len2": long2}, {}):
        collapse_same_bits(hip.mesh_collapse_round(verts.to(DEV), faces.to(DEV), 7, details=True, **kw),
                           meshing.mesh_collapse_round(verts, faces, 7, details=True, **kw), (name, kw), n=8)


def test_empty_meshes_write_their_counts():
    from arah_release_amd import hip, meshing
    verts, faces = mesh("octahedron")
    dv, df = verts.to(DEV), faces.to(DEV)
    for v, f, hv, hf in ((dv[:0], df[:0], verts[:0], faces[:0]), (dv, df[:0], verts, faces[:0]), (dv[:0], df, verts[:0], faces)):
        collapse_same_bits(hip.mesh_collapse_round(v, f, 3, details=True, short_len2=1.0, long_len2=2.0),
                           meshing.mesh_collapse_round(hv, hf, 3, details=True, short_len2=1.0, long_len2=2.0), (v.shape, f.shape), n=8)
        ns = torch.zeros(hv.shape[0], 3, dtype=torch.float64)
        assert torch.equal(bits(hip.mesh_tangential_step(v, f, ns.to(DEV))), bits(meshing.mesh_tangential_step(hv, hf, ns)))


def same_remesh(res, ref, what):
    assert res["verts"].is_cuda and res["faces"].dtype == ref["faces"].dtype and (res["n_verts"], res["n_tris"]) == (ref["n_verts"], ref["n_tris"])
    for key in ("verts", "faces", "src_face", "src_bary", "w", "label"):
        assert torch.equal(bits(res[key]), bits(ref[key])), (what, key)
    assert res["report"] == ref["report"], what


def test_remesh_on_the_device_is_the_remesh_on_the_host_sphere():
    from arah_release_amd import geometry
    ref, attrs = remeshed("sphere33")
    verts, faces = mesh("sphere33")
    res = geometry.isotropic_remesh(verts.to(DEV), faces.to(DEV), iterations=5, attributes={k: t.to(DEV) for k, t in attrs.items()})
    same_remesh(res, ref, "sphere33")
    topo = geometry.mesh_topology(res["verts"], res["faces"])
    assert topo["watertight"] and topo["manifold"] and topo["euler"] == 2


def test_remesh_on_the_device_is_the_remesh_on_the_host_f10():
    from arah_release_amd import geometry
    verts, faces = mesh("f10")
    attrs = {"w": verts.double() * 3.0, "label": torch.arange(verts.shape[0])}
    kw = {"iterations": 2, "edge_length": 1.5 * geometry.mesh_quality(verts, faces)["edge_mean"]}
    ref = geometry.isotropic_remesh(verts, faces, attributes=attrs, **kw)
    res = geometry.isotropic_remesh(verts.to(DEV), faces.to(DEV), attributes={k: t.to(DEV) for k, t in attrs.items()}, **kw)
    same_remesh(res, ref, "f10")
    assert res["n_tris"] < faces.shape[0] and geometry.mesh_topology(res["verts"], res["faces"])["euler"] == 2


@pytest.fixture(scope="module")
def subject(scene):
    from conftest import get_model
    dev = torch.device(DEV)
    model, _ = get_model("zju377_mono", dev)
    model.eval()
    return model, scene.make_inputs(32, 32, frame_idx=0, device=dev)


def test_posed_mesh_remeshed_is_manifold_and_watertight(subject):
    from arah_release_amd import geometry
    model, inputs = subject
    with torch.no_grad():
        plain = model.posed_mesh(inputs, n_side=64, indexed=True, clean="largest")
        fine = model.posed_mesh(inputs, n_side=64, indexed=True, clean="largest", isotropic={"iterations": 3})
    before, after = geometry.mesh_topology(plain["verts"], plain["faces"]), geometry.mesh_topology(fine["verts"], fine["faces"])
    assert after["watertight"] and after["manifold"] and after["euler"] == before["euler"] and before["watertight"]
    rep = fine["isotropic"]["report"]
    print("posed mesh at 64^3: %d -> %d faces; edges in range %.3f -> %.3f; angles below 30 degrees %.3f -> %.3f"
          % (plain["n_tris"], fine["n_tris"], rep["before"]["edges_in_range"], rep["after"]["edges_in_range"],
             rep["before"]["small_angle_share"], rep["after"]["small_angle_share"]))
    assert rep["after"]["edges_in_range"] > rep["before"]["edges_in_range"]
    assert rep["after"]["small_angle_share"] < rep["before"]["small_angle_share"]
    assert fine["verts"].shape == (fine["n_verts"], 3) and fine["isotropic"]["src_face"].shape == (fine["n_verts"],)
    assert int(fine["isotropic"]["src_face"].max()) < plain["n_tris"] and bool(torch.isfinite(fine["verts"]).all())
    with pytest.raises(ValueError):
        model.posed_mesh(inputs, n_side=64, isotropic=0.01)
    with torch.no_grad():
        canon = model.canonical_mesh(inputs, n_side=64, clean="largest", isotropic={"iterations": 1}, attributes=("color",))
    assert canon["color"].shape == (canon["n_verts"], 3) and bool(torch.isfinite(canon["color"]).all()) and "isotropic" in canon
