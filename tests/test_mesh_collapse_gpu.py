"""The kernels of csrc/meshcollapse.hpp (arah_mesh_collapse_round) against their tensor specification
meshing.mesh_collapse_round, bit for bit in every output, counter and per-edge table, on the meshes of
tests/test_mesh_collapse.py; geometry.decimate_mesh on device tensors against the same loop over the specification after every
round; the C entry on buffers of the test's own; and the model's entries with simplify={"method": "collapse", ...}."""
import ctypes as C

import pytest
import torch

from test_mesh_collapse import NAMES, counts_of, mesh, same_bits, shaped, spec

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x5A
PAD = 5
# closed surfaces of one and two components and of genus 1, a rim of pinned vertices, an edge with three faces, a vertex that
# is not a number, ids out of range and a repeated id, two apexes with forty faces each (more than a lane's tree holds), the
# smallest closed meshes; no face count here is a multiple of the workgroup's 256 or of the compaction's chunk of 1024
CASES = ("sphere17", "sphere33", "torus", "two_spheres", "sheet", "grid8", "three_faces", "nan_vertex", "bad_ids", "bicone40",
         "tetrahedron", "octahedron", "bipyramid")


def run(name, need=10 ** 6, reg=1e-3, max_cost=float("inf"), faces_dtype=torch.int32):
    from arah_release_amd import hip
    verts, faces = mesh(name)
    return hip.mesh_collapse_round(verts.to(DEV), faces.to(DEV).to(faces_dtype), need, reg, max_cost, details=True)


@pytest.mark.parametrize("name", CASES)
def test_kernels_are_the_specification(name):
    want = spec(name)
    first = run(name)
    same_bits(first, want, name, n=8)
    c = counts_of(want)
    if name == "bicone40":
        assert c["long_edges"] == 80 and c["candidates"] > 0
    if name in ("sheet", "grid8", "three_faces", "nan_vertex"):
        assert c["pinned"] > 0
    if name in ("sphere33", "torus"):
        assert c["flips"] > 0 and c["applied"] > 64                               # more than one wave of collapses
    if name in ("sphere17", "sphere33", "torus", "two_spheres", "sheet", "bad_ids"):
        assert c["applied"] > 0 and mesh(name)[1].shape[0] % 256 != 0
    # again, from faces of another integer type: the order of arrival does not show
    same_bits(run(name, faces_dtype=torch.int64), first, (name, "again"), n=8)


@pytest.mark.parametrize("kind", ["whole_waves", "isolated"])
def test_whole_waves_of_entries_and_isolated_vertices(kind):
    from arah_release_amd import hip, meshing
    verts, faces = shaped(kind)
    adj = meshing.mesh_adjacency(faces, verts.shape[0])
    assert (int(adj[2][-1]) % 64 == 0) == (kind == "whole_waves") and (int(adj[7][6]) == 2) == (kind == "isolated")
    for bounds in ({}, {"short_len2": 1.5, "long_len2": 9.0}):
        want = meshing.mesh_collapse_round(verts, faces, 10 ** 6, details=True, **bounds)
        same_bits(hip.mesh_collapse_round(verts.to(DEV), faces.to(DEV), 10 ** 6, details=True, **bounds), want, (kind, bounds), n=8)


@pytest.mark.parametrize("need", [0, 1, 7, 10 ** 6])
def test_cap_keeps_the_first_selected_edges(need):
    want = spec("sphere17", need)
    same_bits(run("sphere17", need), want, need, n=8)
    c = counts_of(want)
    assert c["selected"] > 7 and c["applied"] == min(need, c["selected"]) and c["n_faces"] == mesh("sphere17")[1].shape[0] - 2 * c["applied"]


@pytest.mark.parametrize("reg,max_cost", [(0.0, float("inf")), (0.5, float("inf")), (1e-3, 0.0), (1e-3, 1e-9)])
def test_other_regularisers_and_bounds(reg, max_cost):
    for name in ("sphere17", "sheet"):
        same_bits(run(name, 10 ** 6, reg, max_cost), spec(name, 10 ** 6, reg, max_cost), (name, reg, max_cost), n=8)
    if max_cost == 1e-9:
        assert 0 < counts_of(spec("sphere17", 10 ** 6, reg, max_cost))["over_error"]


def test_empty_meshes_write_their_counts():
    from arah_release_amd import hip, meshing
    verts, faces = mesh("octahedron")
    dv, df = verts.to(DEV), faces.to(DEV)
    for v, f, hv, hf in ((dv[:0], df[:0], verts[:0], faces[:0]), (dv, df[:0], verts, faces[:0]), (dv[:0], df, verts[:0], faces)):
        same_bits(hip.mesh_collapse_round(v, f, 3, details=True), meshing.mesh_collapse_round(hv, hf, 3, details=True),
                  (v.shape, f.shape), n=8)


def test_entry_writes_its_arrays_and_nothing_else():
    from arah_release_amd import hip
    verts, faces = mesh("bad_ids")
    want = spec("bad_ids")
    verts, f32 = verts.to(DEV), faces.to(DEV).to(torch.int32).contiguous()
    lib = hip.load_library()
    V, F = verts.shape[0], f32.shape[0]

    def buf(nbytes):
        return torch.full((nbytes + PAD,), SENTINEL, dtype=torch.uint8, device=DEV)
    sizes = (V * 12, F * 12, V * 4, F * 4, 12 * 4, 6 * F * 12, 6 * F * 8, 6 * F)
    with hip._on_device(verts.device):
        scratch = hip._mesh_cc_buf(verts.device, int(lib.arah_mesh_collapse_round_scratch_bytes(V, F)))
        for nbytes, rc_want in ((16, -3), (scratch.numel(), 0)):                  # ARAH_E_WORKSPACE launches nothing
            bufs = [buf(n) for n in sizes]
            rc = lib.arah_mesh_collapse_round(hip._ptr(verts), C.c_int64(V), hip._ptr(f32), C.c_int64(F), C.c_int32(10 ** 6),
                                              C.c_double(1e-3), C.c_float(float("inf")), *[hip._ptr(b) for b in bufs],
                                              hip._ptr(scratch), C.c_size_t(nbytes), hip._stream())
            torch.cuda.synchronize()
            assert rc == rc_want
            if rc:
                assert all(bool((b == SENTINEL).all()) for b in bufs)
    for b, n in zip(bufs, sizes):
        assert bool((b[n:] == SENTINEL).all())
    kinds = (torch.float32, torch.int32, torch.int32, torch.int32, torch.int32, torch.float32, torch.int64, torch.uint8)
    shapes = ((V, 3), (F, 3), (V,), (F,), (12,), (6 * F, 3), (6 * F,), (6 * F,))
    got = [b[:n].view(k).reshape(s) for b, n, k, s in zip(bufs, sizes, kinds, shapes)]
    same_bits(got, want, "raw entry", n=8)


def test_decimate_on_the_device_is_the_specification_after_every_round():
    from arah_release_amd import geometry, hip, meshing
    verts, faces = mesh("sphere33")
    target = faces.shape[0] // 8
    v, f = verts, faces
    dv, df = verts.to(DEV), faces.to(DEV).to(torch.int32)
    history = [faces.shape[0]]
    while f.shape[0] > target:
        need = (f.shape[0] - target + 1) // 2
        want, got = meshing.mesh_collapse_round(v, f, need), hip.mesh_collapse_round(dv, df, need)
        same_bits(got, want, ("round", len(history)))
        c = counts_of(want)
        assert c["applied"] > 0
        v, f = want[0][:c["n_verts"]], want[1][:c["n_faces"]]
        dv, df = got[0][:c["n_verts"]], got[1][:c["n_faces"]]
        history.append(c["n_faces"])
    assert 20 < len(history) < 60                                                 # a round takes a few percent of the faces
    weights = torch.arange(verts.shape[0] * 2, dtype=torch.float32).reshape(-1, 2)
    ref = geometry.decimate_mesh(verts, faces, target_faces=target, attributes={"weights": weights})
    res = geometry.decimate_mesh(verts.to(DEV), faces.to(DEV).to(torch.int32), target_faces=target, attributes={"weights": weights.to(DEV)})
    assert res["report"] == ref["report"] and res["report"]["faces"] == history and res["verts"].is_cuda
    assert res["faces"].dtype == torch.int32 and (res["n_verts"], res["n_tris"]) == (ref["n_verts"], ref["n_tris"])
    same_bits((res["verts"], res["faces"].long(), res["vert_src"], res["face_src"], res["weights"]),
              (ref["verts"], ref["faces"], ref["vert_src"], ref["face_src"], ref["weights"]), "decimate_mesh")
    topo = geometry.mesh_topology(res["verts"], res["faces"])
    assert topo["watertight"] and topo["manifold"] and topo["euler"] == 2 and res["n_tris"] in (target, target - 1)


@pytest.fixture(scope="module")
def subject(scene):
    from conftest import get_model
    dev = torch.device(DEV)
    model, _ = get_model("zju377_mono", dev)
    model.eval()
    return model, scene.make_inputs(32, 32, frame_idx=0, device=dev)


def test_posed_mesh_decimated_stays_a_closed_surface(subject):
    from arah_release_amd import geometry
    model, inputs = subject
    how = {"method": "collapse", "ratio": 0.25}
    with torch.no_grad():
        plain = model.posed_mesh(inputs, n_side=64, indexed=True)
        small = model.posed_mesh(inputs, n_side=64, indexed=True, simplify=how)
        expect = geometry.decimate_mesh(plain["verts"], plain["faces"], ratio=0.25)
    before, after = geometry.mesh_topology(plain["verts"], plain["faces"]), geometry.mesh_topology(small["verts"], small["faces"])
    assert before["faces"] > 1000 and small["n_tris"] == after["faces"] < before["faces"]
    assert torch.equal(small["verts"], expect["verts"]) and torch.equal(small["faces"], expect["faces"])
    assert small["report"] == expect["report"] and small["verts"].shape == (small["n_verts"], 3)
    if before["manifold"] and before["watertight"]:
        assert after["manifold"] and after["watertight"] and after["euler"] == before["euler"]
        assert small["n_tris"] in (before["faces"] // 4, before["faces"] // 4 - 1) or not small["report"]["reached"]
    else:                                                                         # whatever was open or pinched stays exactly so
        assert after["boundary_edges"] == before["boundary_edges"] and after["nonmanifold_edges"] == before["nonmanifold_edges"]
    with torch.no_grad():
        canon = model.canonical_mesh(inputs, n_side=33, simplify={"method": "collapse", "target_faces": 400}, attributes=("normal",))
    assert canon["n_tris"] <= 400 or not canon["report"]["reached"]
    assert canon["normal"].shape == (canon["n_verts"], 3) and bool(torch.isfinite(canon["normal"]).all())
