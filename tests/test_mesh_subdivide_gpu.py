"""The kernels of csrc/meshsubdiv.hpp (arah_mesh_subdivide_round) against their tensor specification
meshing.mesh_subdivide_round, bit for bit in every output and counter, on the meshes of tests/test_mesh_subdivide.py and sphere33;
empty inputs; the C entry on buffers of the test's own; geometry.subdivide_mesh on device tensors against the same loop over the
specification after every round; and the model's entries with subdivide=."""
import ctypes as C

import pytest
import torch

from test_mesh_collapse import mesh, shaped
from test_mesh_subdivide import CASES, counts_of, modes, same_bits, spec, thresholds

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x5A
PAD = 5


def run(name, method="midpoint", max_len2=None, faces_dtype=torch.int32):
    from arah_release_amd import hip
    verts, faces = mesh(name)
    return hip.mesh_subdivide_round(verts.to(DEV), faces.to(DEV).to(faces_dtype), method, max_len2)


# sphere33: 6 F = 31 k entries and 5 k faces, more than one wave, workgroup and chunk of every pass; no face count here is a
# multiple of the workgroup's 256 or of the walk's chunk of 1024
@pytest.mark.parametrize("name", CASES + ("sphere33",))
def test_kernels_are_the_specification(name):
    assert mesh(name)[1].shape[0] % 256 != 0
    for method, max_len2 in modes(name):
        want = spec(name, method, max_len2)
        first = run(name, method, max_len2)
        same_bits(first, want, (name, method, max_len2))
        # again, from faces of another integer type: the order of arrival in the adjacency build does not show
        same_bits(run(name, method, max_len2, faces_dtype=torch.int64), first, (name, method, max_len2, "again"))
    if name == "sphere33":
        c = counts_of(spec(name, "midpoint", thresholds(name)[0]))
        assert min(c["faces_%d" % m] for m in range(4)) > 0 and c["marked"] > 1024
        assert counts_of(spec(name, "loop"))["interior"] == mesh(name)[0].shape[0] > 1024


@pytest.mark.parametrize("kind", ["whole_waves", "isolated"])
def test_whole_waves_of_entries_and_isolated_vertices(kind):
    from arah_release_amd import hip, meshing
    verts, faces = shaped(kind)
    adj = meshing.mesh_adjacency(faces, verts.shape[0])
    assert (int(adj[2][-1]) % 64 == 0) == (kind == "whole_waves") and (int(adj[7][6]) == 2) == (kind == "isolated")
    for method, max_len2 in (("midpoint", None), ("midpoint", 1.5), ("loop", None)):
        want = meshing.mesh_subdivide_round(verts, faces, method, max_len2)
        same_bits(hip.mesh_subdivide_round(verts.to(DEV), faces.to(DEV), method, max_len2), want, (kind, method, max_len2))


def test_empty_meshes_write_their_counts():
    from arah_release_amd import hip, meshing
    verts, faces = mesh("octahedron")
    dv, df = verts.to(DEV), faces.to(DEV)
    for v, f, hv, hf in ((dv[:0], df[:0], verts[:0], faces[:0]), (dv, df[:0], verts, faces[:0]), (dv[:0], df, verts[:0], faces)):
        for method in ("midpoint", "loop"):
            same_bits(hip.mesh_subdivide_round(v, f, method), meshing.mesh_subdivide_round(hv, hf, method), (v.shape, f.shape, method))


def test_entry_writes_its_arrays_and_nothing_else():
    from arah_release_amd import hip
    name = "bad_ids"
    max_len2 = thresholds(name)[0]
    verts, faces = mesh(name)
    want = spec(name, "midpoint", max_len2)
    verts, f32 = verts.to(DEV), faces.to(DEV).to(torch.int32).contiguous()
    lib = hip.load_library()
    V, F = verts.shape[0], f32.shape[0]

    def buf(nbytes):
        return torch.full((nbytes + PAD,), SENTINEL, dtype=torch.uint8, device=DEV)
    sizes = ((V + 3 * F) * 12, 4 * F * 12, (V + 3 * F) * 8, 4 * F * 4, 13 * 4)
    need = int(lib.arah_mesh_subdivide_round_scratch_bytes(V, F))
    with hip._on_device(verts.device):
        scratch = buf(need)                                                       # the test's own, padded like the outputs
        for nbytes, rc_want in ((need - 1, -3), (need, 0)):                       # ARAH_E_WORKSPACE launches nothing
            bufs = [buf(n) for n in sizes]
            rc = lib.arah_mesh_subdivide_round(hip._ptr(verts), C.c_int64(V), hip._ptr(f32), C.c_int64(F), C.c_int32(0), C.c_int32(1),
                                               C.c_double(max_len2), *[hip._ptr(b) for b in bufs], hip._ptr(scratch),
                                               C.c_size_t(nbytes), hip._stream())
            torch.cuda.synchronize()
            assert rc == rc_want
            if rc:
                assert all(bool((b == SENTINEL).all()) for b in bufs) and bool((scratch == SENTINEL).all())
    for b, n in zip(bufs + [scratch], sizes + (need,)):
        assert bool((b[n:] == SENTINEL).all())
    kinds = (torch.float32, torch.int32, torch.int32, torch.int32, torch.int32)
    shapes = ((V + 3 * F, 3), (4 * F, 3), (V + 3 * F, 2), (4 * F,), (13,))
    got = [b[:n].view(k).reshape(s) for b, n, k, s in zip(bufs, sizes, kinds, shapes)]
    same_bits(got, want, "raw entry")
    c = counts_of(want)
    assert 0 < c["marked"] < c["edges"] and c["invalid"] == 4                      # rows between the counts and the capacity: zero
    assert not got[0][c["n_verts"]:].any() and not got[2][c["n_verts"]:].any() and c["n_verts"] < V + 3 * F
    assert not got[1][c["n_faces"]:].any() and not got[3][c["n_faces"]:].any() and c["n_faces"] < 4 * F


def rounds_by_hand(verts, faces, method, max_len2, n_rounds):
    """The loop of subdivide_mesh over the specification on the host and over the kernels on the device, compared after every round."""
    from arah_release_amd import hip, meshing
    v, f = verts, faces
    dv, df = verts.to(DEV), faces.to(DEV).to(torch.int32)
    history = []
    for _ in range(n_rounds):
        want, got = meshing.mesh_subdivide_round(v, f, method, max_len2), hip.mesh_subdivide_round(dv, df, method, max_len2)
        same_bits(got, want, ("round", len(history)))
        c = counts_of(want)
        history.append(c["marked"])
        if max_len2 is not None and c["marked"] == 0:
            break
        v, f = want[0][:c["n_verts"]], want[1][:c["n_faces"]]
        dv, df = got[0][:c["n_verts"]], got[1][:c["n_faces"]]
    return history


@pytest.mark.parametrize("name,kw", [("torus", {"levels": 2}), ("torus", {"levels": 2, "method": "loop"}), ("sphere17", {"max_edge": None})])
def test_subdivide_on_the_device_is_the_specification_after_every_round(name, kw):
    from arah_release_amd import geometry
    verts, faces = mesh(name)
    if "max_edge" in kw:
        kw = {"max_edge": 0.6 * thresholds(name)[0] ** 0.5}
    max_len2 = float(kw["max_edge"]) ** 2 if "max_edge" in kw else None
    history = rounds_by_hand(verts, faces, kw.get("method", "midpoint"), max_len2, kw.get("levels", 16))
    attrs = {"w": torch.arange(verts.shape[0] * 2, dtype=torch.float32).reshape(-1, 2), "label": torch.arange(verts.shape[0])}
    ref = geometry.subdivide_mesh(verts, faces, attributes=attrs, **kw)
    res = geometry.subdivide_mesh(verts.to(DEV), faces.to(DEV).to(torch.int32), attributes={k: t.to(DEV) for k, t in attrs.items()}, **kw)
    assert res["report"] == ref["report"] and res["report"]["marked"] == history and res["verts"].is_cuda and res["report"]["reached"]
    assert res["faces"].dtype == torch.int32 and (res["n_verts"], res["n_tris"]) == (ref["n_verts"], ref["n_tris"])
    same_bits((res["verts"], res["faces"].long(), res["vert_src"], res["face_src"], res["w"]),
              (ref["verts"], ref["faces"], ref["vert_src"], ref["face_src"], ref["w"]), "subdivide_mesh")
    assert torch.equal(res["label"].cpu(), ref["label"])
    assert torch.equal(res["vert_weights"].to_dense().cpu(), ref["vert_weights"].to_dense())
    topo = geometry.mesh_topology(res["verts"], res["faces"])
    assert topo["watertight"] and topo["manifold"] and topo["euler"] == (0 if name == "torus" else 2)


@pytest.fixture(scope="module")
def subject(scene):
    from conftest import get_model
    dev = torch.device(DEV)
    model, _ = get_model("zju377_mono", dev)
    model.eval()
    return model, scene.make_inputs(32, 32, frame_idx=0, device=dev)


def test_model_refines_before_it_asks_the_networks(subject):
    from arah_release_amd import geometry
    model, inputs = subject
    how = {"method": "collapse", "ratio": 0.2}
    with torch.no_grad():
        coarse = model.canonical_mesh(inputs, n_side=64, simplify=how)
        same = model.canonical_mesh(inputs, n_side=64, simplify=how, subdivide=None, attributes=("color", "verts_posed"))
        plain = model.canonical_mesh(inputs, n_side=64, simplify=how, attributes=("color", "verts_posed"))
        fine = model.canonical_mesh(inputs, n_side=64, simplify=how, subdivide=1, attributes=("color", "verts_posed"))
    assert set(same) == set(plain) and all(torch.equal(same[k], plain[k]) for k in ("verts", "faces", "color", "verts_posed"))
    before, after = geometry.mesh_topology(coarse["verts"], coarse["faces"]), geometry.mesh_topology(fine["verts"], fine["faces"])
    assert fine["n_verts"] == coarse["n_verts"] + before["edges"] and fine["n_tris"] == 4 * coarse["n_tris"] == after["faces"]
    assert fine["color"].shape == (fine["n_verts"], 3) and fine["verts_posed"].shape == (fine["n_verts"], 3)
    assert bool(torch.isfinite(fine["color"]).all()) and bool(torch.isfinite(fine["verts_posed"]).all())
    assert torch.equal(fine["verts"][:coarse["n_verts"]], coarse["verts"]) and fine["subdivide"]["report"]["rounds"] == 1
    assert fine["report"] == coarse["report"] and fine["subdivide"]["vert_src"].shape == (fine["n_verts"], 2)
    if before["watertight"]:
        assert after["watertight"] and after["manifold"] and after["euler"] == before["euler"]
    with torch.no_grad():
        img = model.render_mesh(inputs, height=40, width=48, n_side=64, simplify=how, subdivide=1, attributes=("color",))
        posed = model.posed_mesh(inputs, n_side=64, indexed=True, simplify=how, subdivide={"levels": 1, "method": "loop"})
        hits = model.mesh_intersections(inputs, n_side=64, simplify=how, subdivide=1)
    assert img["color"].shape == (40, 48, 3) and img["mask"].shape == (40, 48) and bool(img["mask"].any())
    assert img["mesh"]["n_tris"] == fine["n_tris"] == hits["mesh"]["n_tris"]
    assert posed["n_tris"] % 4 == 0 and posed["verts"].shape == (posed["n_verts"], 3) and posed["subdivide"]["report"]["counts"]["interior"] > 0
    with pytest.raises(ValueError):
        model.posed_mesh(inputs, n_side=64, subdivide=1)
