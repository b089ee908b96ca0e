"""The kernels of csrc/meshquadric.hpp (arah_mesh_quadric_place) against their tensor specification meshing.mesh_quadric_place, bit
for bit, on the meshes of tests/test_mesh_quadric.py: pos, vert_src and qcounts, the rows beyond K zero; the C entry on buffers
of the test's own; and geometry.simplify_mesh(position="quadric" / target_faces=...) and the model's entries on device tensors
against the host path."""
import ctypes as C

import pytest
import torch

from test_mesh_quadric import OLD_KEYS, clustered, mesh, same_bits, spec

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x5A
PAD = 5
SHORT, BLOCK, LIMIT = 32, 256, 1 << 15                                            # kMqShort, kImeshThreads, kMqLimit
# every size class and both sides of every threshold: the lane's counter, one block of the workgroup's tree, several blocks and
# a partial last one, the longest segment that is placed and the shortest that is not
FANS = (1, 2, 3, SHORT - 1, SHORT, SHORT + 1, BLOCK, BLOCK + 1, 2 * BLOCK + 37, LIMIT, LIMIT + 1)
CASES = ([("sphere%d" % n, mult) for n in (17, 33) for mult in (2, 4, 8, 0)] + [("sphere17_dirty", 2), ("sphere17_dirty", 4)]
         + [("fan%d" % n, 0) for n in FANS] + [("plane150", 0)])


def on_device(name, mult):
    verts, faces, vert_map, means, counts, cell = clustered(name, mult)
    return verts.to(DEV), faces.to(DEV), vert_map.to(DEV), means.to(DEV), counts.to(DEV), cell


@pytest.mark.parametrize("name,mult", CASES, ids=lambda x: str(x))
def test_kernels_are_the_specification(name, mult):
    from arah_release_amd import hip
    want = spec(name, mult)
    args = on_device(name, mult)
    first = hip.mesh_quadric_place(*args)
    same_bits(first, want, (name, mult))
    K = int(clustered(name, mult)[4][0])
    assert not first[0][K:].any() and not first[1][K:].any()
    if name.startswith("fan"):                                                    # one segment of exactly that many faces
        n = int(name[3:])
        assert want[2].tolist()[1:] == [n, n, 2 if n > LIMIT else 0]
    if name == "plane150":
        assert want[2].tolist() == [0, 45000, 45000, 2]
    if (name, mult) == ("sphere33", 0):
        assert want[2].tolist()[2] == mesh(name)[1].shape[0] > 6000               # the workgroup's class, 24 blocks
    # again, with other integer types and K as a number: the order of arrival does not show
    verts, faces, vert_map, means, counts, cell = args
    again = hip.mesh_quadric_place(verts, faces.to(torch.int32), vert_map.long(), means, K, cell)
    for key, a, b in zip(("pos", "vert_src", "qcounts"), first, again):
        a, b = (a.view(torch.int32), b.view(torch.int32)) if a.dtype.is_floating_point else (a, b)
        assert torch.equal(a, b), (name, mult, key)


@pytest.mark.parametrize("reg", [0.0, 1e-9, 0.5])
def test_other_regularisers(reg):
    from arah_release_amd import hip
    for name, mult in (("sphere17", 4), ("fan33", 0)):
        same_bits(hip.mesh_quadric_place(*on_device(name, mult), reg=reg), spec(name, mult, reg), (name, mult, reg))


def test_empty_meshes_write_their_counts():
    from arah_release_amd import hip, meshing
    verts, faces, vert_map, means, counts, cell = on_device("sphere17", 2)
    got = hip.mesh_quadric_place(verts, faces[:0], vert_map, means, counts, cell)  # F = 0: every cluster falls back
    h = clustered("sphere17", 2)
    same_bits(got, meshing.mesh_quadric_place(h[0], h[1][:0], h[2], h[3], h[4], h[5]), "F = 0")
    assert got[2].tolist() == [int(counts[0]), 0, 0, 0]
    none = hip.mesh_quadric_place(verts[:0], faces[:0], vert_map[:0], means[:0], 0, cell)       # V = 0
    assert none[0].shape == (0, 3) and none[1].shape == (0,) and none[2].tolist() == [0, 0, 0, 0]
    zero = hip.mesh_quadric_place(verts, faces, vert_map, means, 0, cell)          # K = 0: no cluster, every row zero
    assert not zero[0].any() and not zero[1].any() and zero[2].tolist() == [0, 0, 0, 0]


def test_entry_writes_its_arrays_and_nothing_else():
    from arah_release_amd import hip
    verts, faces, vert_map, means, counts, cell = on_device("sphere17_dirty", 2)
    lib = hip.load_library()
    V, F = verts.shape[0], faces.shape[0]
    f32 = faces.to(torch.int32).contiguous()
    bufs = [None] + [torch.full((n + PAD,), SENTINEL, dtype=torch.int32, device=DEV) for n in (V, 4)]
    pos_bytes = torch.full(((V + PAD) * 12,), SENTINEL, dtype=torch.uint8, device=DEV)
    with hip._on_device(verts.device):
        scratch = hip._mesh_cc_buf(verts.device, int(lib.arah_mesh_quadric_place_scratch_bytes(V, F)))
        short = lib.arah_mesh_quadric_place(hip._ptr(verts), C.c_int64(V), hip._ptr(f32), C.c_int64(F), hip._ptr(vert_map),
                                            hip._ptr(means), hip._ptr(counts), C.c_float(cell), C.c_double(1e-3),
                                            hip._ptr(pos_bytes), hip._ptr(bufs[1]), hip._ptr(bufs[2]), hip._ptr(scratch),
                                            C.c_size_t(16), hip._stream())
        assert short == -3                                                        # ARAH_E_WORKSPACE, and nothing was launched
        torch.cuda.synchronize()
        assert bool((pos_bytes == SENTINEL).all()) and bool((bufs[2] == SENTINEL).all())
        rc = lib.arah_mesh_quadric_place(hip._ptr(verts), C.c_int64(V), hip._ptr(f32), C.c_int64(F), hip._ptr(vert_map),
                                         hip._ptr(means), hip._ptr(counts), C.c_float(cell), C.c_double(1e-3), hip._ptr(pos_bytes),
                                         hip._ptr(bufs[1]), hip._ptr(bufs[2]), hip._ptr(scratch), C.c_size_t(scratch.numel()),
                                         hip._stream())
    assert rc == 0
    pos = pos_bytes[:V * 12].view(torch.float32).reshape(V, 3)
    same_bits((pos, bufs[1][:V], bufs[2][:4]), spec("sphere17_dirty", 2), "raw entry")
    assert bool((pos_bytes[V * 12:] == SENTINEL).all())
    assert bool((bufs[1][V:] == SENTINEL).all()) and bool((bufs[2][4:] == SENTINEL).all())


def _same_dicts(got, ref):
    assert set(got) == set(ref)
    for k in ref:
        if torch.is_tensor(ref[k]):
            g = got[k].cpu().long() if k == "faces" else got[k].cpu()
            g, r = (g.view(torch.int32), ref[k].view(torch.int32)) if g.dtype == torch.float32 else (g, ref[k])
            assert torch.equal(g, r), k
        else:
            assert got[k] == ref[k], k


@pytest.mark.parametrize("how", [{"cell": 0.125, "position": "quadric"}, {"resolution": 9, "position": "quadric", "quadric_reg": 0.05},
                                 {"cell": 0.25, "position": "quadric", "drop_unreferenced": False, "dedup": False},
                                 {"target_faces": 300}, {"target_faces": 1000, "position": "quadric"}, {"target_faces": 3}], ids=str)
def test_simplify_mesh_on_the_device_is_the_host(how):
    from arah_release_amd import geometry
    verts, faces = mesh("sphere33")
    weights = torch.arange(verts.shape[0] * 2, dtype=torch.float32).reshape(-1, 2)
    ref = geometry.simplify_mesh(verts, faces, attributes={"weights": weights}, **how)
    got = geometry.simplify_mesh(verts.to(DEV), faces.to(DEV).to(torch.int32), attributes={"weights": weights.to(DEV)}, **how)
    extra = ({"quadric"} if how.get("position") == "quadric" else set()) | ({"resolution", "probes", "reached"} if "target_faces" in how
                                                                            else set())
    assert set(ref) == OLD_KEYS | {"weights"} | extra and got["verts"].is_cuda and got["faces"].dtype == torch.int32
    assert 0 < ref["n_tris"] < faces.shape[0] // 2
    _same_dicts(got, ref)


def test_long_segment_raises_on_the_device():
    from arah_release_amd import geometry
    verts, faces = mesh("plane150")
    with pytest.raises(ValueError, match="smaller cell or position='mean'"):
        geometry.simplify_mesh(verts.to(DEV), faces.to(DEV), cell=4.0, bounds=([-2.0] * 3, [2.0] * 3), position="quadric")


@pytest.fixture(scope="module")
def subject(scene):
    from conftest import get_model
    dev = torch.device(DEV)
    model, _ = get_model("zju377_mono", dev)
    model.eval()
    return model, scene.make_inputs(32, 32, frame_idx=0, device=dev)


def test_model_entries_take_the_new_keys(subject):
    from arah_release_amd import geometry
    model, inputs = subject
    with torch.no_grad():
        plain = model.posed_mesh(inputs, n_side=33, indexed=True)
        how = {"resolution": 10, "position": "quadric"}
        small = model.posed_mesh(inputs, n_side=33, indexed=True, simplify=how)
        expect = geometry.simplify_mesh(plain["verts"], plain["faces"], **how)
        assert set(small) == set(plain) | {"vert_src", "removed", "cell", "dims", "quadric"}
        assert 0 < small["n_tris"] < plain["n_tris"] and small["verts"].shape == (small["n_verts"], 3)
        assert torch.equal(small["verts"], expect["verts"]) and torch.equal(small["faces"], expect["faces"])
        assert small["quadric"] == expect["quadric"]
        how = {"target_faces": 300, "position": "quadric"}
        canon = model.canonical_mesh(inputs, n_side=33, simplify=how, attributes=("normal",))
        bare = model.canonical_mesh(inputs, n_side=33)
        expect = geometry.simplify_mesh(bare["verts"], bare["faces"], **how)
        assert canon["reached"] and 0 < canon["n_tris"] <= 300 and canon["resolution"] == expect["resolution"]
        assert torch.equal(canon["verts"], expect["verts"]) and torch.equal(canon["faces"], expect["faces"])
        assert canon["normal"].shape == (canon["n_verts"], 3) and bool(torch.isfinite(canon["normal"]).all())
