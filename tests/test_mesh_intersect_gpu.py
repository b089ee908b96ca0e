"""The kernels of csrc/meshintersect.hpp (arah_mesh_intersections) against their tensor specification, bit for bit, on the meshes
of tests/test_mesh_intersect.py plus two that the device alone needs -- one whose long triangles go to the index's big list, one
whose rows are long enough for the workgroup sort --; the C entry on buffers of the test's own; and geometry.self_intersections /
mesh_intersections and model.mesh_intersections on device tensors against the host path."""
import ctypes as C

import pytest
import torch

from conftest import get_model
from test_mesh_intersect import GPU_ONLY, MESHES, NAMES, QUANT, _level_set, mesh, spec, two_sphere_groups

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x5A
PAD = 5


def _same(got, want, what):
    for key, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and tuple(g.shape) == tuple(w.shape), (what, key, g.dtype, tuple(g.shape), tuple(w.shape))
        assert torch.equal(g.cpu(), w), (what, key)


@pytest.mark.parametrize("name", MESHES + GPU_ONLY)
def test_kernels_are_the_specification(name):
    from arah_release_amd import hip, meshing
    verts, faces = mesh(name)
    v, f = verts.to(DEV), faces.to(DEV)
    want = spec(name)
    first = hip.mesh_intersections(v, f, quant=QUANT.get(name))
    c = want[4].tolist()
    print("%s: %d faces, %d pairs on %d faces, %d void" % (name, faces.shape[0], c[0], c[1], c[3]))
    _same(first, want, name)
    quant = QUANT.get(name) or meshing.orient_quant(verts)
    calls = [hip.mesh_intersections(v, f, quant=quant), hip.mesh_intersections(v, f, quant=QUANT.get(name))]   # given, and once more
    if name != "hand":                                                 # the hand-made mesh has ids that only int64 holds
        calls.append(hip.mesh_intersections(v, f.to(torch.int32), quant=QUANT.get(name)))
    for again in calls:
        for key, a, b in zip(NAMES, first, again):
            assert torch.equal(a, b), (name, key)
    tested = hip.mesh_intersections(v, f, quant=QUANT.get(name), want_tested=True)
    assert len(tested) == 6 and tested[5].dtype == torch.int64 and int(tested[5]) >= 2 * c[0]   # a pair is tested once per side
    _same(tested[:5], want, (name, "tested"))


def test_big_list_mesh_takes_the_big_list():
    """Three long triangles through the sphere's box: the index puts them on its big list, one of them cuts the sphere, two of them
    cut each other, one meets nothing."""
    from arah_release_amd import hip, meshing
    verts, faces = mesh("big_list")
    F = faces.shape[0]
    q, void = meshing.intersect_soup(verts, faces, meshing.orient_quant(verts))
    head = hip.mesh_index(q.float().to(DEV)).header()
    print("big_list: n_big %d, cells %s" % (head["n_big"], head["n"]))
    assert head["n_big"] >= 3 and head["status"] == 0 and not bool(void.any())
    hits, _, pair_start, pairs, counts = spec("big_list")
    assert hits[F - 3] > 10 and hits[F - 2] > 10 and hits[F - 1] == 0
    assert [F - 3, F - 2] in pairs.tolist()
    assert int(pair_start[F - 2] - pair_start[F - 3]) == 1             # the first long triangle's row: the second one alone is above it


def test_noise25_has_long_rows_and_ragged_sizes():
    verts, faces = mesh("noise25")
    hits, _, pair_start, _, counts = spec("noise25")
    F = faces.shape[0]
    assert F % 64 != 0 and F % 256 != 0 and F > 1024
    rows = pair_start[1:] - pair_start[:-1]
    print("noise25: %d faces, %d pairs, longest row %d" % (F, counts[0].item(), int(rows.max())))
    assert counts[0].item() > 500


def test_long_rows_go_through_the_workgroup_sort():
    """A fan of 80 long blades through one plate: the plate's row and the blades' own rows are longer than a thread sorts alone."""
    from arah_release_amd import hip, meshing
    n = 80
    g = torch.Generator().manual_seed(3)
    plate = torch.tensor([[-1.0, -1.0, 0.0], [1.0, -1.0, 0.0], [0.0, 1.0, 0.0]])
    ang = torch.rand(n, generator=g) * 3.14159
    base = torch.stack([0.3 * torch.cos(ang), 0.3 * torch.sin(ang) - 0.3, torch.full((n,), -0.5)], 1)
    blades = torch.stack([base, base * torch.tensor([-1.0, 1.0, 1.0]) + torch.tensor([0.0, 0.0, 0.01]),
                          base * 0.1 + torch.tensor([0.0, -0.3, 0.5])], 1) + 0.01 * torch.randn(n, 3, 3, generator=g)
    verts = torch.cat([plate, blades.reshape(-1, 3)]).float()
    faces = torch.arange(3 * (n + 1)).reshape(-1, 3)
    want = meshing.mesh_intersections(verts, faces)
    rows = want[2][1:] - want[2][:-1]
    print("fan: %d pairs, longest row %d" % (want[4][0].item(), int(rows.max())))
    assert int(rows.max()) > 32
    _same(hip.mesh_intersections(verts.to(DEV), faces.to(DEV)), want, "fan")
    perm = torch.randperm(n + 1, generator=g)                          # the long rows elsewhere, the partners in another order
    want = meshing.mesh_intersections(verts, faces[perm])
    _same(hip.mesh_intersections(verts.to(DEV), faces[perm].to(DEV)), want, "fan, permuted")


@pytest.mark.parametrize("max_pairs", [0, 1, 10, 50])
def test_truncated_pair_lists(max_pairs):
    from arah_release_amd import hip
    verts, faces = mesh("two_spheres")
    want = spec("two_spheres", False, max_pairs)
    assert want[4][0].item() > 50
    _same(hip.mesh_intersections(verts.to(DEV), faces.to(DEV), max_pairs=max_pairs), want, max_pairs)
    whole = hip.mesh_intersections(verts.to(DEV), faces.to(DEV), max_pairs=max_pairs, trim=False)
    assert whole[3].shape == (max_pairs, 2) and torch.equal(whole[3].cpu(), want[3])


def test_between_two_meshes():
    from arah_release_amd import hip
    verts, faces = mesh("two_spheres")
    group, Fa = two_sphere_groups()
    v, f = verts.to(DEV), faces.to(DEV)
    _same(hip.mesh_intersections(v, f, group=group.to(DEV), between=True), spec("two_spheres", True), "between")
    none = hip.mesh_intersections(v, f, group=torch.zeros_like(group).to(DEV), between=True)
    assert none[4].tolist() == [0, 0, 0, 0, 0] and none[3].shape == (0, 2) and not bool(none[0].any())
    _same(hip.mesh_intersections(v, f, group=group.to(DEV), between=False), spec("two_spheres"), "a group without between")
    with pytest.raises(ValueError):
        hip.mesh_intersections(v, f, group=group, between=True)        # the group on the host
    with pytest.raises(ValueError):
        hip.mesh_intersections(v, f, between=True)
    with pytest.raises(ValueError):
        hip.mesh_intersections(verts, f)
    with pytest.raises(ValueError):
        hip.mesh_intersections(v, f, max_pairs=-1)


def test_no_face_and_one_face():
    from arah_release_amd import hip, meshing
    none = torch.zeros(0, 3, dtype=torch.int64)
    for verts in (torch.zeros(0, 3), torch.randn(4, 3, generator=torch.Generator().manual_seed(1))):
        _same(hip.mesh_intersections(verts.to(DEV), none.to(DEV)), meshing.mesh_intersections(verts, none), ("no face", verts.shape[0]))
    verts = torch.randn(4, 3, generator=torch.Generator().manual_seed(1))
    for one in (torch.tensor([[0, 1, 2]]), torch.tensor([[0, 1, 4]])):
        _same(hip.mesh_intersections(verts.to(DEV), one.to(DEV)), meshing.mesh_intersections(verts, one), ("one face", one.tolist()))


# ---- the C entry on the test's own buffers ---------------------------------------------------------------------------------------
def _buffers(shapes_dtypes):
    """Buffers PAD rows longer than the entry's arrays, pre-filled with a sentinel: -> (the buffers, the arrays, the paddings)."""
    bufs, arrays, pads = [], [], []
    for shape, dtype in shapes_dtypes:
        b = torch.full((shape[0] + PAD,) + tuple(shape[1:]), SENTINEL, dtype=dtype, device=DEV)
        bufs.append(b)
        arrays.append(b[:shape[0]])
        pads.append(b[shape[0]:])
    return bufs, arrays, pads


def raw_intersections(verts, faces, quant, max_pairs):
    from arah_release_amd import hip
    lib = hip.load_library()
    V, F = verts.shape[0], faces.shape[0]
    v, f = verts.to(DEV).contiguous(), faces.to(DEV).to(torch.int32).contiguous()
    i32 = torch.int32
    bufs, arrays, pads = _buffers([((F,), i32), ((V,), torch.uint8), ((F + 1,), i32), ((max_pairs, 2), i32), ((5,), i32), ((1,), torch.int64)])
    origin, scale = quant
    with hip._on_device(f.device):
        scratch = hip._mesh_cc_buf(f.device, int(lib.arah_mesh_intersections_scratch_bytes(V, F, max_pairs)))
        rc = lib.arah_mesh_intersections(hip._ptr(v), C.c_int64(V), hip._ptr(f), C.c_int64(F), None, C.c_int32(0), (C.c_float * 3)(*origin),
                                         C.c_double(scale), C.c_int64(max_pairs), *[hip._ptr(b) for b in bufs], hip._ptr(scratch),
                                         C.c_size_t(scratch.numel()), hip._stream())
    assert rc == 0
    return arrays, pads


@pytest.mark.parametrize("name,max_pairs", [("two_spheres", 1 << 10), ("two_spheres", 7), ("noise25", 1 << 12), ("noise25", 100), ("big_list", 1 << 10),
                                            ("sphere17", 16)])
def test_c_entry_on_the_tests_own_buffers(name, max_pairs):
    """Rows beyond the arrays come back untouched; rows of pairs beyond the pairs written, inside the array, are zero."""
    from arah_release_amd import meshing
    verts, faces = mesh(name)
    want = spec(name, False, max_pairs)
    arrays, pads = raw_intersections(verts, faces, meshing._check_quant(meshing.orient_quant(verts), name), max_pairs)
    written = want[4][4].item()
    got = list(arrays[:5])
    assert not bool(got[3][written:].any()), (name, "rows behind the pairs written")
    got[3] = got[3][:written]
    _same(got, want, (name, max_pairs))
    assert all(bool((p == SENTINEL).all()) for p in pads), name
    assert int(arrays[5]) > 0 or want[4][0].item() == 0


def test_c_entry_refuses_bad_arguments():
    from arah_release_amd import hip
    lib = hip.load_library()
    assert lib.arah_mesh_intersections_scratch_bytes(-1, 4, 16) == 0 and lib.arah_mesh_intersections_scratch_bytes(4, (1 << 26) + 1, 16) == 0
    assert lib.arah_mesh_intersections_scratch_bytes(4, 4, 1 << 31) == 0 and lib.arah_mesh_intersections_scratch_bytes(4, 4, 16) % 256 == 0
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    p = hip._ptr(buf)
    args = lambda scale, scratch_bytes: (p, C.c_int64(4), p, C.c_int64(1), None, C.c_int32(0), (C.c_float * 3)(0, 0, 0), C.c_double(scale),
                                         C.c_int64(4), p, p, p, p, p, None, p, C.c_size_t(scratch_bytes), None)
    assert lib.arah_mesh_intersections(*args(0.0, 1 << 16)) != 0      # the scale
    assert lib.arah_mesh_intersections(*args(1.0, 16)) != 0            # the scratch


# ---- geometry and the model ---------------------------------------------------------------------------------------------------------
def _same_report(dev, host, what):
    assert set(dev) == set(host), what
    for key, h in host.items():
        d = dev[key]
        if isinstance(h, torch.Tensor):
            assert d.is_cuda and d.dtype == h.dtype and torch.equal(d.cpu(), h), (what, key)
        else:
            assert d == h, (what, key)


def test_geometry_on_the_device_is_geometry_on_the_host():
    from arah_release_amd import geometry
    for name in ("two_spheres", "noise17", "hand", "big_list"):
        verts, faces = mesh(name)
        for kw in (dict(), dict(max_pairs=5), dict(return_pairs=False)):
            _same_report(geometry.self_intersections(verts.to(DEV), faces.to(DEV), **kw), geometry.self_intersections(verts, faces, **kw), (name, kw))
    (va, fa), (vb, fb) = _level_set(17, 0.4, (-0.2, 0.0, 0.0)), _level_set(17, 0.4, (0.2, 0.03, 0.01))
    for kw in (dict(), dict(max_pairs=5), dict(return_pairs=False)):
        _same_report(geometry.mesh_intersections((va.to(DEV), fa.to(DEV)), (vb.to(DEV), fb.to(DEV)), **kw),
                     geometry.mesh_intersections((va, fa), (vb, fb), **kw), ("two meshes", kw))
    far = geometry.mesh_intersections((va.to(DEV), fa.to(DEV)), (vb.to(DEV) + 5.0, fb.to(DEV)))
    assert far["disjoint"] and far["count"] == 0
    with pytest.raises(ValueError):
        geometry.mesh_intersections((va.to(DEV), fa.to(DEV)), (vb, fb))


def test_model_reports_where_the_posed_body_passes_through_itself(scene):
    from arah_release_amd import geometry
    dev = torch.device(DEV)
    model, _ = get_model("zju377_mono", dev)
    model.eval()
    inputs = scene.make_inputs(64, 64, frame_idx=0, device=dev)
    with torch.no_grad():
        for space in ("posed", "canonical"):
            res = model.mesh_intersections(inputs, n_side=64, space=space)
            m = res["mesh"]
            verts = m["verts_posed"] if space == "posed" else m["verts"]
            host = geometry.self_intersections(verts.cpu(), m["faces"].cpu())
            print("model, %s: %d faces, %d pairs on %d faces" % (space, m["faces"].shape[0], res["count"], res["faces_hit"]))
            _same_report({k: v for k, v in res.items() if k != "mesh"}, host, space)
            assert res["vert_hit"].shape == (verts.shape[0],) and res["hits"].shape == (m["faces"].shape[0],)
        drawn = model.render_mesh(inputs, 64, 64, n_side=64, attributes=())
        picture = geometry.render_mesh(m["verts"], m["faces"], 32, 32, camera={"azim": 0.0},
                                       attributes={"hit": res["vert_hit"].float()[:, None]})
        assert picture["hit"].shape == (32, 32, 1) and drawn["mesh"]["faces"].shape == m["faces"].shape
    with pytest.raises(ValueError):
        model.mesh_intersections(inputs, n_side=64, space="world")
