"""Signed distance to a mesh on the device (DESIGN.md "Signed distance to a mesh on the device"): arah_mesh_sdf_grid
(csrc/meshsdf.hpp) against the specification meshing.mesh_sdf_grid bit for bit, the C entry on the test's own buffers,
geometry.mesh_sdf, geometry.remesh bracketed by the icosphere's balls, MetaAvatarRender.geometry_metrics(sdf=N) and
`validate --geometry-sdf`."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from conftest import get_model
from test_geometry_metrics import icosphere
from test_mesh_contains import cube, f10, indexed
from test_mesh_sdf import sphere_radii

gpu = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")
DIMS = ((1, 1, 1), (5, 3, 70), (33, 17, 65), (2, 1, 4100))
CLASSES = ("lane", "wave", "group", "huge")


def _meshes():
    """name -> (verts float32, faces int32) on the host."""
    verts, faces, _, _ = f10()
    verts = verts.to(torch.float32)
    out = {"f10": (verts, faces)}
    out["icosphere"] = indexed(icosphere(2))
    out["f10_open"] = (verts, faces[torch.arange(faces.shape[0]) % 3 != 0])            # a third of the faces removed: an open sheet
    n = verts.shape[0]
    extra = torch.cat([verts, torch.tensor([[0.1, 0.2, 0.3], [0.3, 0.2, 0.1]])])
    flat = torch.tensor([[5, 5, 9], [7, 7, 7], [n, n, n], [n, n + 1, n], [3, 900, 3]], dtype=torch.int32)   # points and segments
    out["f10_zero_area"] = (extra, torch.cat([faces[:2000], flat, faces[2000:]]))
    lo, hi = verts.amin(0) - 0.1, verts.amax(0) + 0.1
    quad = torch.stack([lo, torch.stack([hi[0], lo[1], lo[2]]), hi, torch.stack([lo[0], hi[1], hi[2]])])
    out["f10_sheet"] = (torch.cat([verts, quad]), torch.cat([faces, torch.tensor([[n, n + 1, n + 2], [n, n + 2, n + 3]], dtype=torch.int32)]))
    return out


def _axes(lo, hi, dims, dev):
    """Nodes from lo to hi (one node: the middle), float64 rounded to float32; the largest step."""
    axes, step = [], 0.0
    for a, n in enumerate(dims):
        if n == 1:
            x = torch.tensor([0.5 * (lo[a] + hi[a])], dtype=torch.float64)
        else:
            x = lo[a] + torch.arange(n, dtype=torch.float64) * ((hi[a] - lo[a]) / (n - 1))
            step = max(step, float(hi[a] - lo[a]) / (n - 1))
        axes.append(x.to(torch.float32).to(dev))
    return axes, step


def _cut(full_d2, full_face, t):
    """The band of the specification: a node with d2 > t^2 reports +inf, -1."""
    out = full_d2 > t * t
    return torch.where(out, torch.full_like(full_d2, INF), full_d2), torch.where(out, torch.full_like(full_face, -1), full_face)


def _same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    ints = {torch.float64: torch.int64, torch.float32: torch.int32}.get(a.dtype)
    if ints is not None:
        a, b = a.contiguous().view(ints), b.contiguous().view(ints)
    assert torch.equal(a, b), what


_RUNS = {}


def _run(name):
    """Every lattice and every band of one mesh through the kernel and the specification: asserts, returns the class counts seen."""
    if name in _RUNS:
        return _RUNS[name]
    from arah_release_amd import hip, meshing
    dev = torch.device(DEV)
    verts, faces = (x.to(dev) for x in _meshes()[name])
    tris = verts[faces.long()].contiguous()
    index = hip.contains_index(verts, faces, 512)
    lo, hi = verts.double().amin(0).cpu() - 0.05, verts.double().amax(0).cpu() + 0.05
    diag = float((hi - lo).norm())
    seen = dict.fromkeys(CLASSES, 0)
    for dims in DIMS:
        axes, step = _axes(lo, hi, dims, dev)
        step = step or 0.05 * diag
        grid = torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1).reshape(-1, 3)
        want_in = meshing.mesh_contains(verts, faces, grid, 512)[0].reshape(dims)
        full_d2, full_face = meshing.mesh_sdf_grid(tris, *axes, INF, chunk_pairs=1 << 23)          # the reference, once per lattice
        occ, _ = hip.mesh_contains_grid(index, *axes)
        assert torch.equal(occ, want_in), (name, dims)
        for trunc in (0.0, 0.4 * step, 3.0 * step, 2.0 * diag):
            t = meshing.check_trunc(trunc)
            what = "%s %s trunc %g" % (name, dims, t)
            want_d2, want_face = _cut(full_d2, full_face, t)
            d2, face, sdf, info = hip.mesh_sdf_grid(tris, *axes, trunc, occupancy=occ, want_face=True, want_info=True)
            _same_bits(d2, want_d2, what + ": d2")
            _same_bits(face, want_face, what + ": face")
            _same_bits(sdf, meshing.signed_distance(want_d2, want_in, t), what + ": sdf")
            got = hip.read_sdf_grid_info(info)
            band = int(((want_d2 <= t * t) & (want_d2 < INF)).sum())
            assert got["status"] == 0 and got["band"] == band, (what, got, band)
            assert got["tests"] >= band and sum(got[c] for c in CLASSES) <= tris.shape[0], (what, got)
            if trunc > diag:    # every node is in the band: the untruncated brute force
                n = dims[0] * dims[1] * dims[2]
                assert band == n and got["tests"] == n * tris.shape[0] and sum(got[c] for c in CLASSES) == tris.shape[0], (what, got)
                assert bool((face >= 0).all())
            for c in CLASSES:
                seen[c] += got[c]
            # without the face the band is walked once; d2 and sdf are the same
            d2_only, no_face, sdf_only, _ = hip.mesh_sdf_grid(tris, *axes, trunc, occupancy=occ)
            assert no_face is None
            _same_bits(d2_only, want_d2, what + ": d2 without face")
            _same_bits(sdf_only, sdf, what + ": sdf without face")
    print("%s: triangles per class over all cases %s" % (name, seen))
    _RUNS[name] = seen
    return seen


@gpu
@pytest.mark.parametrize("name", ["f10", "icosphere", "f10_open", "f10_zero_area", "f10_sheet"])
def test_kernel_equals_specification_bit_for_bit(name):
    _run(name)


@gpu
def test_every_size_class_was_exercised():
    seen = dict.fromkeys(CLASSES, 0)
    for name in ("f10", "icosphere", "f10_open", "f10_zero_area", "f10_sheet"):
        for c, n in _run(name).items():
            seen[c] += n
    print("triangles per class:", seen)
    assert all(seen[c] > 0 for c in CLASSES), seen


@gpu
def test_class_edges_and_the_remainder_of_the_parts():
    """Six triangles with corners on the nodes of an integer lattice and trunc = 1 / 4: a box holds the nodes of the triangle's own
    bounding box, here exactly 32, 33, 2048, 2049, 32768 and 32769 = 33 x 3 x 331 (no multiple of the 64 parts) -- the last of the
    lane, the first and the last of the wave and of the workgroup class, the first of the several-workgroups class."""
    from arah_release_amd import hip, meshing
    dev = torch.device(DEV)
    dims, trunc = (33, 32, 683), 0.25
    boxes = ((4, 4, 2), (3, 11, 1), (16, 16, 8), (3, 1, 683), (32, 32, 32), (33, 3, 331))
    tris = torch.tensor([[[0, 0, 0], [w - 1, 0, d - 1], [0, h - 1, 0]] for w, h, d in boxes], dtype=torch.float32)
    axes = [torch.arange(n, dtype=torch.float32) for n in dims]
    nodes = [int(np.prod([int(((x >= t[:, a].min() - trunc) & (x <= t[:, a].max() + trunc)).sum()) for a, x in enumerate(axes)])) for t in tris]
    assert nodes == [32, 33, 2048, 2049, 32768, 32769]
    tris, axes = tris.to(dev), [x.to(dev) for x in axes]
    want_d2, want_face = meshing.mesh_sdf_grid(tris, *axes, trunc)
    d2, face, _, info = hip.mesh_sdf_grid(tris, *axes, trunc, want_face=True, want_info=True)          # both passes
    _same_bits(d2, want_d2, "d2")
    _same_bits(face, want_face, "face")
    got = hip.read_sdf_grid_info(info)
    assert [got[c] for c in CLASSES] == [1, 2, 2, 1] and got["status"] == 0, got
    assert got["tests"] == sum(nodes), got                        # every node of every box once, whatever its class
    assert got["band"] == int(torch.isfinite(want_d2).sum()) > 0
    d2_only, no_face, _, info = hip.mesh_sdf_grid(tris, *axes, trunc, want_info=True)                  # the first pass alone
    assert no_face is None
    _same_bits(d2_only, want_d2, "d2 without face")
    assert hip.read_sdf_grid_info(info) == got


@gpu
def test_cut_is_the_specifications_band():
    """The reference the cases share is cut after the fact; the specification with a finite trunc says the same."""
    from arah_release_amd import meshing
    dev = torch.device(DEV)
    verts, faces = (x.to(dev) for x in _meshes()["icosphere"])
    tris = verts[faces.long()].contiguous()
    axes, step = _axes(torch.tensor([-1.2] * 3, dtype=torch.float64), torch.tensor([1.2] * 3, dtype=torch.float64), (9, 4, 11), dev)
    full = meshing.mesh_sdf_grid(tris, *axes, INF)
    for trunc in (0.0, 0.1, 3.0 * step):
        got = meshing.mesh_sdf_grid(tris, *axes, trunc)
        want = _cut(*full, meshing.check_trunc(trunc))
        _same_bits(got[0], want[0], "d2")
        _same_bits(got[1], want[1], "face")


@gpu
def test_two_runs_give_identical_bits():
    from arah_release_amd import hip
    dev = torch.device(DEV)
    verts, faces = (x.to(dev) for x in _meshes()["f10_sheet"])
    tris = verts[faces.long()].contiguous()
    axes, step = _axes(verts.double().amin(0).cpu(), verts.double().amax(0).cpu(), (40, 23, 31), dev)
    runs = [hip.mesh_sdf_grid(tris, *axes, 2.5 * step, want_face=True, want_info=True) for _ in range(2)]
    runs.append(hip.mesh_sdf_grid(tris.clone(), *[x.clone() for x in axes], 2.5 * step, want_face=True, want_info=True))
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            _same_bits(a, b, "two runs")
    # no occupancy: every node counts as outside, the value is the truncated unsigned distance
    assert bool((runs[0][2] >= 0).all()) and float(runs[0][2].max()) == float(np.float32(2.5 * step))


@gpu
def test_ties_on_mesh_vertices_take_the_lowest_face():
    from arah_release_amd import hip, meshing
    dev = torch.device(DEV)
    verts, faces = cube(1.0)
    tris = verts[faces.long()].contiguous().to(dev)
    axis = torch.tensor([0.0, 0.5, 1.0], device=dev)
    d2, face, _, _ = hip.mesh_sdf_grid(tris, axis, axis, axis, 0.25, want_face=True)
    want_d2, want_face = meshing.mesh_sdf_grid(tris, axis, axis, axis, 0.25)
    _same_bits(d2, want_d2, "d2")
    _same_bits(face, want_face, "face")
    for v in range(8):
        i, j, k = (2 * int(c) for c in verts[v])
        lowest = min(f for f in range(12) if v in faces[f].tolist())
        assert float(d2[i, j, k]) == 0.0 and int(face[i, j, k]) == lowest, (v, int(face[i, j, k]), lowest)
    assert float(d2[1, 1, 1]) == INF and int(face[1, 1, 1]) == -1           # the centre is 0.5 away
    assert float(d2[1, 1, 0]) == 0.0 and int(face[1, 1, 0]) == 0            # on the diagonal two faces share


@gpu
def test_c_entry_on_the_tests_own_buffers():
    """Sentinels around every output, F = 0, NULL face / sdf, a vertex that is not finite."""
    from arah_release_amd import hip, meshing
    lib = hip.load_library()
    dev = torch.device(DEV)
    verts, faces = (x.to(dev) for x in _meshes()["icosphere"])
    tris = verts[faces.long()].contiguous()
    dims = (7, 5, 9)
    axes, step = _axes(torch.tensor([-1.1] * 3, dtype=torch.float64), torch.tensor([1.1] * 3, dtype=torch.float64), dims, dev)
    n, pad = dims[0] * dims[1] * dims[2], 64
    trunc = 2.0 * step
    want_d2, want_face = meshing.mesh_sdf_grid(tris, *axes, trunc)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call(tris_t, n_faces, want_face_out=True, want_sdf=True):
        bufs = {"d2": torch.full((n + 2 * pad,), -7.0, dtype=torch.float64, device=dev),
                "face": torch.full((n + 2 * pad,), -77, dtype=torch.int32, device=dev),
                "sdf": torch.full((n + 2 * pad,), -7.0, dtype=torch.float32, device=dev),
                "info": torch.full((8 + 2 * pad,), -77, dtype=torch.int32, device=dev)}
        nbytes = int(lib.arah_mesh_sdf_grid_bytes(n_faces, *dims))
        assert nbytes > 0
        scratch = torch.full((nbytes + 2 * 256,), 0x5a, dtype=torch.uint8, device=dev)
        at = lambda b: C.c_void_p(b.data_ptr() + pad * b.element_size())
        with torch.cuda.device(dev):
            rc = lib.arah_mesh_sdf_grid(C.c_void_p(tris_t.data_ptr()) if tris_t is not None else None, C.c_int32(n_faces),
                                        C.c_void_p(axes[0].data_ptr()), C.c_int32(dims[0]), C.c_void_p(axes[1].data_ptr()), C.c_int32(dims[1]),
                                        C.c_void_p(axes[2].data_ptr()), C.c_int32(dims[2]), C.c_float(trunc), None, at(bufs["d2"]),
                                        at(bufs["face"]) if want_face_out else None, at(bufs["sdf"]) if want_sdf else None, at(bufs["info"]),
                                        C.c_void_p(scratch.data_ptr() + 256), C.c_size_t(nbytes), stream)
        assert rc == 0
        torch.cuda.synchronize(dev)
        for key, b in bufs.items():
            fill = -7.0 if b.dtype.is_floating_point else -77
            m = 8 if key == "info" else n
            assert bool((b[:pad] == fill).all()) and bool((b[pad + m:] == fill).all()), key + ": written outside"
        assert bool((scratch[:256] == 0x5a).all()) and bool((scratch[256 + nbytes:] == 0x5a).all()), "scratch: written outside"
        if not want_face_out:
            assert bool((bufs["face"] == -77).all())
        if not want_sdf:
            assert bool((bufs["sdf"] == -7.0).all())
        return (bufs["d2"][pad:pad + n].reshape(dims), bufs["face"][pad:pad + n].reshape(dims), bufs["sdf"][pad:pad + n].reshape(dims),
                hip.read_sdf_grid_info(bufs["info"][pad:pad + 8]))
    d2, face, sdf, info = call(tris, tris.shape[0])
    _same_bits(d2, want_d2, "d2")
    _same_bits(face, want_face, "face")
    _same_bits(sdf, meshing.signed_distance(want_d2, torch.zeros(dims, dtype=torch.bool, device=dev), trunc), "sdf")
    assert info["status"] == 0 and info["band"] == int(torch.isfinite(want_d2).sum()) > 0
    d2, _, _, _ = call(tris, tris.shape[0], want_face_out=False, want_sdf=False)       # NULL face and sdf
    _same_bits(d2, want_d2, "d2 alone")
    d2, face, sdf, info = call(None, 0)                                                 # no triangle
    assert bool((d2 == INF).all()) and bool((face == -1).all()) and bool((sdf == np.float32(trunc)).all())
    assert info == dict.fromkeys(info, 0)
    bad = tris.clone()
    bad[17, 1, 2] = float("nan")
    d2, face, sdf, info = call(bad, bad.shape[0])
    assert info["status"] == 1 and info["band"] == 0
    assert bool(torch.isnan(d2).all()) and bool((face == -1).all()) and bool(torch.isnan(sdf).all())
    bad[17, 1, 2] = float("inf")
    assert call(bad, bad.shape[0])[3]["status"] == 1


@gpu
def test_geometry_mesh_sdf_equals_the_specification_on_f10():
    from arah_release_amd import geometry, hip, meshing
    dev = torch.device(DEV)
    verts, faces, points, contains = f10()
    verts, faces, points = verts.to(torch.float32).to(dev), faces.to(dev), points.to(torch.float32).to(dev)
    for trunc in (INF, 0.05):
        got = geometry.mesh_sdf((verts, faces), points, trunc=trunc)
        want = meshing.mesh_sdf(verts, faces, points, trunc, chunk_pairs=1 << 23)        # the specification, on the same tensors
        for key, w in zip(("d2", "face", "closest", "inside", "ambiguous"), want):
            _same_bits(got[key], w, "trunc %g: %s" % (trunc, key))
        _same_bits(got["sdf"], meshing.signed_distance(want[0], want[3], trunc), "sdf")
        assert set(got) == set(geometry.SDF_KEYS)
    np.testing.assert_array_equal(got["inside"].cpu().numpy(), contains)
    # ... and on the host: the same bits from the same rule
    sel = slice(0, 8256, 16)
    host = geometry.mesh_sdf((verts.cpu(), faces.cpu()), points[sel].cpu(), trunc=0.05)
    for key in geometry.SDF_KEYS:
        if key == "closest":       # its NaNs (outside the band) carry no particular bits
            assert got[key].dtype == host[key].dtype
            np.testing.assert_array_equal(got[key][sel].cpu().numpy(), host[key].numpy(), err_msg="host: " + key)
        elif key == "gradient":    # torch's own sqrt and division on the two devices: components of a unit vector, a few roundings of 2^-53
            assert got[key].dtype == host[key].dtype
            np.testing.assert_allclose(got[key][sel].cpu().numpy(), host[key].numpy(), rtol=0, atol=2.0 ** -50, err_msg="host: " + key)
        else:
            _same_bits(got[key][sel].cpu(), host[key], "host: " + key)
    # the indices may be built once and handed in
    tris = verts[faces.long()].contiguous()
    again = geometry.mesh_sdf((verts, faces), points, trunc=0.05, index=hip.mesh_index(tris), contains_index=hip.contains_index(verts, faces, 512))
    for key in geometry.SDF_KEYS:
        _same_bits(again[key], got[key], "with indices: " + key)


@gpu
def test_geometry_mesh_sdf_grid_and_its_host_path():
    from arah_release_amd import geometry
    dev = torch.device(DEV)
    tris = torch.from_numpy(icosphere(1))
    on_gpu = geometry.mesh_sdf_grid(tris.to(dev), dims=(9, 8, 10), padding=0.2, want_face=True)
    on_host = geometry.mesh_sdf_grid(tris, dims=(9, 8, 10), padding=0.2, want_face=True)
    for key in ("sdf", "d2", "face", "inside", "xs", "ys", "zs"):
        _same_bits(on_gpu[key].cpu(), on_host[key], key)
    assert int(on_gpu["band"]) == int(on_host["band"]) > 0 and on_gpu["trunc"] == on_host["trunc"] and on_gpu["bounds"] == on_host["bounds"]
    assert int(on_gpu["ambiguous"]) == int(on_host["ambiguous"])


@gpu
def test_remesh_of_the_icosphere():
    """A marching-cubes vertex lies on a lattice edge that crosses the level set, hence within one edge length h of it; the level
    `offset` of the distance to a convex body between B(r_in) and B(R) lies between the spheres r_in + offset and R + offset."""
    from arah_release_amd import geometry
    dev = torch.device(DEV)
    tris = icosphere(2)
    r_in, R = sphere_radii(tris)
    mesh = torch.from_numpy(tris).to(dev)
    n = 32
    h = 2.0 / (n - 5)                      # extent 2, two steps of padding on either side
    verts, faces = geometry.remesh(mesh, n_side=n)
    topo = geometry.mesh_topology(verts, faces)
    r = verts.double().norm(dim=1)
    print("remesh: %d vertices, %d faces, radii %.4f .. %.4f for [%.4f, %.4f] +- %.4f" % (verts.shape[0], faces.shape[0], float(r.min()),
                                                                                       float(r.max()), r_in, R, h))
    assert verts.dtype == torch.float32 and faces.dtype == torch.int32 and faces.shape[0] > 1000
    assert topo["watertight"] and topo["euler"] == 2, topo
    assert bool((r >= r_in - h).all()) and bool((r <= R + h).all())
    h = 2.0 / (n - 5 - 3)                  # extent + 2 (delta + 2 h) = (n - 1) h with delta = 1.5 h
    delta = 1.5 * h
    verts, faces = geometry.remesh(mesh, n_side=n, offset=delta, trunc=3.0 * h)
    topo = geometry.mesh_topology(verts, faces)
    r = verts.double().norm(dim=1)
    print("offset %.4f: %d vertices, radii %.4f .. %.4f" % (delta, verts.shape[0], float(r.min()), float(r.max())))
    assert topo["watertight"] and topo["euler"] == 2, topo
    assert bool((r >= r_in + delta - h).all()) and bool((r <= R + delta + h).all())
    # the policies of the other mesh entries
    smooth_v, smooth_f = geometry.remesh(mesh, n_side=n, clean="largest", smooth=2)
    assert smooth_f.shape == geometry.remesh(mesh, n_side=n)[1].shape and geometry.mesh_topology(smooth_v, smooth_f)["watertight"]


# ------------------------------------------------------------------------------------------------------ model level
@gpu
def test_geometry_metrics_with_sdf(scene):
    dev = torch.device(DEV)
    model, _ = get_model("zju377_mono", dev)
    model.eval()
    inputs = scene.make_inputs(32, 32, frame_idx=0, device=dev)
    band = 0.05
    with torch.no_grad():
        tris = model.posed_mesh(inputs, n_side=64)["tris"]
        plain = model.geometry_metrics(inputs, tris, n_side=64, n_samples=20000)
        own = model.geometry_metrics(inputs, tris, n_side=64, n_samples=20000, sdf=5000)
        narrow = model.geometry_metrics(inputs, tris, n_side=64, n_samples=20000, sdf=5000, sdf_band=0.01)
    new = {"sdf_l1", "sdf_sign", "sdf_n", "sdf_ambiguous"}
    assert set(own) == set(plain) | new and not new & set(plain)
    assert all(torch.equal(torch.as_tensor(own[k]), torch.as_tensor(plain[k])) for k in plain)
    print("posed SDF against its own 64^3 mesh: sdf_l1 %.6f m, sdf_sign %.4f, %d of 5000 points, %d ambiguous; band 0.01: sdf_l1 %.6f m, "
          "sdf_sign %.4f" % (float(own["sdf_l1"]), float(own["sdf_sign"]), int(own["sdf_n"]), int(own["sdf_ambiguous"]),
                             float(narrow["sdf_l1"]), float(narrow["sdf_sign"])))
    assert 0 < int(own["sdf_n"]) <= 5000 and 0.0 <= float(own["sdf_sign"]) <= 1.0 and 0 <= int(own["sdf_ambiguous"]) <= int(own["sdf_n"])
    # two values both clamped to [-band, band] differ by at most the band's width
    assert np.isfinite(float(own["sdf_l1"])) and float(own["sdf_l1"]) < 2.0 * band
    assert np.isfinite(float(narrow["sdf_l1"])) and float(narrow["sdf_l1"]) < 2.0 * 0.01
    with pytest.raises(ValueError):
        model.geometry_metrics(inputs, tris.reshape(-1, 3), n_side=64, n_samples=20000, sdf=1000)      # a scan has no sign
    for bad in ({"sdf": 0}, {"sdf": 100, "sdf_band": 0.0}, {"sdf": 100, "sdf_band": INF}):
        with pytest.raises(ValueError):
            model.geometry_metrics(inputs, tris, n_side=64, n_samples=20000, **bad)


@gpu
def test_validate_with_geometry_sdf(tmp_path, scene, monkeypatch):
    """validate --geometry DIR --geometry-sdf N: one frame against its own posed mesh, one against a scan, one without ground truth."""
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
    validate.main(argv + common + ["--geometry-sdf", "5000", "--geometry-sdf-band", "0.04"], body=body, faces=faces, log=lines.append)
    line = json.loads(lines[-1])
    print("validate --geometry-sdf:", lines[-1])
    new = {"sdf_l1", "sdf_sign"}
    assert set(line) == set(without) | new and not new & set(without)
    assert 0.0 <= line["sdf_l1"] < 2.0 * 0.04 and 0.0 <= line["sdf_sign"] <= 1.0 and line["n_geometry"] == 2
    assert all(line[k] == without[k] for k in without if k != "seconds_per_frame")
    frames = json.load(open(tmp_path / "out" / "validation.json"))["frames"]
    assert set(frames[0]) == set(frames_without[0]) | new and frames[0]["sdf_l1"] == line["sdf_l1"]
    assert set(frames[2]) == set(frames_without[2]) and set(frames[1]) == set(frames_without[1])          # a scan, and no ground truth
    with pytest.raises(ValueError):
        validate.main(argv + ["--geometry-sdf", "5000"], body=body, faces=faces, log=lines.append)
