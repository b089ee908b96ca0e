"""Indexed meshes (shared vertices) from marching cubes: arah_marching_cubes_indexed (csrc/mcubes.hpp), its tensor specification
meshing.marching_cubes_indexed, MetaAvatarRender.posed_mesh(indexed=True) / canonical_mesh and geometry.save_mesh.

A marching-cubes vertex lies on a lattice edge; the vertices are the crossing edges in ascending order of their integer key
((ix n + iy) n + iz) 3 + axis, the faces are the soup's triangles as vertex ids.  CPU tests hold the specification to the soup
extraction, to an independent count of the crossing edges and to the topology of known shapes; GPU tests hold the kernel to the
specification and to the soup kernel, bit for bit."""
import os
import re
from collections import Counter

import numpy as np
import pytest
import torch

from conftest import REPO, get_model

gpu = pytest.mark.gpu
DEV = "cuda:0"


# ---- fields on the lattice of [-1,1]^3 -------------------------------------------------------------------------------------
def _lattice(n):
    ax = torch.linspace(-1, 1, n)
    return torch.meshgrid(ax, ax, ax, indexing="ij")


def sphere(n, radius=0.7123):
    X, Y, Z = _lattice(n)
    return torch.sqrt(X ** 2 + Y ** 2 + Z ** 2) - radius


def torus(n):
    X, Y, Z = _lattice(n)
    return torch.sqrt((torch.sqrt(X ** 2 + Y ** 2) - 0.55) ** 2 + Z ** 2) - 0.2371


def two_blobs(n):
    X, Y, Z = _lattice(n)
    a = torch.sqrt((X - 0.4) ** 2 + Y ** 2 + Z ** 2) - 0.31
    b = torch.sqrt((X + 0.4) ** 2 + Y ** 2 + Z ** 2) - 0.27
    return torch.minimum(a, b)


def noise(n=20, seed=11):
    v = torch.randn(n, n, n, generator=torch.Generator().manual_seed(seed))
    v[0], v[-1], v[:, 0], v[:, -1], v[:, :, 0], v[:, :, -1] = 1, 1, 1, 1, 1, 1
    return v


def quantised(n):
    """Many lattice values exactly at the level: crossing points at t = 0, degenerate triangles."""
    X, Y, Z = _lattice(n)
    return torch.round(4.0 * (torch.sqrt(X ** 2 + Y ** 2 + Z ** 2) - 0.55)) / 4.0


def one_corner():
    v = torch.ones(2, 2, 2)
    v[0, 0, 0] = -1.0
    return v


FIELDS = {"sphere3": lambda: sphere(3), "sphere17": lambda: sphere(17), "sphere33": lambda: sphere(33),
          "torus33": lambda: torus(33), "blobs33": lambda: two_blobs(33), "noise20": noise}
SIZES = {"sphere3": (6, 8), "sphere17": (606, 1208), "sphere33": (2430, 4856), "torus33": (1840, 3680), "blobs33": (804, 1600)}
EULER = {"sphere3": 2, "sphere17": 2, "sphere33": 2, "torus33": 0, "blobs33": 4}


def crossing_edges(sdf, level=0.0):
    """The number of sign-changing lattice edges, by three shifted comparisons."""
    i = sdf < level
    return int((i[1:] != i[:-1]).sum()) + int((i[:, 1:] != i[:, :-1]).sum()) + int((i[:, :, 1:] != i[:, :, :-1]).sum())


def edge_counts(faces):
    f = faces.tolist()
    directed = Counter((t[i], t[(i + 1) % 3]) for t in f for i in range(3))
    undirected = Counter(frozenset(e) for e in directed.elements())
    return directed, undirected


_SPEC = {}


def spec(name):
    """(sdf, verts, faces, vert_edge, soup) of a named field on the host, computed once and shared; never modified."""
    from arah_release_amd import meshing
    if name not in _SPEC:
        sdf = FIELDS[name]()
        _SPEC[name] = (sdf,) + tuple(meshing.marching_cubes_indexed(sdf)) + (meshing.marching_cubes(sdf),)
    return _SPEC[name]


# ---- CPU: the tensor specification -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FIELDS))
def test_spec_is_the_soup_with_one_vertex_per_crossing_edge(name):
    sdf, verts, faces, vert_edge, soup = spec(name)
    n = sdf.shape[0]
    assert faces.dtype == torch.int64 and vert_edge.dtype == torch.int64
    assert torch.equal(verts[faces], soup)
    assert verts.shape[0] == vert_edge.shape[0] == crossing_edges(sdf)
    assert bool((vert_edge[1:] > vert_edge[:-1]).all())
    point, axis = vert_edge // 3, vert_edge % 3
    lo = torch.stack([point // (n * n), (point // n) % n, point % n], 1)
    hi = lo + torch.nn.functional.one_hot(axis, 3)
    assert int(hi.max()) < n
    inside = sdf < 0.0
    assert bool((inside[lo[:, 0], lo[:, 1], lo[:, 2]] != inside[hi[:, 0], hi[:, 1], hi[:, 2]]).all())
    assert torch.equal(torch.unique(faces), torch.arange(verts.shape[0]))      # every vertex is referenced by a face


@pytest.mark.parametrize("name", sorted(SIZES))
def test_spec_sizes_and_topology_of_smooth_fields(name):
    sdf, verts, faces, _, soup = spec(name)
    V, F = verts.shape[0], faces.shape[0]
    assert (V, F) == SIZES[name] and soup.shape[0] == F
    directed, undirected = edge_counts(faces)
    assert set(undirected.values()) == {2} and set(directed.values()) == {1}   # closed, oriented 2-manifold
    assert V - len(undirected) + F == EULER[name]


def test_spec_noise_volume_has_no_boundary_edges():
    _, _, faces, _, _ = spec("noise20")
    _, undirected = edge_counts(faces)
    assert 1 not in undirected.values() and 3 not in undirected.values()


def test_spec_level_and_empty_volume():
    from arah_release_amd import meshing
    sdf = sphere(17)
    verts, faces, vert_edge = meshing.marching_cubes_indexed(sdf, 0.05)
    assert torch.equal(verts[faces], meshing.marching_cubes(sdf, 0.05)) and verts.shape[0] == crossing_edges(sdf, 0.05)
    verts, faces, vert_edge = meshing.marching_cubes_indexed(torch.ones(5, 5, 5))
    assert verts.shape == (0, 3) and faces.shape == (0, 3) and vert_edge.shape == (0,)
    v, f = meshing.indexed_mesh(sphere(17))                                     # a volume on the host: the specification
    assert torch.equal(v, spec("sphere17")[1]) and torch.equal(f, spec("sphere17")[2])


@pytest.mark.parametrize("ext", [".npz", ".ply"])
@pytest.mark.parametrize("attrs", [False, True])
def test_save_mesh_round_trip(tmp_path, ext, attrs):
    from arah_release_amd import geometry
    _, verts, faces, _, _ = spec("sphere17")
    g = torch.Generator().manual_seed(1)
    normals = torch.nn.functional.normalize(torch.randn(verts.shape[0], 3, generator=g), dim=1) if attrs else None
    colors = torch.rand(verts.shape[0], 3, generator=g) if attrs else None
    path = str(tmp_path / ("mesh" + ext))
    geometry.save_mesh(path, verts, faces.to(torch.int32), normals=normals, colors=colors)
    v, f = geometry.load_mesh(path)
    assert v.dtype == torch.float32 and torch.equal(v, verts) and torch.equal(f, faces)
    if ext == ".ply":
        header = open(path, "rb").read().split(b"end_header")[0].decode("ascii")
        assert "format binary_little_endian 1.0" in header
        assert ("property float nx" in header and "property float nz" in header) == attrs
        assert ("property uchar red" in header and "property uchar blue" in header) == attrs
    elif attrs:
        with np.load(path) as z:
            assert np.array_equal(z["normals"], normals.numpy()) and np.array_equal(z["colors"], colors.numpy())


def test_save_mesh_rejects_bad_input(tmp_path):
    from arah_release_amd import geometry
    _, verts, faces, _, _ = spec("sphere3")
    with pytest.raises(ValueError):
        geometry.save_mesh(str(tmp_path / "mesh.obj"), verts, faces)
    with pytest.raises(ValueError):
        geometry.save_mesh(str(tmp_path / "mesh.ply"), verts, faces, normals=torch.zeros(verts.shape[0] + 1, 3))
    with pytest.raises(ValueError):
        geometry.save_mesh(str(tmp_path / "mesh.npz"), verts, faces, colors=torch.zeros(verts.shape[0] - 1, 3))
    bad = faces.clone()
    bad[0, 0] = verts.shape[0]
    with pytest.raises(ValueError):
        geometry.save_mesh(str(tmp_path / "mesh.ply"), verts, bad)
    bad[0, 0] = -1
    with pytest.raises(ValueError):
        geometry.save_mesh(str(tmp_path / "mesh.npz"), verts, bad)
    assert not os.listdir(str(tmp_path))                                        # nothing half-written


def test_indexed_symbols_are_declared_and_exported():
    from arah_release_amd import hip
    header = open(os.path.join(REPO, "include", "arah_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("arah_marching_cubes_indexed_scratch_bytes", "arah_marching_cubes_indexed"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in hip.EXPORTS, name


# ---- GPU: the kernel against the specification and the soup kernel ----------------------------------------------------------
def _outside_sphere(n):
    return sphere(n, 1.2)                         # leaves the lattice through all six faces: crossings on the last layers


KERNEL_CASES = {
    "one_corner_n2": (one_corner, 0.0), "sphere_n3": (lambda: sphere(3), 0.0), "sphere_n33": (lambda: sphere(33), 0.0),
    "torus_n65": (lambda: torus(65), 0.0), "blobs_n66": (lambda: two_blobs(66), 0.0), "sphere_n258": (lambda: sphere(258), 0.0),
    "leaves_lattice_n33": (lambda: _outside_sphere(33), 0.0), "quantised_n33": (lambda: quantised(33), 0.0),
    "level_n33": (lambda: torus(33), 0.05), "all_positive_n9": (lambda: torch.ones(9, 9, 9), 0.0), "noise_n20": (noise, 0.0),
}


@gpu
@pytest.mark.parametrize("case", sorted(KERNEL_CASES))
def test_indexed_kernel_is_the_specification_and_the_soup(case):
    from arah_release_amd import hip, meshing
    make, level = KERNEL_CASES[case]
    sdf = make()
    rv, rf, re_ = meshing.marching_cubes_indexed(sdf, level)
    V, F = rv.shape[0], rf.shape[0]
    if case == "one_corner_n2":
        assert (V, F) == (3, 1)
    if case == "all_positive_n9":
        assert (V, F) == (0, 0)
    if case == "leaves_lattice_n33":   # crossing edges whose lower end lies on the last layer of another axis, all three axes
        n = sdf.shape[0]
        p, a = re_ // 3, re_ % 3
        idx = torch.stack([p // (n * n), (p // n) % n, p % n], 1)
        for axis in range(3):
            assert bool(((idx[:, axis] == n - 1) & (a != axis)).any())
    if case == "quantised_n33":
        assert int((sdf == 0).sum()) > 100
    d = sdf.to(DEV)
    vc, fc = V + 37, F + 53
    verts, faces, counts, edge = hip.marching_cubes_indexed(d, level, vert_cap=vc, face_cap=fc, want_edge=True)
    soup, n_soup = hip.marching_cubes(d, level, cap=fc)
    assert counts.tolist() == [V, F] and int(n_soup.item()) == F
    assert verts.shape == (vc, 3) and faces.shape == (fc, 3) and faces.dtype == torch.int32 and edge.dtype == torch.int32
    assert torch.equal(verts[:V].cpu(), rv) and torch.equal(edge[:V].cpu().long(), re_)
    assert not bool(verts[V:].any()) and not bool(edge[V:].any()) and not bool(faces[F:].any())
    assert bool(((faces[:F] >= 0) & (faces[:F] < max(V, 1))).all())
    assert torch.equal(verts[faces[:F].long()], soup[:F])                       # the soup kernel's triangles, its own flips
    got = faces[:F].cpu().long()
    same = (got == rf).all(-1)
    flipped = (got[:, [0, 2, 1]] == rf).all(-1)
    assert bool((same | flipped).all())
    tri = rv[rf]
    area = torch.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], dim=1).norm(dim=1)
    assert bool((area[~same] < 1e-9).all()), int((~same).sum())                 # the corner swap on degenerate triangles only


@gpu
def test_indexed_kernel_respects_its_caps():
    from arah_release_amd import hip
    _, rv, rf, _, _ = spec("torus33")
    V, F = rv.shape[0], rf.shape[0]
    d = torus(33).to(DEV)
    full_v, full_f, _, full_e = hip.marching_cubes_indexed(d, 0.0, vert_cap=V + 10, face_cap=F + 10, want_edge=True)
    lib = hip.load_library()
    import ctypes as C
    vc, fc, guard = V // 2, F // 2, 64
    nan_bits = 0x7FC00BAD
    table, ntri = hip._mc_device_tables(d.device)
    for cap_v, cap_f in ((vc, fc), (V + 5, F + 7)):
        verts = torch.full(((cap_v + guard) * 3,), nan_bits, dtype=torch.int32, device=DEV)
        edge = torch.full((cap_v + guard,), nan_bits, dtype=torch.int32, device=DEV)
        faces = torch.full(((cap_f + guard) * 3,), nan_bits, dtype=torch.int32, device=DEV)
        counts = torch.zeros(2, dtype=torch.int32, device=DEV)
        scratch = torch.empty(int(lib.arah_marching_cubes_indexed_scratch_bytes(33)), dtype=torch.uint8, device=DEV)
        with hip._on_device(d.device):
            hip._check(lib.arah_marching_cubes_indexed(hip._ptr(d), C.c_int32(33), C.c_float(0.0), hip._ptr(table), hip._ptr(ntri),
                                                       hip._ptr(verts), C.c_int32(cap_v), hip._ptr(edge), hip._ptr(faces),
                                                       C.c_int32(cap_f), hip._ptr(counts), hip._ptr(scratch),
                                                       C.c_size_t(scratch.numel()), hip._stream()), "arah_marching_cubes_indexed")
        assert counts.tolist() == [V, F]                                        # the true sizes, whatever the caps
        kv, kf = min(V, cap_v), min(F, cap_f)
        assert torch.equal(verts[:kv * 3].view(torch.float32), full_v[:kv].reshape(-1))
        assert torch.equal(edge[:kv], full_e[:kv]) and torch.equal(faces[:kf * 3], full_f[:kf].reshape(-1))
        assert not bool(verts[kv * 3:cap_v * 3].any()) and not bool(edge[kv:cap_v].any()) and not bool(faces[kf * 3:cap_f * 3].any())
        for buf, cap, width in ((verts, cap_v, 3), (edge, cap_v, 1), (faces, cap_f, 3)):
            assert bool((buf[cap * width:] == nan_bits).all())                  # nothing written beyond a cap
    # the ABI's argument checks
    with hip._on_device(d.device):
        args = lambda n, cv, cf, sb: lib.arah_marching_cubes_indexed(
            hip._ptr(d), C.c_int32(n), C.c_float(0.0), hip._ptr(table), hip._ptr(ntri), hip._ptr(verts), C.c_int32(cv), None,
            hip._ptr(faces), C.c_int32(cf), hip._ptr(counts), hip._ptr(scratch), C.c_size_t(sb), hip._stream())
        assert args(1, 8, 8, scratch.numel()) == -1 and args(895, 8, 8, scratch.numel()) == -1      # ARAH_E_BADARG
        assert args(33, 0, 8, scratch.numel()) == -1 and args(33, 8, 0, scratch.numel()) == -1
        assert args(33, 8, 8, scratch.numel() - 1) == -3                                              # ARAH_E_WORKSPACE
    assert lib.arah_marching_cubes_indexed_scratch_bytes(894) > 0 and lib.arah_marching_cubes_indexed_scratch_bytes(895) == 0
    with pytest.raises(ValueError):
        hip.marching_cubes_indexed(d, 0.0, vert_cap=0)
    torch.cuda.synchronize()


@gpu
def test_indexed_kernel_is_deterministic_and_isolated():
    from arah_release_amd import hip
    d33, d129 = sphere(33).to(DEV), two_blobs(129).to(DEV)
    _, rv, rf, re_, _ = spec("sphere33")
    caps = dict(vert_cap=rv.shape[0] + 11, face_cap=rf.shape[0] + 13, want_edge=True)
    hip._mc_indexed_scratch.clear()
    fresh = hip.marching_cubes_indexed(d33, **caps)
    again = hip.marching_cubes_indexed(d33, **caps)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = hip.marching_cubes_indexed(d33, **caps)
    side.synchronize()
    big = hip.marching_cubes_indexed(d129, vert_cap=1 << 16, face_cap=1 << 17)
    assert big[2].tolist()[0] > rv.shape[0]
    key = (torch.device(DEV), torch.cuda.current_stream().cuda_stream)
    grown = hip._mc_indexed_scratch[key]
    after = hip.marching_cubes_indexed(d33, **caps)                             # on the scratch the n = 129 call left behind
    assert hip._mc_indexed_scratch[key] is grown
    for run in (again, other, after):
        for a, b in zip(fresh, run):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(fresh[0][:rv.shape[0]].cpu(), rv) and torch.equal(fresh[1][:rf.shape[0]].cpu().long(), rf)


# ---- GPU: the model's entries ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def subject(scene):
    dev = torch.device(DEV)
    model, _ = get_model("zju377_mono", dev)
    model.eval()
    return model, scene.make_inputs(32, 32, frame_idx=0, device=dev)


@gpu
@pytest.mark.parametrize("method", ["lattice", "skinned"])
def test_posed_mesh_indexed_is_the_soup(subject, method, tmp_path):
    from arah_release_amd import geometry
    model, inputs = subject
    with torch.no_grad():
        soup = model.posed_mesh(inputs, n_side=128, method=method)
        mesh = model.posed_mesh(inputs, n_side=128, method=method, indexed=True)
    assert "tris" not in mesh and mesh["n_tris"] == soup["n_tris"] > 500
    verts, faces = mesh["verts"], mesh["faces"]
    assert verts.shape == (mesh["n_verts"], 3) and faces.shape == (mesh["n_tris"], 3)
    assert mesh["n_verts"] < mesh["n_tris"]                                     # V ~ F / 2: shared, not 3 F corners
    assert torch.equal(verts[faces.long()], soup["tris"])
    if method == "lattice":
        assert torch.equal(mesh["box"], soup["box"]) and torch.equal(mesh["counts"], soup["counts"])
        # the pair IS the soup, so it scores as the soup scores against itself: zero up to the float32 rounding of a sample
        # point (the bound of test_geometry_metrics for a mesh against itself), and the same bits
        res = geometry.mesh_metrics((verts, faces), soup["tris"], n_samples=20000)
        own = geometry.mesh_metrics(soup["tris"], soup["tris"], n_samples=20000)
        tol = np.sqrt(3) * 4 * 2.0 ** -24 * float(soup["tris"].abs().max())
        for k in ("accuracy", "completeness", "chamfer_l1", "hausdorff_ab", "hausdorff_ba"):
            assert float(res[k]) <= tol and torch.equal(res[k], own[k]), k
        for ext in (".npz", ".ply"):
            path = str(tmp_path / ("posed" + ext))
            geometry.save_mesh(path, verts, faces)
            v, f = geometry.load_mesh(path, device=verts.device)
            assert torch.equal(v, verts) and torch.equal(f, faces.long())


@gpu
def test_canonical_mesh_and_its_attributes(subject):
    from arah_release_amd import hip, meshing, training
    model, inputs = subject
    with torch.no_grad():
        plain = model.canonical_mesh(inputs, n_side=128)
        mesh = model.canonical_mesh(inputs, n_side=128, attributes=("weights", "verts_posed", "normal", "color"))
        frame, ws = model._posed_frame(inputs, "test")
        tri, posed, n_dev = meshing.skinned_mesh(frame, ws, inputs, 128, cap=1 << 18)   # the reference-style posed soup
        n = int(n_dev.item())
        verts, faces, V = mesh["verts"], mesh["faces"].long(), mesh["n_verts"]
        assert set(plain) == {"verts", "faces", "n_verts", "n_tris"} and torch.equal(plain["verts"], verts)
        assert mesh["n_tris"] == n > 500 and V == verts.shape[0] < n
        assert torch.equal(verts[faces], tri[:n]) and float(verts.abs().max()) <= 1.0
        assert torch.equal(mesh["verts_posed"][faces], posed[:n])
        x_hat = training.unnormalize_canonical_points(verts.reshape(1, -1, 3), inputs["coord_min"][:1], inputs["coord_max"][:1],
                                                      inputs["center"][:1])[0]
        w, _, _ = hip.skin_lbs(frame, ws, x_hat)
        assert mesh["weights"].shape == (V, 24) and torch.equal(mesh["weights"], w)
        # unit length to the rounding of a float32 normalisation: 3 squares, 2 sums, a square root and a division
        assert float((mesh["normal"].norm(dim=1) - 1.0).abs().max()) <= 8 * 2.0 ** -24
        # ... up the gradient, out of the body (a sign check: the faces' right-hand normals point down the gradient)
        fn = -meshing.face_normals(tri[:n])
        assert float((fn * mesh["normal"][faces[:, 0]]).sum(1).mean()) > 0.0
        color = mesh["color"]
        assert color.shape == (V, 3) and bool(torch.isfinite(color).all()) and float(color.min()) >= 0.0 and float(color.max()) <= 1.0
        fixed = model.canonical_mesh(inputs, n_side=128, attributes=("color",), view_dirs=(0.0, 0.0, 1.0))["color"]
        assert fixed.shape == (V, 3) and float(fixed.min()) >= 0.0 and float(fixed.max()) <= 1.0
    with pytest.raises(ValueError):
        model.canonical_mesh(inputs, attributes=("nope",))
    model.train()
    try:
        with pytest.raises(ValueError):
            model.canonical_mesh(inputs)
    finally:
        model.eval()
