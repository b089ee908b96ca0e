"""Laplacian / Taubin smoothing of indexed meshes: arah_mesh_smooth (csrc/meshadj.hpp), its tensor specification
meshing.mesh_smooth, geometry.smooth_mesh / check_smooth and the `smooth` option of MetaAvatarRender.posed_mesh /
canonical_mesh with its "vertex_normal" attribute.  (The adjacency it runs over: tests/test_mesh_adjacency.py.)

A step sums a vertex's finite neighbours in ascending id in float64, every operation rounded on its own: the result is unique.
CPU tests hold the specification to a restatement in python floats and to what smoothing must do (pin boundaries, leave NaN
vertices alone, denoise without shrinking); GPU tests hold the kernel to the specification bit for bit."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from conftest import get_model
from test_mesh_adjacency import ALL_MESHES, DEV, mesh, restated, spec

gpu = pytest.mark.gpu
RADIUS = 0.7123


# ---- an independent restatement ---------------------------------------------------------------------------------------------------
def py_smooth(verts, neighbours, flags, factors, pin):
    """The ordered steps once more, in python floats (IEEE doubles, one rounding per operation): factors one per step."""
    cur = np.asarray(verts, np.float32).copy()
    finite = lambda p: all(math.isfinite(x) for x in p)
    for f in factors:
        f = float(np.float32(f))
        rows = cur.tolist()                                                       # float32 values as python floats: exact
        new = cur.copy()
        for v, p in enumerate(rows):
            if not finite(p) or (pin and flags[v] & 3):
                continue
            s, m = [0.0, 0.0, 0.0], 0
            for n in neighbours[v]:
                q = rows[n]
                if finite(q):
                    s = [s[a] + q[a] for a in range(3)]
                    m += 1
            if m:
                new[v] = [np.float32(p[a] + f * (s[a] / m - p[a])) for a in range(3)]
        cur = new
    return cur


def bits(t):
    return (t if isinstance(t, np.ndarray) else t.cpu().numpy()).view(np.int32)


def nan_mesh():
    """sphere17 with a few vertices that are not numbers: they stay, and their neighbours do without them."""
    verts, faces = mesh("sphere17")
    verts = verts.clone()
    verts[5, 1] = float("nan")
    verts[77] = float("inf")
    verts[300, 2] = float("-inf")
    verts[301, 0] = float("nan")
    return verts, faces


# ---- CPU: the specification ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_MESHES)
def test_spec_is_the_restatement(name):
    from arah_release_amd import meshing
    verts, faces = mesh(name)
    ref = restated(name)
    # the fan's apex makes the specification's padded gather 4097 wide: one iteration there, two elsewhere
    n = 1 if name == "fan4096" else 2
    for method, factors in (("taubin", (0.5, -0.53) * n), ("laplacian", (0.63,) * n)):
        for boundary in ("pin", "free"):
            got = meshing.mesh_smooth(verts, faces, n, lamb=factors[0], mu=-0.53, method=method, boundary=boundary, adjacency=spec(name))
            want = py_smooth(verts.numpy(), ref["neighbours"], ref["vert_flags"].tolist(), factors, boundary == "pin")
            assert got.dtype == torch.float32 and got.shape == verts.shape
            assert np.array_equal(bits(got), bits(want)), (method, boundary)


def test_spec_on_vertices_that_are_not_numbers():
    from arah_release_amd import meshing
    verts, faces = nan_mesh()
    ref = restated("sphere17")
    got = meshing.mesh_smooth(verts, faces, 3)
    want = py_smooth(verts.numpy(), ref["neighbours"], ref["vert_flags"].tolist(), (0.5, -0.53) * 3, True)
    assert np.array_equal(bits(got), bits(want))
    bad = ~torch.isfinite(verts).all(1)
    assert bad.sum() == 4 and np.array_equal(bits(got[bad]), bits(verts[bad]))     # a NaN vertex stays, bit for bit
    assert torch.isfinite(got[~bad]).all()                                         # ... and poisons nobody
    clean = meshing.mesh_smooth(mesh("sphere17")[0], faces, 3)
    near = torch.zeros(verts.shape[0], dtype=torch.bool)
    for v in torch.nonzero(bad)[:, 0].tolist():
        near[ref["neighbours"][v]] = True
    near &= ~bad
    assert (got[near] != verts[near]).any(1).all()                                 # ... nor stops its neighbours
    assert (got[near] != clean[near]).any(1).all()                                 # which do without it


def test_spec_identity_pins_and_isolated_vertices():
    from arah_release_amd import geometry, meshing
    verts, faces = mesh("clipped17")
    flags = spec("clipped17")[6]
    on_boundary = (flags & 1) != 0
    assert spec("clipped17")[7][2].item() == 264 and on_boundary.sum() == 264      # six circles: as many vertices as edges
    same = meshing.mesh_smooth(verts, faces, 0)
    assert np.array_equal(bits(same), bits(verts)) and same.data_ptr() != verts.data_ptr()
    pinned = meshing.mesh_smooth(verts, faces, 10, boundary="pin")
    assert np.array_equal(bits(pinned[on_boundary]), bits(verts[on_boundary]))
    assert (pinned[~on_boundary] != verts[~on_boundary]).any(1).all()
    free = meshing.mesh_smooth(verts, faces, 10, boundary="free")
    assert (free[on_boundary] != verts[on_boundary]).any()
    assert torch.equal(geometry.smooth_mesh(verts, faces), pinned)                 # the defaults: 10 Taubin iterations, pinned
    assert torch.equal(geometry.smooth_mesh(verts, faces, adjacency=geometry.mesh_adjacency(verts, faces), boundary="free"), free)
    # non-manifold edges pin their ends as well
    verts, faces = mesh("three_on_edge")
    out = meshing.mesh_smooth(verts, faces, 1, method="laplacian")
    assert torch.equal(out, verts)                                                 # every vertex is on a boundary or the triple edge
    out = meshing.mesh_smooth(verts, faces, 1, method="laplacian", boundary="free")
    assert (out != verts).any(1).all()
    # isolated vertices stay, among vertices that move
    verts, faces = mesh("isolated_between")
    out = meshing.mesh_smooth(verts, faces, 4, boundary="free")
    lonely = (spec("isolated_between")[6] & 4) != 0
    assert lonely.sum() == 4 and torch.equal(out[lonely], verts[lonely]) and (out[~lonely] != verts[~lonely]).any(1).all()
    for name in ("empty", "no_faces"):
        verts, faces = mesh(name)
        assert torch.equal(meshing.mesh_smooth(verts, faces, 3), verts)


def test_taubin_denoises_without_shrinking():
    """Radial noise of 0.3 lattice steps on sphere(33): 10 Taubin iterations bring the RMS of |p| - R from 0.0188 to 0.0070 and move
    the mean radius by 5e-4; 20 Laplacian steps at the same lamb shrink it by 2.3e-2.  Asserted: the two inequalities."""
    from arah_release_amd import meshing
    verts, faces = mesh("sphere33")
    g = torch.Generator().manual_seed(33)
    r = verts.norm(dim=1, keepdim=True)
    noisy = (verts + verts / r * (0.3 * (2.0 / 32) * torch.randn(verts.shape[0], 1, generator=g))).contiguous()
    adj = spec("sphere33")
    radius = lambda p: p.double().norm(dim=1)
    rms = lambda p: float(((radius(p) - RADIUS) ** 2).mean().sqrt())
    taubin = meshing.mesh_smooth(noisy, faces, 10, adjacency=adj)
    laplace = meshing.mesh_smooth(noisy, faces, 20, method="laplacian", adjacency=adj)
    drift = lambda p: abs(float(radius(p).mean() - radius(noisy).mean()))
    print("rms in %.4f taubin %.4f laplacian %.4f; drift taubin %.2e laplacian %.2e"
          % (rms(noisy), rms(taubin), rms(laplace), drift(taubin), drift(laplace)))
    assert rms(taubin) < rms(noisy)
    assert drift(taubin) < drift(laplace)


def test_arguments():
    from arah_release_amd import geometry, meshing
    verts, faces = mesh("sphere17")
    adj = spec("sphere17")
    for fn in (meshing.mesh_smooth, geometry.smooth_mesh):
        for bad in (lambda: fn(verts, faces, -1), lambda: fn(verts, faces, 2.0), lambda: fn(verts, faces, True), lambda: fn(verts, faces, None),
                    lambda: fn(verts, faces, 1, lamb=0.0), lambda: fn(verts, faces, 1, lamb=1.01), lambda: fn(verts, faces, 1, lamb=float("nan")),
                    lambda: fn(verts, faces, 1, lamb="half"), lambda: fn(verts, faces, 1, mu=0.0), lambda: fn(verts, faces, 1, mu=-1.2),
                    lambda: fn(verts, faces, 1, mu=0.3), lambda: fn(verts, faces, 1, method="cotan"), lambda: fn(verts, faces, 1, boundary="fixed"),
                    lambda: fn(verts.reshape(-1), faces, 1), lambda: fn(verts, faces.float(), 1), lambda: fn(verts, faces.reshape(-1), 1),
                    lambda: fn(verts.long(), faces, 1), lambda: fn(verts, faces, 1, adjacency=adj[:7]), lambda: fn(verts[:-1], faces, 1, adjacency=adj)):
            with pytest.raises(ValueError):
                bad()
    with pytest.raises(ValueError):
        meshing.mesh_smooth(verts.double(), faces, 1)
    assert geometry.smooth_mesh(verts.double(), faces, 1).dtype == torch.float32   # narrowed, like simplify_mesh
    assert torch.equal(meshing.mesh_smooth(verts, faces, 1, lamb=1.0, mu=-1.1), meshing.mesh_smooth(verts, faces.to(torch.int32), 1, lamb=1, mu=-1.1))
    # check_smooth: None, a number of iterations, a dict of the keywords
    assert geometry.check_smooth(None) is None and geometry.check_smooth(3) == {"iterations": 3} and geometry.check_smooth(0) == {"iterations": 0}
    how = {"iterations": 4, "lamb": 0.3, "mu": -0.31, "method": "laplacian", "boundary": "free"}
    assert geometry.check_smooth(how) == how and geometry.check_smooth(how) is not how and geometry.check_smooth({}) == {}
    for bad in (-1, 2.5, True, "a little", (3,), {"iterations": -2}, {"steps": 3}, {"lamb": 0.0}, {"mu": 0.1}, {"method": "cotan"},
                {"boundary": None}, {"iterations": 1.5}):
        with pytest.raises(ValueError):
            geometry.check_smooth(bad)


def test_model_entries_refuse_smooth_on_a_soup():
    model, _ = get_model("zju377_mono")
    model.eval()
    with pytest.raises(ValueError, match="indexed=True"):                         # refused before the frame is looked at
        model.posed_mesh({}, smooth=3)
    with pytest.raises(ValueError, match="smooth"):
        model.posed_mesh({}, indexed=True, smooth={"iterations": 3, "weights": "cotan"})
    with pytest.raises(ValueError, match="smooth"):
        model.canonical_mesh({}, smooth=-1)
    with pytest.raises(ValueError, match="unknown attributes"):
        model.canonical_mesh({}, attributes=("face_normal",))


# ---- GPU: the kernel against the specification ----------------------------------------------------------------------------------
def _smooth_meshes(name):
    return nan_mesh() if name == "nan_verts" else mesh(name)


@gpu
@pytest.mark.parametrize("name", ["sphere17", "clipped17", "noise20", "torus33_s", "nan_verts", "fan4096", "bad_faces"])
def test_kernel_is_the_specification(name):
    from arah_release_amd import hip, meshing
    verts, faces = _smooth_meshes(name)
    adj = spec("sphere17" if name == "nan_verts" else name)
    v, f, dadj = verts.to(DEV), faces.to(DEV), tuple(t.to(DEV) for t in adj)
    # odd and even step counts: the final buffer.  The fan's apex makes the specification's padded gather 4097 wide: one iteration
    for iterations in ((1,) if name == "fan4096" else (1, 2, 7)):
        for method in ("taubin", "laplacian"):
            for boundary in ("pin", "free"):
                want = meshing.mesh_smooth(verts, faces, iterations, method=method, boundary=boundary, adjacency=adj)
                got = hip.mesh_smooth(v, f, iterations, method=method, boundary=boundary, adjacency=dadj)
                assert got.dtype == torch.float32 and got.is_cuda
                assert np.array_equal(bits(got), bits(want)), (iterations, method, boundary)
    assert np.array_equal(bits(v), bits(verts))                                    # the input is never written
    if name != "fan4096":
        got = hip.mesh_smooth(v, f.to(torch.int32), 3, lamb=0.7, mu=-0.71)         # builds its own adjacency
        assert np.array_equal(bits(got), bits(meshing.mesh_smooth(verts, faces, 3, lamb=0.7, mu=-0.71, adjacency=adj)))
    same = hip.mesh_smooth(v, f, 0, adjacency=dadj)
    assert np.array_equal(bits(same), bits(verts)) and same.data_ptr() != v.data_ptr()


@gpu
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 1025])
def test_kernel_is_the_specification_round_the_launch_geometry(n):
    from arah_release_amd import hip, meshing
    verts, faces = mesh("noise20")
    low = faces[(faces < n).all(1)]
    for f, V in ((faces[:n], verts.shape[0]), (faces, n), (low, n)):
        v = verts[:V].contiguous()
        want = meshing.mesh_smooth(v, f, 2, boundary="free")
        got = hip.mesh_smooth(v.to(DEV), f.to(DEV), 2, boundary="free")
        assert got.shape == (V, 3) and np.array_equal(bits(got), bits(want))


@gpu
def test_device_smoothing_is_the_host_and_shares_an_adjacency():
    from arah_release_amd import geometry
    verts, faces = mesh("torus33")
    v, f = verts.to(DEV), faces.to(DEV).to(torch.int32)
    adj = geometry.mesh_adjacency(v, f)
    for how in ({}, {"iterations": 3, "method": "laplacian", "lamb": 0.25}, {"iterations": 2, "boundary": "free", "mu": -0.6}):
        want = geometry.smooth_mesh(verts, faces, **how)
        assert np.array_equal(bits(geometry.smooth_mesh(v, f, **how)), bits(want))
        assert np.array_equal(bits(geometry.smooth_mesh(v, f, adjacency=adj, **how)), bits(want))
    smooth = geometry.smooth_mesh(v, f, adjacency=adj)
    normals = geometry.vertex_normals(smooth, f, adjacency=adj)                    # one build serves both
    assert torch.equal(normals.cpu(), geometry.vertex_normals(smooth.cpu(), faces))


@gpu
def test_entry_validates():
    from arah_release_amd import hip
    verts, faces = mesh("sphere17")
    V = verts.shape[0]
    v, f = verts.to(DEV), faces.to(DEV).to(torch.int32)
    adj = hip.mesh_adjacency(f, V)
    for bad in (lambda: hip.mesh_smooth(verts, f, 1), lambda: hip.mesh_smooth(v, faces, 1), lambda: hip.mesh_smooth(v.double(), f, 1),
                lambda: hip.mesh_smooth(v, f, -1), lambda: hip.mesh_smooth(v, f, 1, lamb=2.0), lambda: hip.mesh_smooth(v, f, 1, mu=-2.0),
                lambda: hip.mesh_smooth(v, f, 1, method="cotan"), lambda: hip.mesh_smooth(v, f, 1, boundary="fixed"),
                lambda: hip.mesh_smooth(v, f, 1, adjacency=adj[:2]), lambda: hip.mesh_smooth(v, f, 1, adjacency=tuple(t.cpu() for t in adj))):
        with pytest.raises(ValueError):
            bad()
    lib = hip.load_library()
    BADARG = -1
    p = hip._ptr
    tmp, out = torch.empty_like(v), torch.full_like(v, 7.0)
    factors = (C.c_float * 2)(0.5, -0.53)

    def smooth(verts_p=p(v), n_verts=V, start=p(adj[2]), nbr=p(adj[3]), flags=p(adj[6]), n_steps=2, fac=factors, tmp_p=p(tmp), out_p=p(out)):
        return lib.arah_mesh_smooth(verts_p, C.c_int64(n_verts), start, nbr, flags, C.c_int32(n_steps), fac, C.c_int32(1), tmp_p, out_p,
                                    hip._stream(DEV))
    for key in ("verts_p", "start", "flags", "fac", "tmp_p", "out_p"):
        assert smooth(**{key: None}) == BADARG, key
    assert smooth(n_verts=-1) == BADARG and smooth(n_verts=2 ** 31) == BADARG and smooth(n_steps=-1) == BADARG
    assert smooth(fac=(C.c_float * 2)(0.5, float("nan"))) == BADARG and smooth(fac=(C.c_float * 2)(float("inf"), 0.5)) == BADARG
    torch.cuda.synchronize()
    assert (out == 7.0).all()                                                      # the refused calls launched nothing
    assert smooth() == 0
    want = hip.mesh_smooth(v, f, 1, adjacency=adj)
    assert np.array_equal(bits(out), bits(want))
    assert smooth(n_steps=1, tmp_p=None) == 0 and smooth(n_steps=0, tmp_p=None) == 0     # no second buffer needed
    assert np.array_equal(bits(out), bits(v))                                      # no step: a copy
    assert lib.arah_mesh_smooth(None, C.c_int64(0), p(adj[2]), None, None, C.c_int32(3), factors, C.c_int32(1), None, None, hip._stream(DEV)) == 0
    torch.cuda.synchronize()


# ---- GPU: the model's entries ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def subject(scene):
    dev = torch.device(DEV)
    model, _ = get_model("zju377_mono", dev)
    model.eval()
    return model, scene.make_inputs(32, 32, frame_idx=0, device=dev)


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        if torch.is_tensor(a[k]):
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


@gpu
def test_posed_mesh_smooth_is_smooth_mesh_of_the_posed_mesh(subject):
    from arah_release_amd import geometry
    model, inputs = subject
    with torch.no_grad():
        plain = model.posed_mesh(inputs, n_side=65, indexed=True)
        _same(plain, model.posed_mesh(inputs, n_side=65, indexed=True, smooth=None))
        assert plain["n_tris"] > 1000
        smooth = model.posed_mesh(inputs, n_side=65, indexed=True, smooth=3)
        assert set(smooth) == set(plain)
        expect = geometry.smooth_mesh(plain["verts"], plain["faces"], iterations=3)
        assert torch.equal(smooth["verts"], expect) and not torch.equal(expect, plain["verts"])
        _same({k: v for k, v in smooth.items() if k != "verts"}, {k: v for k, v in plain.items() if k != "verts"})
        span = float((plain["verts"].max(0).values - plain["verts"].min(0).values).max())
        how = {"iterations": 2, "method": "laplacian", "lamb": 0.4, "boundary": "free"}
        front = model.posed_mesh(inputs, n_side=65, indexed=True, clean="largest", simplify=span / 24)
        both = model.posed_mesh(inputs, n_side=65, indexed=True, clean="largest", simplify=span / 24, smooth=how)
        assert 0 < front["n_tris"] < plain["n_tris"]
        assert torch.equal(both["verts"], geometry.smooth_mesh(front["verts"], front["faces"], **how))       # after clean and simplify
        _same({k: v for k, v in both.items() if k != "verts"}, {k: v for k, v in front.items() if k != "verts"})
    with pytest.raises(ValueError):
        model.posed_mesh(inputs, n_side=65, smooth=3)                             # a soup has no shared vertices
    with pytest.raises(ValueError):
        model.posed_mesh(inputs, n_side=65, indexed=True, smooth={"iterations": 1, "lamb": 3.0})


@gpu
def test_canonical_mesh_smooths_before_its_attributes(subject):
    from arah_release_amd import geometry, hip
    model, inputs = subject
    with torch.no_grad():
        bare = model.canonical_mesh(inputs, n_side=65)
        _same(bare, model.canonical_mesh(inputs, n_side=65, smooth=None))
        names = ("normal", "vertex_normal")
        plain = model.canonical_mesh(inputs, n_side=65, attributes=names)
        _same(plain, model.canonical_mesh(inputs, n_side=65, attributes=names, smooth=None))
        assert torch.equal(plain["vertex_normal"], geometry.vertex_normals(plain["verts"], plain["faces"]))
        got = model.canonical_mesh(inputs, n_side=65, attributes=("vertex_normal",), smooth=2)
        assert set(got) == set(bare) | {"vertex_normal"} and torch.equal(got["faces"], bare["faces"])
        assert torch.equal(got["verts"], geometry.smooth_mesh(bare["verts"], bare["faces"], iterations=2))
        assert torch.equal(got["vertex_normal"], geometry.vertex_normals(got["verts"], got["faces"]))
        assert got["vertex_normal"].shape == (got["n_verts"], 3) and not torch.equal(got["vertex_normal"], plain["vertex_normal"])
        # the mesh's own normals and the SDF's agree in direction up to the mesh's orientation (towards decreasing values: inwards)
        cos = (plain["vertex_normal"] * plain["normal"]).sum(1)
        assert (cos < 0).float().mean().item() > 0.9
        # the SDF's normal is taken AT the smoothed positions
        both = model.canonical_mesh(inputs, n_side=65, attributes=names, clean="largest", simplify=4.0 / 64, smooth=2)
        frame, ws = model._posed_frame(inputs, "test")
        grad = hip.sdf_eval(frame, ws, both["verts"].contiguous(), want_grad=True)[2]
        assert torch.equal(both["normal"], grad / grad.norm(dim=1, keepdim=True).clamp_min(1e-20))
        assert torch.equal(both["vertex_normal"], geometry.vertex_normals(both["verts"], both["faces"]))
    with pytest.raises(ValueError):
        model.canonical_mesh(inputs, n_side=65, smooth={"mu": 0.5})
