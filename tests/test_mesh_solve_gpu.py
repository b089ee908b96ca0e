"""The kernels of csrc/meshsolve.hpp (arah_mesh_solve_begin, arah_mesh_solve_steps) against their tensor specification
meshing.laplacian_solve: bit for bit in x, iters, status, rr, r0, counts and classes; launch geometry up to a second level of the
finishing tree; batching; empty inputs; the C entries on buffers of the test's own; the public functions on device tensors against
the same calls on the host; the model's smooth={"method": "implicit"}."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_mesh_laplacian import mesh, same_bits, spec
from test_mesh_solve import OUTPUTS, implicit_system, mean_edge, pins_of, same_outputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x5A
PAD = 5
MAX_ITER = 1000
# bicone40: two vertices with 40 neighbours; jgrid33_1: 1 089 vertices, 4 blocks and a short fifth; sphere33, f10: a dozen blocks
# and hundreds of steps; nan_vertex: a vertex that is not live; open_sphere: isolated vertices without area; fin: a non-manifold edge
DEVICE = ("tetrahedron", "kite", "sheet", "nan_vertex", "open_sphere", "bicone40", "fin", "jgrid33_1", "ico3", "sphere33", "f10")
_DEVICE_OP = {}


def device_operator(name, faces_dtype=torch.int32, cached=True):
    """weight, area and the adjacency of a named mesh, built on the device; the int32 one is computed once and shared."""
    from arah_release_amd import hip
    if not cached or name not in _DEVICE_OP:
        verts, faces = mesh(name)
        dv, df = verts.to(DEV), faces.to(DEV).to(faces_dtype)
        adj = hip.mesh_adjacency(df, dv.shape[0])
        weight, _, area, _, _ = hip.mesh_cotangent(dv, df, "mixed", adj)
        if not cached:
            return weight, area, adj
        _DEVICE_OP[name] = (weight, area, adj)
    return _DEVICE_OP[name]


def solve_both(name, rhs, x0, pinned, mc, sc, what, operator=None, **kw):
    """hip.laplacian_solve on the device against meshing.laplacian_solve on the host: every output, bit for bit.  -> the host's."""
    from arah_release_amd import hip, meshing
    adj, lap, _ = spec(name)
    weight, area, dadj = operator or device_operator(name)
    max_iter = kw.pop("max_iter", MAX_ITER)
    want = meshing.laplacian_solve(lap[0], lap[2], adj, rhs, x0, pinned=pinned, mass_coef=mc, stiff_coef=sc, max_iter=max_iter)
    got = hip.laplacian_solve(weight, area, dadj, rhs.to(DEV), x0.to(DEV), pinned=None if pinned is None else pinned.to(DEV), mass_coef=mc,
                              stiff_coef=sc, max_iter=max_iter, **kw)
    assert all(t.is_cuda for t in got)
    same_outputs(got, want, what)
    return want


@pytest.mark.parametrize("name", DEVICE)
def test_kernels_are_the_specification(name):
    verts, _ = mesh(name)
    V = verts.shape[0]
    pinned = pins_of(name)
    steps = []
    for factor in (1.0, 100.0):
        mc, sc, rhs, x0 = implicit_system(name, factor)
        for pins in (pinned, None):
            want = solve_both(name, rhs, x0, pins, mc, sc, (name, factor, pins is not None))
            steps += want[1].tolist()
            assert bool(((want[2] == 1) | (want[1] == MAX_ITER)).all())
    p = x0
    dirichlet = (torch.zeros_like(p), torch.where(pinned[:, None], p, torch.zeros_like(p)), pinned, 0.0, 1.0)
    want = solve_both(name, *dirichlet, (name, "dirichlet"))
    steps += want[1].tolist()
    # once more from int64 faces and an adjacency built anew: the order of arrival does not show
    solve_both(name, *dirichlet, (name, "dirichlet", "again"), operator=device_operator(name, torch.int64, cached=False))
    # 1, 7 and 32 columns of seeded normals with a row that is not finite, against zeros
    rs = np.random.RandomState(11)
    sc = mean_edge(name) ** 2
    for n_ch in (1, 7, 32):
        rhs = torch.from_numpy(rs.standard_normal((V, n_ch)))
        rhs[3 % V, n_ch // 2] = float("nan")
        want = solve_both(name, rhs, torch.zeros_like(rhs), None, 1.0, sc, (name, "columns", n_ch))
        assert int(want[5][3]) == 1 and bool(torch.isfinite(want[0]).all())
    print("%s: %d vertices, %d to %d steps" % (name, V, min(steps), max(steps)))


def strip(n_verts):
    """A fan strip with exactly n_verts vertices, as tests/test_mesh_laplacian_gpu.py builds it."""
    g = torch.Generator().manual_seed(n_verts)
    verts = torch.rand(n_verts, 3, generator=g)
    i = torch.arange(n_verts - 2)
    faces = torch.stack([i, i + 1, i + 2], 1)
    faces[1::2] = faces[1::2].flip(1)
    return verts, faces


@pytest.mark.parametrize("n_verts", [63, 64, 65, 255, 256, 257, 511, 512, 513, 257 * 256 + 1])
def test_launch_geometry(n_verts):
    """The last lane, the last wave, one and two blocks' sums, and with 258 blocks a second chunk of the finishing tree."""
    from arah_release_amd import hip, meshing
    verts, faces = strip(n_verts)
    adj = meshing.mesh_adjacency(faces, n_verts)
    lap = meshing.mesh_cotangent(verts, faces, "mixed", adj)
    p = verts.double()
    rhs = lap[2][:, None] * p
    want = meshing.laplacian_solve(lap[0], lap[2], adj, rhs, p, mass_coef=1.0, stiff_coef=0.05, max_iter=8)
    dv, df = verts.to(DEV), faces.to(DEV)
    dadj = hip.mesh_adjacency(df, n_verts)
    weight, _, area, _, _ = hip.mesh_cotangent(dv, df, "mixed", dadj)
    got = hip.laplacian_solve(weight, area, dadj, rhs.to(DEV), p.to(DEV), mass_coef=1.0, stiff_coef=0.05, max_iter=8)
    same_outputs(got, want, (n_verts,))
    assert want[2].tolist() == [0, 0, 0] and want[1].tolist() == [8, 8, 8] and int(want[5][0]) > n_verts // 2


def test_batches_do_not_show():
    from arah_release_amd import hip
    # ico3 stops after 15 steps: inside the first batch of 32, inside the fourth batch of 4, at the end of a batch of 5, and under a
    # look after every step
    name = "ico3"
    mc, sc, rhs, x0 = implicit_system(name, 1.0)
    want = solve_both(name, rhs, x0, None, mc, sc, (name, 32), check_every=32)
    assert want[2].tolist() == [1, 1, 1] and 0 < max(want[1].tolist()) < 32 and max(want[1].tolist()) % 4
    for every in (1, 4, 5):
        solve_both(name, rhs, x0, None, mc, sc, (name, every), check_every=every)
    # a zero column stops at the start and the other two after different numbers of steps, while max_iter cuts a batch short
    name = "jgrid33_1"
    mc, sc, rhs, x0 = implicit_system(name, 10.0)
    want = solve_both(name, rhs, x0, pins_of(name), mc, sc, (name, 32))
    assert int(want[1][2]) == 0 and int(want[1][0]) != int(want[1][1]) and want[2].tolist() == [1, 1, 1]
    for every, max_iter in ((1, MAX_ITER), (5, MAX_ITER), (7, 20), (32, 33)):
        solve_both(name, rhs, x0, pins_of(name), mc, sc, (name, every, max_iter), check_every=every, max_iter=max_iter)
    with pytest.raises(ValueError):
        hip.laplacian_solve(*device_operator(name), rhs.to(DEV), x0.to(DEV), check_every=0)


def test_empty_inputs():
    from arah_release_amd import hip, meshing
    verts, faces = mesh("octahedron")
    for v, f in ((verts[:0], faces[:0]), (verts, faces[:0])):
        V = v.shape[0]
        adj, dadj = meshing.mesh_adjacency(f, V), hip.mesh_adjacency(f.to(DEV), V)
        lap = meshing.mesh_cotangent(v, f, "mixed", adj)
        dlap = hip.mesh_cotangent(v.to(DEV), f.to(DEV), "mixed", dadj)
        rhs = v.double() + 1.0
        for mc in (0.0, 1.0):
            want = meshing.laplacian_solve(lap[0], lap[2], adj, rhs, rhs, mass_coef=mc)
            got = hip.laplacian_solve(dlap[0], dlap[2], dadj, rhs.to(DEV), rhs.to(DEV), mass_coef=mc)
            same_outputs(got, want, (V, mc))
            assert want[2].tolist() == [1, 1, 1] and want[1].tolist() == [0, 0, 0] and int(want[5][0]) == 0


def test_entries_write_their_arrays_and_nothing_else():
    from arah_release_amd import hip, meshing
    name = "open_sphere"
    adj, lap, _ = spec(name)
    weight, area, dadj = device_operator(name)
    mc, sc, rhs, x0 = implicit_system(name, 10.0)
    pinned = pins_of(name)
    V, n_ch, F = rhs.shape[0], rhs.shape[1], dadj[3].shape[0] // 6
    drhs, dx0, dpin = rhs.to(DEV), x0.to(DEV), pinned.to(DEV).to(torch.uint8)
    lib = hip.load_library()
    p, i64, i32, f64 = hip._ptr, C.c_int64, C.c_int32, C.c_double
    need = int(lib.arah_mesh_solve_scratch_bytes(V, n_ch))
    sizes = (V * n_ch * 8, n_ch * 4, n_ch * 4, n_ch * 8, n_ch * 8, 8 * 4, V, need)    # x, iters, status, rr, r0, counts, classes, scratch
    kinds = (torch.float64, torch.int32, torch.int32, torch.float64, torch.float64, torch.int32, torch.uint8)

    def buf(nbytes):
        return torch.full((nbytes + PAD,), SENTINEL, dtype=torch.uint8, device=DEV)

    def untouched(bufs):
        return all(bool((b == SENTINEL).all()) for b in bufs)

    def tails(bufs):
        return all(bool((b[n:] == SENTINEL).all()) for b, n in zip(bufs, sizes))

    def outputs(bufs):
        out = [b[:n].view(k) for b, n, k in zip(bufs, sizes, kinds)]
        return [out[0].reshape(V, n_ch)] + out[1:]

    def begin(bufs, n_ch_=n_ch, mc_=mc, sc_=sc, tol=1e-10, nbytes=need):
        rc = lib.arah_mesh_solve_begin(p(weight), p(area), p(dadj[2]), p(dadj[3]), i64(V), i64(F), p(drhs), p(dx0), p(dpin), i32(n_ch_),
                                       f64(mc_), f64(sc_), f64(tol), *[p(b) for b in bufs[:7]], p(bufs[7]), C.c_size_t(nbytes), hip._stream())
        torch.cuda.synchronize()
        return rc

    def steps(bufs, n, n_ch_=n_ch, sc_=sc, nbytes=need):
        rc = lib.arah_mesh_solve_steps(p(weight), p(area), p(dadj[2]), p(dadj[3]), i64(V), i64(F), i32(n_ch_), f64(mc), f64(sc_), i32(n),
                                       *[p(b) for b in bufs[:5]], p(bufs[7]), C.c_size_t(nbytes), hip._stream())
        torch.cuda.synchronize()
        return rc

    with hip._on_device(torch.device(DEV)):
        for bad, rc_want in (({"n_ch_": 0}, -1), ({"n_ch_": 33}, -1), ({"mc_": -1.0}, -1), ({"sc_": 0.0}, -1), ({"tol": float("nan")}, -1),
                             ({"nbytes": need - 1}, -3)):
            bufs = [buf(n) for n in sizes]
            assert begin(bufs, **bad) == rc_want and untouched(bufs), bad            # the refused calls launch nothing
        bufs = [buf(n) for n in sizes]
        assert begin(bufs) == 0 and tails(bufs)
        want = meshing.laplacian_solve(lap[0], lap[2], adj, rhs, x0, pinned=pinned, mass_coef=mc, stiff_coef=sc, max_iter=0)
        same_outputs(outputs(bufs), want, ("raw begin",))
        before = [b.clone() for b in bufs]
        for bad, rc_want in (({"n": -1}, -1), ({"n_ch_": 33}, -1), ({"sc_": -1.0}, -1), ({"nbytes": need - 1}, -3)):
            assert steps(bufs, **dict({"n": 2}, **bad)) == rc_want, bad
            assert all(torch.equal(a, b) for a, b in zip(bufs, before)), bad
        assert steps(bufs, 3) == 0 and steps(bufs, 0) == 0 and steps(bufs, 2) == 0 and tails(bufs)
        want = meshing.laplacian_solve(lap[0], lap[2], adj, rhs, x0, pinned=pinned, mass_coef=mc, stiff_coef=sc, max_iter=5)
        same_outputs(outputs(bufs), want, ("raw steps",))
        assert want[1].tolist() == [5, 5, 5]


@pytest.mark.parametrize("name", ["open_sphere", "jgrid33_1", "f10"])
def test_public_functions_on_the_device_are_the_hosts(name):
    from arah_release_amd import geometry
    verts, faces = mesh(name)
    dv, df = verts.to(DEV), faces.to(DEV)
    ref, res = geometry.mesh_laplacian(verts, faces), geometry.mesh_laplacian(dv, df)
    t = 4.0 * mean_edge(name) ** 2
    pinned = pins_of(name)
    rhs = ref["area"][:, None] * verts.double()
    # the start is half the positions: on the planar grid the positions themselves solve the system to rounding, r0 would be
    # rounding noise and no residual could be small against it
    a = geometry.solve_laplacian(ref, rhs, 1.0, t, pinned=pinned, x0=0.5 * verts)
    b = geometry.solve_laplacian(res, rhs.to(DEV), 1.0, t, pinned=pinned.to(DEV), x0=0.5 * dv, check_every=8)
    assert b["x"].is_cuda and a["converged"] and {k: a[k] for k in ("iterations", "status", "converged", "residual", "report")} == \
        {k: b[k] for k in ("iterations", "status", "converged", "residual", "report")}
    same_bits(b["x"].cpu(), a["x"], (name, "solve"))
    assert max(b["true_residual"]) <= 1e-9 and np.allclose(a["true_residual"], b["true_residual"], rtol=1e-6, atol=1e-14)
    one = geometry.solve_laplacian(res, rhs[:, 1].float().to(DEV), 1.0, t)
    assert one["x"].shape == (verts.shape[0],) and one["status"] == "converged" and isinstance(one["iterations"], int)
    values = torch.stack([verts[:, 0].double() ** 2, verts[:, 1].double() - 1.0], 1)
    a = geometry.harmonic_extend(verts, faces, pinned, values)
    b = geometry.harmonic_extend(dv, df, pinned.to(DEV), values.to(DEV), laplacian=res)
    assert a["converged"] and a["iterations"] == b["iterations"] and a["report"] == b["report"]
    same_bits(b["values"].cpu(), a["values"], (name, "harmonic"))
    for how in ({"boundary": "pin"}, {"boundary": "free"}):
        got = geometry.smooth_mesh(dv, df, iterations=2, method="implicit", time=t, **how)
        assert got.is_cuda and got.dtype == torch.float32
        same_bits(got.cpu(), geometry.smooth_mesh(verts, faces, iterations=2, method="implicit", time=t, **how), (name, "implicit", how))


def test_model_surface(scene):
    from arah_release_amd import geometry
    from conftest import get_model
    model, _ = get_model("zju377_mono", torch.device(DEV))
    model.eval()
    inputs = scene.make_inputs(64, 64, frame_idx=0, device=torch.device(DEV))
    how = {"method": "implicit", "time": 4e-4, "iterations": 1}
    with torch.no_grad():
        plain = model.posed_mesh(inputs, n_side=49, indexed=True)
        smooth = model.posed_mesh(inputs, n_side=49, indexed=True, smooth=how)
        assert plain["verts"].shape[0] > 500 and torch.equal(smooth["faces"], plain["faces"])
        expect = geometry.smooth_mesh(plain["verts"], plain["faces"], **how)
        assert torch.equal(smooth["verts"], expect) and not torch.equal(expect, plain["verts"])
        same_bits(expect.cpu(), geometry.smooth_mesh(plain["verts"].cpu(), plain["faces"].cpu(), **how), "the host's")
        canon = model.canonical_mesh(inputs, n_side=49, smooth=how)
        assert torch.equal(canon["verts"], geometry.smooth_mesh(model.canonical_mesh(inputs, n_side=49)["verts"], canon["faces"], **how))
    with pytest.raises(ValueError, match="time"):
        model.posed_mesh(inputs, n_side=49, indexed=True, smooth={"method": "implicit"})
