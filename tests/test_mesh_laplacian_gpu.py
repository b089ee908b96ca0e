"""The kernels of csrc/meshlaplace.hpp (arah_mesh_cotangent, arah_mesh_laplacian_apply, arah_mesh_curvature,
arah_mesh_smooth_cotangent) against their tensor specifications in meshing.py: bit for bit in every array and counter, except
angle_sum -- and through it gaussian, k1 and k2 -- by the atan2 allowance; launch geometry; empty inputs; the C entries on buffers
of the test's own; the public functions on device tensors against the same calls on the host; the model's curvature attributes."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_mesh_laplacian import ATAN2_TERM, HOST, MASSES, bits, mesh, same_bits, spec

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x5A
PAD = 5
# jgrid33_1: 6 272 = 98 x 64 neighbour entries, whole waves; sphere33 and f10: several workgroups per launch; bicone40: two vertices
# with 40 faces, past kMaShort = 32, so k_ml_cot_long has work
DEVICE = HOST + ("fin", "jgrid33_1", "sphere33", "f10")


def device_mesh(name, faces_dtype=torch.int32):
    verts, faces = mesh(name)
    return verts.to(DEV), faces.to(DEV).to(faces_dtype)


def angle_allowance(adj):
    """The atan2 term for every face of the vertex."""
    return (adj[0][1:] - adj[0][:-1]).double() * ATAN2_TERM


def check_operator(got, want, adj, what):
    """weight, diag, area, counts bit for bit; angle_sum within the allowance.  -> the largest difference of angle_sum."""
    for i, key in ((0, "weight"), (1, "diag"), (2, "area"), (4, "counts")):
        same_bits(got[i].cpu(), want[i], what + (key,))
    off = (got[3].cpu() - want[3]).abs()
    assert bool((off <= angle_allowance(adj)).all()), what + ("angle_sum", float(off.max()))
    return float(off.max()) if off.numel() else 0.0


def check_curvature(got, want, lap, adj, what):
    """mean, mean_abs, mean_normal, valid, counts bit for bit -- they do not see angle_sum; gaussian within the angle's allowance
    over the area; k1, k2 within what that moves the root by."""
    g, w = got[0].cpu(), want[0]
    same_bits(g[:, :2], w[:, :2], what + ("mean, mean_abs",))
    same_bits(got[1].cpu(), want[1], what + ("mean_normal",))
    same_bits(got[2].cpu(), want[2], what + ("valid",))
    same_bits(got[3].cpu(), want[3], what + ("counts",))
    ok = want[2].bool()
    allow = angle_allowance(adj)[ok] / lap[2][ok]
    off = (g[ok, 2] - w[ok, 2]).abs()
    assert bool((off <= allow).all()) and bool(torch.isnan(g[~ok]).all()), what + ("gaussian",)
    # r = sqrt(max(mean^2 - gaussian, 0)): |sqrt(a) - sqrt(b)| <= sqrt(|a - b|)
    root = (g[ok, 3:] - w[ok, 3:]).abs().max(1).values if ok.any() else off
    assert bool((root <= allow.sqrt() + allow).all()), what + ("k1, k2",)
    return float(off.max()) if off.numel() else 0.0


@pytest.mark.parametrize("name", DEVICE)
def test_kernels_are_the_specification(name):
    from arah_release_amd import hip, meshing
    verts, faces = mesh(name)
    worst = [0.0, 0.0]
    for mass in MASSES:
        adj, lap, curv = spec(name, mass)
        dv, df = device_mesh(name)
        dadj = hip.mesh_adjacency(df, dv.shape[0])
        first = hip.mesh_cotangent(dv, df, mass, dadj)
        worst[0] = max(worst[0], check_operator(first, lap, adj, (name, mass)))
        # again, from faces of another integer type and an adjacency built anew: the order of arrival does not show
        dv64, df64 = device_mesh(name, torch.int64)
        again = hip.mesh_cotangent(dv64, df64, mass)
        for a, b in zip(again, first):
            same_bits(a.cpu(), b.cpu(), (name, mass, "again"))
        # curvature, given the device's own angle_sum
        want = meshing.mesh_curvature(verts, faces, mass, adj, (lap[0], lap[1], lap[2], first[3].cpu()))
        got = hip.mesh_curvature(dv, df, mass, dadj, first)
        for g, w, key in zip(got, want, ("curv", "mean_normal", "valid", "counts")):
            same_bits(g.cpu(), w, (name, mass, key, "own angles"))
        worst[1] = max(worst[1], check_curvature(hip.mesh_curvature(dv64, df64, mass), curv, lap, adj, (name, mass)))
    adj, lap, _ = spec(name)
    x = torch.from_numpy(np.random.RandomState(7).standard_normal((verts.shape[0], 32)))
    x[3 % verts.shape[0], 5] = float("nan")
    for t in (x, x[:, :1].float().contiguous(), x[:, :7].float().contiguous(), verts):
        same_bits(hip.laplacian_apply(first[0], dadj, t.to(DEV)).cpu(), meshing.laplacian_apply(lap[0], adj, t), (name, "apply", t.shape, t.dtype))
    for how in ({"method": "taubin"}, {"method": "taubin", "boundary": "free", "lamb": 0.4, "mu": -0.42}):
        want = meshing.mesh_smooth(verts, faces, 3, weights="cotangent", adjacency=adj, **how)
        same_bits(hip.mesh_smooth(dv, df, 3, weights="cotangent", adjacency=dadj, **how).cpu(), want, (name, "smooth", how))
        same_bits(hip.mesh_smooth(dv64, df64, 3, weights="cotangent", **how).cpu(), want, (name, "smooth", how, "again"))
    same_bits(hip.mesh_smooth(dv, df, 1, method="laplacian", weights="cotangent").cpu(),
              meshing.mesh_smooth(verts, faces, 1, method="laplacian", weights="cotangent"), (name, "one step"))
    print("%s: angle_sum differs from the specification's by at most %.3g, gaussian by at most %.3g" % (name, worst[0], worst[1]))


@pytest.mark.parametrize("n_verts", [63, 64, 65, 255, 256, 257])
def test_launch_geometry(n_verts):
    """A fan strip with exactly n_verts vertices: the last lanes of the last wave and workgroup."""
    from arah_release_amd import hip, meshing
    g = torch.Generator().manual_seed(n_verts)
    verts = torch.rand(n_verts, 3, generator=g)
    i = torch.arange(n_verts - 2)
    faces = torch.stack([i, i + 1, i + 2], 1)
    faces[1::2] = faces[1::2].flip(1)
    adj = meshing.mesh_adjacency(faces, n_verts)
    lap = meshing.mesh_cotangent(verts, faces, "mixed", adj)
    dv, df = verts.to(DEV), faces.to(DEV)
    got = hip.mesh_cotangent(dv, df)
    check_operator(got, lap, adj, (n_verts,))
    want = meshing.mesh_curvature(verts, faces, "mixed", adj, (lap[0], lap[1], lap[2], got[3].cpu()))
    for g_, w, key in zip(hip.mesh_curvature(dv, df, laplacian=got), want, ("curv", "mean_normal", "valid", "counts")):
        same_bits(g_.cpu(), w, (n_verts, key))
    same_bits(hip.laplacian_apply(got[0], hip.mesh_adjacency(df, n_verts), dv).cpu(), meshing.laplacian_apply(lap[0], adj, verts), (n_verts, "apply"))
    same_bits(hip.mesh_smooth(dv, df, 2, weights="cotangent", boundary="free").cpu(),
              meshing.mesh_smooth(verts, faces, 2, weights="cotangent", boundary="free"), (n_verts, "smooth"))


def test_empty_meshes_write_their_counts():
    from arah_release_amd import hip, meshing
    verts, faces = mesh("octahedron")
    dv, df = verts.to(DEV), faces.to(DEV)
    for v, f, hv, hf in ((dv[:0], df[:0], verts[:0], faces[:0]), (dv, df[:0], verts, faces[:0]), (dv[:0], df, verts[:0], faces)):
        got, want = hip.mesh_cotangent(v, f), meshing.mesh_cotangent(hv, hf)
        for g, w in zip(got, want):
            same_bits(g.cpu(), w, (v.shape, f.shape))
        for g, w in zip(hip.mesh_curvature(v, f), meshing.mesh_curvature(hv, hf)):
            same_bits(g.cpu(), w, (v.shape, f.shape, "curvature"))
        adj, hadj = hip.mesh_adjacency(f, v.shape[0]), meshing.mesh_adjacency(hf, hv.shape[0])
        same_bits(hip.laplacian_apply(got[0], adj, v).cpu(), meshing.laplacian_apply(want[0], hadj, hv), (v.shape, f.shape, "apply"))
        same_bits(hip.mesh_smooth(v, f, 2, weights="cotangent").cpu(), hv, (v.shape, f.shape, "smooth"))


def test_entries_write_their_arrays_and_nothing_else():
    from arah_release_amd import hip, meshing
    name = "bad_ids"
    verts, faces = mesh(name)
    adj, lap, curv = spec(name)
    dv, f32 = verts.to(DEV), faces.to(DEV).to(torch.int32).contiguous()
    lib = hip.load_library()
    V, F = dv.shape[0], f32.shape[0]
    dadj = hip.mesh_adjacency(f32, V)
    normal_sum = hip.vertex_normals(dv, f32, dadj)[0]
    p, i64, i32 = hip._ptr, C.c_int64, C.c_int32

    def buf(nbytes):
        return torch.full((nbytes + PAD,), SENTINEL, dtype=torch.uint8, device=DEV)

    def untouched(bufs):
        return all(bool((b == SENTINEL).all()) for b in bufs)

    def tails(bufs, sizes):
        return all(bool((b[n:] == SENTINEL).all()) for b, n in zip(bufs, sizes))

    with hip._on_device(dv.device):
        # the operator: weight, diag, area, angle_sum, counts
        sizes = (6 * F * 8, V * 8, V * 8, V * 8, 8 * 4)
        for mass, rc_want in ((2, -1), (-1, -1), (1, 0)):                         # the refused calls launch nothing
            bufs = [buf(n) for n in sizes]
            rc = lib.arah_mesh_cotangent(p(dv), i64(V), p(f32), i64(F), p(dadj[0]), p(dadj[1]), p(dadj[2]), p(dadj[3]), i32(mass),
                                         *[p(b) for b in bufs], hip._stream())
            torch.cuda.synchronize()
            assert rc == rc_want and (rc == 0 or untouched(bufs))
        assert tails(bufs, sizes)
        kinds = (torch.float64,) * 4 + (torch.int32,)
        op = [b[:n].view(k) for b, n, k in zip(bufs, sizes, kinds)]
        check_operator(op, lap, adj, ("raw entry",))
        assert counts_ok(lap)
        # apply: y (V, C)
        x = torch.from_numpy(np.random.RandomState(3).standard_normal((V, 32))).to(DEV)
        for n_ch, rc_want in ((0, -1), (33, -1), (32, 0)):
            y = buf(V * 32 * 8)
            rc = lib.arah_mesh_laplacian_apply(p(op[0]), p(dadj[2]), p(dadj[3]), i64(V), i64(F), p(x), i32(1), i32(n_ch), p(y), hip._stream())
            torch.cuda.synchronize()
            assert rc == rc_want and (rc == 0 or untouched([y]))
        assert tails([y], [V * 32 * 8])
        same_bits(y[:V * 32 * 8].view(torch.float64).reshape(V, 32).cpu(), meshing.laplacian_apply(lap[0], adj, x.cpu()), "raw apply")
        # curvature: curv, mean_normal, valid, counts
        sizes = (V * 5 * 8, V * 3 * 8, V, 4)
        bufs = [buf(n) for n in sizes]
        rc = lib.arah_mesh_curvature(p(dv), i64(V), i64(F), p(dadj[2]), p(dadj[3]), p(dadj[6]), p(op[0]), p(op[2]), p(op[3]), p(normal_sum),
                                     *[p(b) for b in bufs], hip._stream())
        torch.cuda.synchronize()
        assert rc == 0 and tails(bufs, sizes)
        want = meshing.mesh_curvature(verts, faces, "mixed", adj, (lap[0], lap[1], lap[2], op[3].cpu()))
        shapes, kinds = ((V, 5), (V, 3), (V,), (1,)), (torch.float64, torch.float64, torch.uint8, torch.int32)
        for b, n, k, s, w in zip(bufs, sizes, kinds, shapes, want):
            same_bits(b[:n].view(k).reshape(s).cpu(), w, "raw curvature")
        # smoothing, three Taubin iterations = six steps: tmp, verts_out, scratch
        need = int(lib.arah_mesh_smooth_cotangent_scratch_bytes(V, F))
        sizes = (V * 12, V * 12, need)
        for nbytes, rc_want in ((need - 1, -3), (need, 0)):
            bufs = [buf(n) for n in sizes]
            rc = lib.arah_mesh_smooth_cotangent(p(dv), i64(V), p(f32), i64(F), p(dadj[0]), p(dadj[1]), p(dadj[2]), p(dadj[3]), p(dadj[6]),
                                                i32(6), (C.c_float * 2)(0.5, -0.53), i32(1), p(bufs[0]), p(bufs[1]), p(bufs[2]),
                                                C.c_size_t(nbytes), hip._stream())
            torch.cuda.synchronize()
            assert rc == rc_want and (rc == 0 or untouched(bufs))
        assert tails(bufs, sizes)
        same_bits(bufs[1][:V * 12].view(torch.float32).reshape(V, 3).cpu(), meshing.mesh_smooth(verts, faces, 3, weights="cotangent"), "raw smooth")


def counts_ok(lap):
    c = lap[4].tolist()
    return c[0] > 0 and c[6] == c[7] == 0


@pytest.mark.parametrize("name", ["open_sphere", "three_faces", "f10"])
def test_public_functions_on_the_device_are_the_hosts(name):
    from arah_release_amd import geometry
    verts, faces = mesh(name)
    dv, df = verts.to(DEV), faces.to(DEV)
    ref, res = geometry.mesh_laplacian(verts, faces), geometry.mesh_laplacian(dv, df)
    assert res["weight"].is_cuda and res["report"] == ref["report"]
    adj = tuple(ref["adjacency"])
    check_operator([res[k] for k in ("weight", "diag", "area", "angle_sum")] + [torch.tensor(list(res["report"].values()) + [0, 0], dtype=torch.int32)],
                   [ref[k] for k in ("weight", "diag", "area", "angle_sum")] + [torch.tensor(list(ref["report"].values()) + [0, 0], dtype=torch.int32)],
                   adj, (name,))
    for kind in ("stiffness", "normalized"):
        dense, want = geometry.laplacian_matrix(res, kind).to_dense().cpu(), geometry.laplacian_matrix(ref, kind).to_dense()
        finite = torch.isfinite(want)
        assert torch.equal(torch.isfinite(dense), finite) and torch.equal(dense[finite], want[finite]), (name, kind)
    same_bits(geometry.apply_laplacian(res, dv[:, 1]).cpu(), geometry.apply_laplacian(ref, verts[:, 1]), (name, "apply"))
    for mass in MASSES:
        cref, cres = geometry.mesh_curvature(verts, faces, mass), geometry.mesh_curvature(dv, df, mass)
        assert cres["report"] == cref["report"] and cres["mean"].is_cuda
        ok = cref["valid"]
        assert torch.equal(cres["valid"].cpu(), ok)
        for key in ("mean", "mean_abs", "mean_normal", "area"):
            same_bits(cres[key].cpu(), cref[key], (name, mass, key))
        allow = angle_allowance(adj)[ok] / cref["area"][ok]
        assert bool(((cres["gaussian"].cpu() - cref["gaussian"])[ok].abs() <= allow).all())
        for key in ("k1", "k2"):
            assert bool(((cres[key].cpu() - cref[key])[ok].abs() <= allow.sqrt() + allow).all())
    how = {"iterations": 2, "weights": "cotangent", "lamb": 0.6, "mu": -0.62}
    same_bits(geometry.smooth_mesh(dv, df, **how).cpu(), geometry.smooth_mesh(verts, faces, **how), (name, "smooth"))


def test_model_surface(scene):
    from arah_release_amd import geometry
    from conftest import get_model
    model, _ = get_model("zju377_mono", torch.device(DEV))
    model.eval()
    inputs = scene.make_inputs(64, 64, frame_idx=0, device=torch.device(DEV))
    names = ("mean_curvature", "gaussian_curvature")
    with torch.no_grad():
        m = model.canonical_mesh(inputs, attributes=names, n_side=64)
        V = m["verts"].shape[0]
        curv = geometry.mesh_curvature(m["verts"], m["faces"])
        assert V > 100 and m["mean_curvature"].shape == (V, 1) and m["gaussian_curvature"].shape == (V, 1)
        same_bits(m["mean_curvature"][:, 0].cpu(), curv["mean"].cpu(), "mean")
        same_bits(m["gaussian_curvature"][:, 0].cpu(), curv["gaussian"].cpu(), "gaussian")
        # a body is mostly convex, and the level set's faces are clockwise seen from outside
        assert float((curv["mean"][curv["valid"]] < 0).double().mean()) > 0.6
        smoothed = model.canonical_mesh(inputs, n_side=64, smooth={"weights": "cotangent", "iterations": 2})
        assert torch.equal(smoothed["verts"], geometry.smooth_mesh(m["verts"], m["faces"], iterations=2, weights="cotangent"))
        img = model.render_mesh(inputs, attributes=("mean_curvature",), n_side=64, height=64, width=64)
        mask = img["mask"].bool()
        assert img["mean_curvature"].shape == (64, 64, 1) and bool(mask.any()) and bool(torch.isfinite(img["mean_curvature"][mask]).all())
        assert bool((img["mean_curvature"][mask] != 0).any())
