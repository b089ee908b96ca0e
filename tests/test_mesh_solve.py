"""Solving with the cotangent operator on the host: the tensor specification meshing.laplacian_solve against a numpy float64
restatement written with python loops (bit for bit), the inner product's tree, the per-column rules, the cases with a known
answer (implicit smoothing of spheres, harmonic extension of linear functions, planar grids), and the argument checks of
geometry.solve_laplacian / harmonic_extend / smooth_mesh(method="implicit").  Everything here runs on the host;
tests/test_mesh_solve_gpu.py holds the kernels of csrc/meshsolve.hpp to the specification."""
import os
import re

import numpy as np
import pytest
import torch

from test_mesh_laplacian import mesh, same_bits, spec

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("arah_mesh_solve_scratch_bytes", "arah_mesh_solve_begin", "arah_mesh_solve_steps")
NAMES = ("solved", "pinned", "not_live", "bad_rhs", "bad_area", "bad_diagonal")
HOST = ("octahedron", "sheet", "jgrid9_0", "nan_vertex", "fin")
OUTPUTS = ("x", "iters", "status", "rr", "r0", "counts", "classes")


def mean_edge(name):
    """The mean edge length h of a named mesh: the tests' times are multiples of h^2."""
    verts, faces = mesh(name)
    p = verts.double()[faces]
    finite = torch.isfinite(p).all(2).all(1)
    return float(torch.cat([(p[finite, i] - p[finite, (i + 1) % 3]).norm(dim=1) for i in range(3)]).mean())


def pins_of(name):
    """The vertices a test pins: those of boundary and non-manifold edges, and on a closed manifold mesh two of its vertices."""
    adj = spec(name)[0]
    pinned = (adj[6] & 3) != 0
    if not bool(pinned.any()):
        pinned[0] = pinned[pinned.shape[0] // 2] = True
    return pinned


def implicit_system(name, factor):
    """(mass_coef, stiff_coef, rhs, x0) of one implicit smoothing step with time = factor h^2 on a named mesh."""
    verts, _ = mesh(name)
    p = verts.double()
    return 1.0, factor * mean_edge(name) ** 2, spec(name)[1][2][:, None] * p, p


# ---- an independent restatement: plain loops over numpy float64 scalars ----------------------------------------------------------
def numpy_tree(x):
    """meshing.quadric_tree_sum of one segment, in place, as its docstring states it."""
    x, n = list(x), len(x)
    if n == 0:
        return np.float64(0.0)
    stride = 1
    while stride < n:
        for i in range(0, n, 2 * stride):
            if i + stride < n:
                x[i] = x[i] + x[i + stride]
        stride *= 2
    return x[0]


def numpy_solve(weight, area, adj, rhs, x0, pinned, mass_coef, stiff_coef, tol, max_iter):
    weight, area, rhs, x0 = weight.numpy(), area.numpy(), rhs.numpy(), x0.numpy()
    start, nbr = adj[2].numpy(), adj[3].numpy()
    V, C = rhs.shape
    mc, sc = np.float64(mass_coef), np.float64(stiff_coef)
    with np.errstate(all="ignore"):
        live = [bool(np.isfinite(x0[v]).all()) for v in range(V)]
        rows = [[(int(nbr[k]), weight[k]) for k in range(start[v], start[v + 1]) if np.isfinite(weight[k]) and live[nbr[k]]] for v in range(V)]
        a = [area[v] if mass_coef != 0 else np.float64(0.0) for v in range(V)]
        d, cls = np.zeros(V), np.zeros(V, dtype=np.uint8)
        for v in range(V):
            dS = np.float64(0.0)
            for _, w in rows[v]:
                dS = dS + w
            d[v] = mc * a[v] + sc * dS
            if pinned is not None and pinned[v]:
                cls[v] = 1
            elif not live[v]:
                cls[v] = 2
            elif not np.isfinite(rhs[v]).all():
                cls[v] = 3
            elif mass_coef != 0 and not (np.isfinite(a[v]) and a[v] > 0):
                cls[v] = 4
            elif not (np.isfinite(d[v]) and d[v] > 0):
                cls[v] = 5
        counts = np.array([int((cls == k).sum()) for k in range(6)] + [0, 0], dtype=np.int32)
        solved = [v for v in range(V) if cls[v] == 0]

        def op(y):
            out = np.zeros(V)
            for v in solved:
                acc = np.float64(0.0)
                for n, w in rows[v]:
                    acc = acc + w * (y[n] - y[v])
                out[v] = mc * (a[v] * y[v]) - sc * acc
            return out

        def dot(u, v):
            return numpy_tree([u[i] * v[i] for i in range(V)])

        x = x0.copy()
        iters, status, rr_out, r0_out = np.zeros(C, dtype=np.int32), np.zeros(C, dtype=np.int32), np.zeros(C), np.zeros(C)
        for c in range(C):
            r, z = np.zeros(V), np.zeros(V)
            q0 = op(x0[:, c])
            for v in solved:
                r[v] = rhs[v, c] - q0[v]
                z[v] = r[v] / d[v]
            p = z.copy()
            rz, rr = dot(r, z), dot(r, r)
            r0 = rr
            thr = (np.float64(tol) * np.float64(tol)) * r0
            st = 2 if not np.isfinite(r0) else 1 if rr <= thr else 0
            it = 0
            while st == 0 and it < max_iter:
                q = op(p)
                pq = dot(p, q)
                if not (np.isfinite(pq) and pq > 0):
                    st = 2
                    break
                alpha = rz / pq
                for v in solved:
                    x[v, c] = x[v, c] + alpha * p[v]
                    r[v] = r[v] - alpha * q[v]
                    z[v] = r[v] / d[v]
                rz_new, rr = dot(r, z), dot(r, r)
                it += 1
                if rr <= thr:
                    st = 1
                    break
                beta = rz_new / rz
                for v in solved:
                    p[v] = z[v] + beta * p[v]
                rz = rz_new
            iters[c], status[c], rr_out[c], r0_out[c] = it, st, rr, r0
    return x, iters, status, rr_out, r0_out, counts, cls


def same_outputs(got, want, what):
    for key, g, w in zip(OUTPUTS, got, want):
        same_bits(g.cpu() if torch.is_tensor(g) else g, w, what + (key,))


# ---- 1: the specification is the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_iter", [0, 3, 10000])
@pytest.mark.parametrize("pins", [False, True])
@pytest.mark.parametrize("name", HOST)
def test_specification_is_the_restatement(name, pins, max_iter):
    from arah_release_amd import meshing
    adj, lap, _ = spec(name)
    pinned = pins_of(name) if pins else None
    systems = [implicit_system(name, 1.0), implicit_system(name, 100.0)]
    if pins:                                                                      # a Dirichlet problem needs its pins
        _, _, _, p = implicit_system(name, 1.0)
        systems.append((0.0, 1.0, torch.zeros_like(p), torch.where(pinned[:, None], p, torch.zeros_like(p))))
    for mc, sc, rhs, x0 in systems:
        got = meshing.laplacian_solve(lap[0], lap[2], adj, rhs, x0, pinned=pinned, mass_coef=mc, stiff_coef=sc, max_iter=max_iter)
        want = numpy_solve(lap[0], lap[2], adj, rhs, x0, None if pinned is None else pinned.numpy(), mc, sc, 1e-10, max_iter)
        same_outputs(got, want, (name, pins, max_iter, mc, sc))
        assert got[1].dtype == torch.int32 and got[5].dtype == torch.int32 and got[6].dtype == torch.uint8
        assert int(got[5][:6].sum()) == rhs.shape[0] and bool((got[1] <= max_iter).all())
        if max_iter == 10000:
            assert got[2].tolist() == [1, 1, 1], (name, pins, mc, sc, got[2].tolist())
        held = got[6] != 0
        same_bits(got[0][held], x0[held], (name, "held rows are x0"))
        if name == "nan_vertex" and mc != 0.0:                                    # x0 holds the positions: vertex 11 is not live
            assert int(got[6][11]) == (1 if pins and bool(pinned[11]) else 2) and bool(torch.isfinite(got[0][got[6] == 0]).all())


# ---- 2: the inner product ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_inner_product_is_the_tree_of_one_segment(n):
    from arah_release_amd import meshing
    rs = np.random.RandomState(n)
    u, v = torch.from_numpy(rs.standard_normal((n, 2))), torch.from_numpy(rs.standard_normal((n, 2)) * 1e3)
    got = meshing.solve_dot(u, v)
    zero = torch.zeros(1, dtype=torch.int64)
    same_bits(got, meshing.quadric_tree_sum(u * v, zero, torch.tensor([n]))[0], (n, "one segment"))
    # aligned blocks of 256, then the blocks' sums: what the workgroups and the finishing workgroup take
    starts = torch.arange(0, n, 256)
    sums = meshing.quadric_tree_sum(u * v, starts, (n - starts).clamp(max=256))
    same_bits(got, meshing.quadric_tree_sum(sums, zero, torch.tensor([sums.shape[0]]))[0], (n, "blocks"))
    same_bits(got[0], numpy_tree((u[:, 0] * v[:, 0]).numpy()), (n, "loops"))
    assert meshing.solve_dot(u[:0], v[:0]).tolist() == [0.0, 0.0]


# ---- 3: the rules per column -----------------------------------------------------------------------------------------------------------
def test_a_zero_column_stops_at_once_and_the_others_do_not_see_it():
    from arah_release_amd import meshing
    name = "jgrid33_1"                                                           # planar: the third coordinate is 0 everywhere
    adj, lap, _ = spec(name)
    mc, sc, rhs, x0 = implicit_system(name, 10.0)
    assert not bool(x0[:, 2].any())
    pinned = pins_of(name)
    got = meshing.laplacian_solve(lap[0], lap[2], adj, rhs, x0, pinned=pinned, mass_coef=mc, stiff_coef=sc)
    print("jgrid33_1 at t = 10 h^2: iterations %s" % got[1].tolist())
    assert got[2].tolist() == [1, 1, 1] and int(got[1][2]) == 0 and min(got[1][:2].tolist()) > 10
    assert float(got[4][2]) == 0.0 and bool(torch.isfinite(got[0]).all())
    two = meshing.laplacian_solve(lap[0], lap[2], adj, rhs[:, :2].contiguous(), x0[:, :2].contiguous(), pinned=pinned, mass_coef=mc,
                                  stiff_coef=sc)
    for i in range(5):
        same_bits(got[i][..., :2], two[i], ("two columns alone", OUTPUTS[i]))
    # a column that stops early does not hold the others back, and is not touched by their steps
    few = meshing.laplacian_solve(lap[0], lap[2], adj, rhs, x0, pinned=pinned, mass_coef=mc, stiff_coef=sc, max_iter=5)
    assert few[1].tolist() == [5, 5, 0] and few[2].tolist() == [0, 0, 1]
    same_bits(few[0][:, 2], x0[:, 2], "the stopped column")


def entry_of(adj, v, n):
    start, nbr = adj[2].long(), adj[3].long()
    return int(start[v]) + nbr[start[v]:start[v + 1]].tolist().index(n)


def test_indefinite_weights_break_down_and_unusable_ones_are_left_out():
    from arah_release_amd import meshing
    name = "jgrid9_0"
    adj, lap, _ = spec(name)
    V = lap[2].shape[0]
    pinned = pins_of(name)
    v = 40
    n = int(adj[3][int(adj[2][v])])
    assert not bool(pinned[v]) and not bool(pinned[n])
    rhs = torch.from_numpy(np.random.RandomState(1).standard_normal((V, 3)))
    rhs[:, 2] = 0.0
    x0 = torch.zeros_like(rhs)
    # an edge weight of -1.5 leaves both diagonals positive (the other weights sum to about 2.9) and the 2 x 2 block of the edge
    # indefinite: p.Ap <= 0 shows within a few steps, the column stops where it was, and the zero column is not touched
    w = lap[0].clone()
    w[entry_of(adj, v, n)] = w[entry_of(adj, n, v)] = -1.5
    out = meshing.laplacian_solve(w, lap[2], adj, rhs, x0, pinned=pinned)
    assert out[2].tolist() == [2, 2, 1] and int(out[5][5]) == 0 and max(out[1].tolist()) < 10
    assert bool(torch.isfinite(out[0]).all()) and bool(torch.isfinite(out[3]).all())
    want = numpy_solve(w, lap[2], adj, rhs, x0, pinned.numpy(), 0.0, 1.0, 1e-10, 10000)
    same_outputs(out, want, ("indefinite",))
    # a weight that is not finite is not usable: the rule leaves the entry out, whichever end it is seen from, and every number
    # stays finite; nothing that is not finite reaches the iteration, so such a weight cannot make a NaN
    for bad in (float("nan"), float("inf")):
        for both in (False, True):
            w = lap[0].clone()
            w[entry_of(adj, v, n)] = bad
            if both:
                w[entry_of(adj, n, v)] = bad
            out = meshing.laplacian_solve(w, lap[2], adj, rhs, x0, pinned=pinned, max_iter=200)
            assert bool(torch.isfinite(out[0]).all()) and bool(torch.isfinite(out[3]).all()) and out[5].tolist()[:2] == [49, 32]
            if both:
                assert out[2].tolist() == [1, 1, 1]
    # a row of rhs or of the area that is not finite holds its vertex
    rhs2, area2 = rhs.clone(), lap[2].clone()
    rhs2[v, 1] = float("nan")
    area2[n] = float("nan")
    out = meshing.laplacian_solve(lap[0], area2, adj, rhs2, x0, pinned=pinned, mass_coef=1.0)
    assert dict(zip(NAMES, out[5].tolist())) == {"solved": 47, "pinned": 32, "not_live": 0, "bad_rhs": 1, "bad_area": 1, "bad_diagonal": 0}
    assert out[2].tolist() == [1, 1, 1] and bool(torch.isfinite(out[0]).all()) and out[6][v] == 3 and out[6][n] == 4
    # with mass_coef = 0 the area is not looked at
    out = meshing.laplacian_solve(lap[0], area2, adj, rhs, x0, pinned=pinned)
    assert int(out[5][4]) == 0 and out[2].tolist() == [1, 1, 1] and bool(torch.isfinite(out[0]).all())


# ---- 4: known answers ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ico3", "ico4"])
def test_an_implicit_step_shrinks_a_sphere_to_a_sphere(name):
    """Mean-curvature flow of a sphere of radius r: S p = (2 / r^2) M p, so (M + t S) p' = M p gives p' = p / (1 + 2 t / r^2)."""
    from arah_release_amd import geometry
    verts, faces = mesh(name)
    r, t = 0.75, mean_edge(name) ** 2
    out = geometry.smooth_mesh(verts, faces, iterations=1, method="implicit", time=t)
    radius = out.double().norm(dim=1)
    want = r / (1.0 + 2.0 * t / r ** 2)
    print("%s: t = h^2 = %.6g: mean radius %.6f against %.6f, spread %.3g" % (name, t, float(radius.mean()), want,
                                                                            float(radius.max() - radius.min())))
    assert out.dtype == torch.float32 and abs(float(radius.mean()) - want) <= 1e-4 * r
    assert float(radius.max() - radius.min()) < 2e-4 * r


@pytest.mark.parametrize("name,tol", [("jgrid9_0", 1e-10), ("jgrid33_1", 1e-10), ("jgrid9_0", 1e-13)])
def test_harmonic_extension_reproduces_a_linear_function(name, tol):
    from arah_release_amd import geometry
    verts, faces = mesh(name)
    adj = spec(name)[0]
    p = verts.double()
    f = torch.stack([0.3 * p[:, 0] - 1.7 * p[:, 1] + 0.25, 2.0 * p[:, 0] + 0.5 * p[:, 1] - 3.0], 1)
    known = (adj[6] & 1) != 0
    span = float((f.max(0).values - f.min(0).values).max())
    garbage = torch.where(known[:, None], f, torch.full_like(f, 1e9))            # values are read at the known vertices only
    out = geometry.harmonic_extend(verts, faces, known, garbage, tol=tol)
    err = float((out["values"] - f).abs().max()) / span
    print("%s tol %g: %s iterations, error %.3g of the range, true residual %s" % (name, tol, out["iterations"], err, out["true_residual"]))
    assert out["converged"] and out["status"] == ["converged"] * 2 and err <= 10 * tol
    assert max(out["true_residual"]) <= 10 * tol and max(out["residual"]) <= tol
    same_bits(out["values"][known], f[known], "known values stay")
    assert out["report"]["pinned"] == int(known.sum()) and out["report"]["solved"] == int((~known).sum())
    one = geometry.harmonic_extend(verts, faces, known, garbage[:, 0].float(), tol=tol)
    assert one["values"].shape == f.shape[:1] and one["values"].dtype == torch.float64 and one["status"] == "converged"
    assert float((one["values"] - f[:, 0]).abs().max()) <= 10 * tol * span + 2.0 ** -23 * float(f.abs().max())   # the float32 input


def test_a_component_without_a_known_vertex_keeps_zero():
    from arah_release_amd import geometry
    va, fa = mesh("jgrid9_0")
    vb, fb = mesh("octahedron")
    verts, faces = torch.cat([va, vb + 20.0]), torch.cat([fa, fb + va.shape[0]])
    known = torch.zeros(verts.shape[0], dtype=torch.bool)
    known[:9] = True
    out = geometry.harmonic_extend(verts, faces, known, verts.double().sum(1) + 1.0)
    assert out["converged"] and not bool(out["values"][va.shape[0]:].any()) and bool(out["values"][9:va.shape[0]].any())


def test_true_residual_is_small_wherever_a_column_converged():
    from arah_release_amd import geometry
    for name, tol in (("sphere9", 1e-10), ("open_sphere", 1e-10), ("bicone40", 1e-8), ("nan_vertex", 1e-12)):
        verts, faces = mesh(name)
        lap = geometry.mesh_laplacian(verts, faces)
        p = torch.nan_to_num(verts.double())
        t = mean_edge(name) ** 2
        out = geometry.solve_laplacian(lap, (lap["area"][:, None] * p).float(), 1.0, 10.0 * t, x0=verts, tol=tol)
        print("%s tol %g: iterations %s residual %s true %s" % (name, tol, out["iterations"], out["residual"], out["true_residual"]))
        assert out["converged"] and out["x"].dtype == torch.float64 and out["x"].shape == verts.shape
        assert all(r <= tol for r in out["residual"]) and all(r <= 10 * tol for r in out["true_residual"])
        assert sum(out["report"].values()) == verts.shape[0] and set(out["report"]) == set(NAMES)


@pytest.mark.parametrize("name", ["jgrid9_0", "jgrid33_1"])
def test_implicit_smoothing_keeps_a_planar_grid(name):
    """The cotangent operator has linear precision: S p = 0 at the interior of a planar mesh, so p solves (M + t S) p' = M p
    whatever t and however the grid is jittered.  The start is the solution; what is left is the float32 rounding of a solve that
    ends within tol: 2^-24 of the magnitude for the rounding, and as much again for the residual."""
    from arah_release_amd import geometry, meshing
    verts, faces = mesh(name)
    adj = spec(name)[0]
    held = (adj[6] & 3) != 0
    t = 25.0 * mean_edge(name) ** 2
    out = geometry.smooth_mesh(verts, faces, iterations=2, method="implicit", time=t, adjacency=adj)
    move = float((out - verts).abs().max())
    print("%s: two implicit iterations at t = 25 h^2 move a vertex by at most %.3g" % (name, move))
    assert move <= 2.0 ** -22 * float(verts.abs().max())
    same_bits(out[held], verts[held], "the pinned rim")
    same_bits(out, meshing.mesh_smooth_implicit(verts, faces, 2, t, adjacency=adj), "the rule")
    free = geometry.smooth_mesh(verts, faces, iterations=1, method="implicit", time=t, boundary="free")
    assert float((free - verts)[held].abs().max()) > 1e-3                          # a free rim shrinks


def test_held_vertices_stay_bit_for_bit():
    from arah_release_amd import geometry
    verts, faces = mesh("nan_vertex")
    out = geometry.smooth_mesh(verts, faces, iterations=2, method="implicit", time=4.0 * mean_edge("nan_vertex") ** 2)
    same_bits(out[11], verts[11], "the vertex that is not finite")
    rest = torch.arange(verts.shape[0]) != 11
    assert bool(torch.isfinite(out[rest]).all()) and bool((out[rest] != verts[rest]).any(1).all())
    verts, faces = mesh("open_sphere")
    flags = spec("open_sphere")[0][6]
    stay = (flags & 7) != 0                                                       # the rim, and the isolated vertices (no area)
    out = geometry.smooth_mesh(verts, faces, iterations=1, method="implicit", time=mean_edge("open_sphere") ** 2)
    same_bits(out[stay], verts[stay], "rim and isolated vertices")
    assert bool((out[~stay] != verts[~stay]).any(1).all())
    same_bits(geometry.smooth_mesh(verts, faces, iterations=0, method="implicit", time=1.0), verts, "no iteration")
    same_bits(geometry.smooth_mesh(verts[:0], faces[:0], iterations=1, method="implicit", time=1.0), verts[:0], "no mesh")


def test_a_solve_that_does_not_converge_raises():
    from arah_release_amd import meshing
    verts, faces = mesh("jgrid33_1")
    with pytest.raises(RuntimeError, match="max_iter"):
        meshing.mesh_smooth_implicit(verts, faces, 1, 100.0, boundary="free", max_iter=2)


# ---- 5: the surface --------------------------------------------------------------------------------------------------------------------
def test_argument_checks():
    from arah_release_amd import geometry, meshing
    verts, faces = mesh("octahedron")
    adj, lap, _ = spec("octahedron")
    V = verts.shape[0]
    rhs = verts.double()
    good = dict(weight=lap[0], area=lap[2], adjacency=adj, rhs=rhs, x0=rhs)
    meshing.laplacian_solve(**good, mass_coef=1.0)
    for bad in ({"rhs": rhs.float()}, {"x0": rhs.float()}, {"rhs": rhs[:5]}, {"rhs": rhs[:, 0]}, {"x0": rhs[:, :2]}, {"area": lap[2].float()},
                {"area": lap[2][:5]}, {"weight": lap[0].float()}, {"weight": lap[0][:-1]}, {"adjacency": adj[:7]},
                {"rhs": torch.zeros(V, 0, dtype=torch.float64), "x0": torch.zeros(V, 0, dtype=torch.float64)},
                {"rhs": torch.zeros(V, 33, dtype=torch.float64), "x0": torch.zeros(V, 33, dtype=torch.float64)},
                {"pinned": torch.zeros(V, dtype=torch.uint8)}, {"pinned": torch.zeros(V - 1, dtype=torch.bool)},
                {"mass_coef": -1.0}, {"mass_coef": float("nan")}, {"mass_coef": None}, {"stiff_coef": 0.0}, {"stiff_coef": -1.0},
                {"stiff_coef": float("inf")}, {"tol": -1e-3}, {"tol": float("nan")}, {"max_iter": -1}, {"max_iter": 2.5}):
        with pytest.raises(ValueError):
            meshing.laplacian_solve(**dict(dict(good, mass_coef=1.0), **bad))
    with pytest.raises(ValueError, match="2\\^24"):                               # by the size check alone: nothing that large is built
        meshing.check_solve_size(2 ** 24 + 1)
    meshing.check_solve_size(2 ** 24)
    d = geometry.mesh_laplacian(verts, faces)
    for bad in ({"rhs": rhs.long()}, {"rhs": rhs[None]}, {"x0": rhs[:, 0]}, {"x0": rhs.half()}, {"mass_coef": -0.5}, {"stiff_coef": 0.0},
                {"rhs": torch.zeros(V, 33)}, {"rhs": torch.zeros(V, 0)}, {"pinned": torch.zeros(V)}, {"lap": {"weight": lap[0]}}):
        with pytest.raises(ValueError):
            geometry.solve_laplacian(**dict(dict(lap=d, rhs=rhs, mass_coef=1.0), **bad))
    known = torch.zeros(V, dtype=torch.bool)
    for bad in ({"known": known[:-1]}, {"known": known.long()}, {"values": rhs[:-1]}, {"values": rhs.long()}, {"values": torch.zeros(V, 33)}):
        with pytest.raises(ValueError):
            geometry.harmonic_extend(verts, faces, **dict(dict(known=known, values=rhs), **bad))
    for bad in ({}, {"time": None}, {"time": 0.0}, {"time": -1.0}, {"time": float("nan")}, {"time": float("inf")}, {"time": "1"},
                {"time": 1.0, "boundary": "pinned"}, {"time": 1.0, "iterations": -1}):
        with pytest.raises(ValueError):
            geometry.smooth_mesh(verts, faces, **dict({"method": "implicit", "iterations": 1}, **bad))
        with pytest.raises(ValueError):
            geometry.check_smooth(dict({"method": "implicit"}, **bad))
    for method in ("taubin", "laplacian", "tangential"):                            # time belongs to the implicit method
        with pytest.raises(ValueError):
            geometry.smooth_mesh(verts, faces, 1, method=method, time=1.0)
    # empty inputs
    for v, f in ((verts[:0], faces[:0]), (verts, faces[:0])):
        e = geometry.mesh_laplacian(v, f)
        out = geometry.solve_laplacian(e, v.double(), 1.0, 1.0)
        assert out["x"].shape == v.shape and out["converged"] and out["iterations"] == [0, 0, 0]
        assert out["report"]["solved"] == 0 and out["report"]["bad_area"] == v.shape[0]


def test_check_smooth_takes_the_new_keys_and_still_refuses_the_old_cases():
    from arah_release_amd import geometry
    for kw in ({"method": "implicit", "time": 0.01}, {"method": "implicit", "time": 2, "iterations": 3, "boundary": "free"}):
        assert geometry.check_smooth(kw) == kw
    assert "time" in geometry._SMOOTH_KEYS
    # what the existing tests expect check_smooth to refuse (tests/test_mesh_adjacency.py, test_mesh_tangential.py,
    # test_mesh_laplacian.py) is still refused, and what they expect it to take is still taken unchanged
    for bad in ({"weights": "cotan"}, {"weights": None}, {"weights": "cotangent", "method": "tangential"}, {"method": "tangential", "boundary": "free"},
                {"lamb": 0.0}, {"lamb": 1.5}, {"mu": 0.5}, {"method": "umbrella"}, {"boundary": "open"}, {"iterations": -1}, {"steps": 3}, -1,
                True, 2.5, "3", {"time": 1.0}, {"method": "taubin", "time": 1.0}):
        with pytest.raises(ValueError):
            geometry.check_smooth(bad)
    assert geometry.check_smooth(None) is None and geometry.check_smooth(4) == {"iterations": 4}
    assert geometry.check_smooth({"weights": "cotangent", "iterations": 2}) == {"weights": "cotangent", "iterations": 2}
    assert geometry.check_smooth({"method": "tangential", "lamb": 0.3}) == {"method": "tangential", "lamb": 0.3}


def test_abi_is_declared_and_checks_its_arguments():
    import ctypes as C
    from arah_release_amd import hip, meshing
    with open(os.path.join(REPO, "include", "arah_hip.h")) as fh:
        declared = set(re.findall(r"\b(arah_\w+)\s*\(", fh.read()))
    lib = hip.load_library()
    for name in NEW_EXPORTS:
        assert name in declared and name in hip.EXPORTS and hasattr(lib, name), name
    assert len(hip.EXPORTS) == len(set(hip.EXPORTS))
    with open(os.path.join(REPO, "arah_release_amd", "csrc", "meshsolve.hpp")) as fh:
        text = fh.read()
    assert "kMzMaxVerts = 1 << 24" in text and meshing.SOLVE_MAX_VERTS == 1 << 24 and "fp contract(off)" in text
    size = lib.arah_mesh_solve_scratch_bytes
    # d and four vectors of C columns, the blocks' partial sums, the columns' scalars, two bytes a vertex
    assert size(1000, 3) >= 8 * 1000 * (1 + 4 * 3) + 2 * 3 * 4 * 8 + 2 * 1000 and size(0, 1) > 0 and size(1000, 3) % 256 == 0
    assert size(1000, 32) > size(1000, 3) and size(2 ** 24, 1) > 0
    for sizes in ((-1, 1), (2 ** 24 + 1, 1), (10, 0), (10, 33), (10, -1)):
        assert size(*sizes) == 0, sizes
    p = C.c_void_p(256)                                                           # never dereferenced: every call is refused
    i64, i32, f64 = C.c_int64, C.c_int32, C.c_double

    def begin(V=4, F=4, n_ch=3, mc=1.0, sc=1.0, tol=1e-10, w=p, area=p, start=p, rhs=p, x0=p, x=p, scratch=p):
        return lib.arah_mesh_solve_begin(w, area, start, p, i64(V), i64(F), rhs, x0, None, i32(n_ch), f64(mc), f64(sc), f64(tol), x, p, p, p,
                                         p, p, p, scratch, C.c_size_t(1 << 30), None)
    for bad in ({"V": -1}, {"V": 2 ** 24 + 1}, {"F": -1}, {"F": 2 ** 28 + 1}, {"n_ch": 0}, {"n_ch": 33}, {"mc": -1.0}, {"mc": float("nan")},
                {"sc": 0.0}, {"sc": -2.0}, {"sc": float("inf")}, {"tol": -1.0}, {"tol": float("nan")}, {"w": None}, {"area": None},
                {"start": None}, {"rhs": None}, {"x0": None}, {"x": None}, {"scratch": None}):
        assert begin(**bad) == -1, bad                                            # ARAH_E_BADARG, nothing launched

    def steps(V=4, F=4, n_ch=3, mc=1.0, sc=1.0, n=2, w=p, area=p, start=p, x=p, scratch=p):
        return lib.arah_mesh_solve_steps(w, area, start, p, i64(V), i64(F), i32(n_ch), f64(mc), f64(sc), i32(n), x, p, p, p, p, scratch,
                                         C.c_size_t(1 << 30), None)
    for bad in ({"V": -1}, {"V": 2 ** 24 + 1}, {"F": -1}, {"n_ch": 0}, {"n_ch": 33}, {"mc": -1.0}, {"sc": 0.0}, {"n": -1}, {"w": None},
                {"area": None}, {"start": None}, {"x": None}, {"scratch": None}):
        assert steps(**bad) == -1, bad
    # a scratch that is too short is refused before anything is launched
    assert lib.arah_mesh_solve_begin(p, p, p, p, i64(4), i64(4), p, p, None, i32(3), f64(1.0), f64(1.0), f64(1e-10), p, p, p, p, p, p, p, p,
                                     C.c_size_t(size(4, 3) - 1), None) == -3
    assert lib.arah_mesh_solve_steps(p, p, p, p, i64(4), i64(4), i32(3), f64(1.0), f64(1.0), i32(1), p, p, p, p, p, p,
                                     C.c_size_t(size(4, 3) - 1), None) == -3
