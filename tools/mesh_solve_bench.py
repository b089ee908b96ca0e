"""Cost of solving with the cotangent operator on the device (hip.laplacian_solve; geometry.solve_laplacian / harmonic_extend /
smooth_mesh(method="implicit")).

    python tools/mesh_solve_bench.py [--n-side 256] [--reps 5] [--spec-reps 1] [--out profiles/mesh_solve_bench.txt]

Four meshes: the synthetic subject's posed level set at n_side^3 as an indexed mesh, its decimate_mesh(target_faces=10000), and each
of the two after flip_edges("delaunay").  On each, after a warm-up of every route at this size, with device events around the
calls (they include the host's looks at the statuses, one per batch of 32 steps) and the routes alternated in one loop, medians:

  * one implicit smoothing step (M + t S) p' = M p at t = 1, 10 and 100 mean-edge^2, tol 1e-10, over a prebuilt operator: the steps
    it takes, its time, the time per step;
  * a harmonic extension from 1 % known vertices (seeded);
  * the tensor specification meshing.laplacian_solve on the same GPU tensors (t = 1 only: it takes a hundred launches a step);
  * alongside, the same preconditioned conjugate gradients written with what the toolkit had before -- geometry.laplacian_matrix
    and torch's sparse CSR product, torch reductions for the inner products, the statuses read every 32 steps as well.  Its sums
    are not in a fixed order, so its step counts may differ by a few.

The kernels' results are compared with the specification's while at it."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TOL = 1e-10
MAX_ITER = 20000


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def med(v):
    return "median %.3f ms (min %.3f, max %.3f, %d calls)" % (statistics.median(v), min(v), max(v), len(v))


def torch_pcg(A, d, rhs, x0, free, check_every=32):
    """Jacobi-preconditioned CG on the rows `free` with a torch sparse CSR matrix (columns of held rows act through x0)."""
    x = x0.clone()
    mask = free[:, None].to(rhs.dtype)
    r = (rhs - A @ x) * mask
    z = r / d[:, None]
    p = z.clone()
    rz, r0 = (r * z).sum(0), (r * r).sum(0)
    thr = TOL * TOL * r0
    steps = 0
    while steps < MAX_ITER:
        for _ in range(check_every):
            q = (A @ p) * mask
            alpha = rz / (p * q).sum(0)
            x = x + alpha * p
            r = r - alpha * q
            z = r / d[:, None]
            rz_new = (r * z).sum(0)
            p = z + (rz_new / rz) * p
            rz = rz_new
            steps += 1
        if bool(((r * r).sum(0) <= thr).all()):                                   # the look at the statuses, once per batch
            break
    return x, steps


def measure(label, verts, faces, args, lines):
    from arah_release_amd import geometry, hip, meshing
    V, F = int(verts.shape[0]), int(faces.shape[0])
    lap = geometry.mesh_laplacian(verts, faces)
    adj, weight, area = tuple(lap["adjacency"]), lap["weight"], lap["area"]
    p = verts[faces.long()].double()
    h = float(torch.cat([(p[:, i] - p[:, (i + 1) % 3]).norm(dim=1) for i in range(3)]).mean())
    lines.append("")
    lines.append("%s: %d vertices, %d faces, mean edge %.5f; %s" % (label, V, F, h, ", ".join("%s %d" % kv for kv in lap["report"].items())))
    pos = verts.double()
    rhs = area[:, None] * pos
    L = geometry.laplacian_matrix(lap).to_sparse_coo()
    ids = torch.arange(V, device=verts.device)
    mass = torch.sparse_coo_tensor(torch.stack([ids, ids]), area, (V, V))

    def csr(m):
        return m.coalesce().to_sparse_csr()

    all_free = torch.ones(V, dtype=torch.bool, device=verts.device)
    g = torch.Generator().manual_seed(1)
    known = (torch.rand(V, generator=g) < 0.01).to(verts.device)
    values = torch.where(known[:, None], pos, torch.zeros_like(pos))
    routes, spec_routes, steps = {}, {}, {}
    for factor in (1, 10, 100):
        t = factor * h * h
        A = csr(mass - t * L)
        d = area + t * lap["diag"]
        routes["implicit step t = %3d h^2  kernels  hip.laplacian_solve" % factor] = \
            lambda t=t: hip.laplacian_solve(weight, area, adj, rhs, pos, mass_coef=1.0, stiff_coef=t, tol=TOL, max_iter=MAX_ITER)
        routes["implicit step t = %3d h^2  torch    sparse CSR products" % factor] = lambda A=A, d=d: torch_pcg(A, d, rhs, pos, all_free)
        if factor == 1:
            spec_routes["implicit step t = %3d h^2  spec     meshing.laplacian_solve" % factor] = \
                lambda t=t: meshing.laplacian_solve(weight, area, adj, rhs, pos, mass_coef=1.0, stiff_coef=t, tol=TOL, max_iter=MAX_ITER)
    A0 = csr(-1.0 * L)
    routes["harmonic extension, 1 % known  kernels  hip.laplacian_solve"] = \
        lambda: hip.laplacian_solve(weight, area, adj, torch.zeros_like(pos), values, pinned=known, tol=TOL, max_iter=MAX_ITER)
    routes["harmonic extension, 1 % known  torch    sparse CSR products"] = \
        lambda: torch_pcg(A0, lap["diag"], torch.zeros_like(pos), values, ~known)
    routes["implicit step t =  10 h^2  public   geometry.smooth_mesh(method='implicit', iterations=1) (builds everything)"] = \
        lambda: geometry.smooth_mesh(verts, faces, iterations=1, method="implicit", time=10 * h * h)
    for fn in routes.values():                                                    # warm-up: every route, at this size
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in list(routes) + list(spec_routes)}
    for r in range(args.reps):                                                    # alternating
        for name, fn in routes.items():
            ms, out = timed(fn)
            t[name].append(ms)
            if torch.is_tensor(out):
                continue
            steps[name] = out[1] if isinstance(out[1], int) else out[1].tolist()
            if not isinstance(out[1], int):
                assert out[2].tolist() == [1, 1, 1], (name, out[2].tolist())
        if r < args.spec_reps:
            for name, fn in spec_routes.items():
                ms, out = timed(fn)
                t[name].append(ms)
                steps[name] = out[1].tolist()
                got = hip.laplacian_solve(weight, area, adj, rhs, pos, mass_coef=1.0, stiff_coef=h * h, tol=TOL, max_iter=MAX_ITER)
                same = all(torch.equal(a, b) for a, b in zip(got, out))
                lines.append("kernels against the specification at this size (t = h^2): x, iters, status, rr, r0, counts, classes %s"
                             % ("bit-equal" if same else "DIFFER"))
    for name in sorted(t):
        if not t[name]:
            continue
        line = "%-62s %s" % (name, med(t[name]))
        if name in steps:
            n = steps[name] if isinstance(steps[name], int) else max(steps[name])
            line += "; steps %s; %.2f us a step" % (steps[name], 1e3 * statistics.median(t[name]) / max(n, 1))
        lines.append(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-side", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spec-reps", type=int, default=1)
    ap.add_argument("--target-faces", type=int, default=10000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from arah_release_amd import config, geometry, synthetic
    dev = torch.device("cuda:0")
    model, _ = config.build_synthetic_model("zju377_mono", device=dev)
    model.eval()
    inputs = synthetic.SyntheticScene(0).make_inputs(32, 32, frame_idx=0, device=dev)
    lines = ["%s, torch %s, HIP %s" % (torch.cuda.get_device_name(0), torch.__version__, torch.version.hip),
             "one session; device events around each call, host looks at the statuses included; a kernel step is 4 launches, a solve 5 "
             "more at its start and 1 per batch of 32 steps; tol %g" % TOL]
    with torch.no_grad():
        posed = model.posed_mesh(inputs, n_side=args.n_side, indexed=True)
        verts, faces = posed["verts"].contiguous(), posed["faces"].contiguous()
        measure("posed level set at %d^3" % args.n_side, verts, faces, args, lines)
        flipped = geometry.flip_edges(verts, faces, "delaunay")
        measure("... after flip_edges('delaunay') (%d rounds, %d flips)" % (flipped["rounds"], flipped["flips"]), verts,
                flipped["faces"].contiguous(), args, lines)
        small = geometry.decimate_mesh(verts, faces, target_faces=args.target_faces)
        sv, sf = small["verts"].contiguous(), small["faces"].contiguous()
        measure("decimate_mesh(target_faces=%d)" % args.target_faces, sv, sf, args, lines)
        flipped = geometry.flip_edges(sv, sf, "delaunay")
        measure("... after flip_edges('delaunay') (%d rounds, %d flips)" % (flipped["rounds"], flipped["flips"]), sv,
                flipped["faces"].contiguous(), args, lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
