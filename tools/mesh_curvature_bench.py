"""Cost of the cotangent Laplacian, its application, the curvatures and cotangent smoothing on the device (hip.mesh_cotangent /
laplacian_apply / mesh_curvature / mesh_smooth(weights="cotangent"); geometry.mesh_laplacian / mesh_curvature / smooth_mesh).

    python tools/mesh_curvature_bench.py [--n-side 256] [--reps 20] [--spec-reps 2] [--iterations 10] [--out profiles/mesh_curvature_bench.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/mesh_curvature_bench.py --reps 5 --spec-reps 0       # per kernel

Three meshes: the synthetic subject's posed level set at n_side^3 as an indexed mesh, its decimate_mesh(target_faces=10000), and
that after flip_edges("delaunay").  On each, after warm-up of every route at this size, with device events around the calls and the
routes alternated in one loop: median time of the adjacency build (for scale), of the operator, of its application to the
positions, of the curvatures and of `--iterations` Taubin iterations with uniform and with cotangent weights, all over a prebuilt
adjacency -- the kernels (hip.*) and the tensor specification (meshing.*) running on the same GPU tensors.  The kernels' results are
compared with the specification's while at it (bit-equal but for the angles' atan2), and the share of edges with a negative weight
is recorded: what the Delaunay flips are for."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def med(v):
    return "median %.3f ms (min %.3f, max %.3f, %d calls)" % (statistics.median(v), min(v), max(v), len(v))


def measure(label, verts, faces, args, lines):
    from arah_release_amd import geometry, hip, meshing
    V, F, it = int(verts.shape[0]), int(faces.shape[0]), args.iterations
    topo = geometry.mesh_topology(verts, faces)
    adj = hip.mesh_adjacency(faces, V)
    lap = hip.mesh_cotangent(verts, faces, "mixed", adj)
    normal_sum = hip.vertex_normals(verts, faces, adjacency=adj)[0]
    c = dict(zip(meshing.COTANGENT_COUNTS, lap[4].tolist()))
    lines.append("")
    lines.append("%s: %d vertices, %d faces, %d edges, max valence %d; %s" % (label, V, F, topo["edges"], topo["max_valence"],
                                                                             ", ".join("%s %d" % kv for kv in c.items())))
    lines.append("%-72s %d of %d = %.3f %%" % ("edges with a negative weight", c["negative_edges"], topo["edges"],
                                               100.0 * c["negative_edges"] / max(topo["edges"], 1)))
    routes = {
        "adjacency  kernels  hip.mesh_adjacency (for scale)": lambda: hip.mesh_adjacency(faces, V),
        "operator   kernels  hip.mesh_cotangent(adjacency=)": lambda: hip.mesh_cotangent(verts, faces, "mixed", adj),
        "apply      kernel   hip.laplacian_apply(weight, adjacency, verts)": lambda: hip.laplacian_apply(lap[0], adj, verts),
        "curvature  kernel   hip.mesh_curvature(adjacency=, laplacian=, normal_sum=)":
            lambda: hip.mesh_curvature(verts, faces, "mixed", adj, lap, normal_sum),
        "curvature  public   geometry.mesh_curvature (builds everything, one host read)": lambda: geometry.mesh_curvature(verts, faces),
        "smoothing  uniform    hip.mesh_smooth(%d, adjacency=)" % it: lambda: hip.mesh_smooth(verts, faces, it, adjacency=adj),
        "smoothing  cotangent  hip.mesh_smooth(%d, adjacency=, weights='cotangent')" % it:
            lambda: hip.mesh_smooth(verts, faces, it, adjacency=adj, weights="cotangent"),
    }
    spec_routes = {
        "operator   spec     meshing.mesh_cotangent(adjacency=)": lambda: meshing.mesh_cotangent(verts, faces, "mixed", adj),
        "apply      spec     meshing.laplacian_apply": lambda: meshing.laplacian_apply(lap[0], adj, verts),
        "curvature  spec     meshing.mesh_curvature(adjacency=, laplacian=, normal_sum=)":
            lambda: meshing.mesh_curvature(verts, faces, "mixed", adj, lap, normal_sum),
        "smoothing  cotangent  spec  meshing.mesh_smooth(%d, adjacency=, weights='cotangent')" % it:
            lambda: meshing.mesh_smooth(verts, faces, it, adjacency=adj, weights="cotangent"),
    }
    for _ in range(3):                                                            # warm-up: every route, at this size
        for fn in routes.values():
            fn()
    if args.spec_reps:
        for fn in spec_routes.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in list(routes) + list(spec_routes)}
    for r in range(args.reps):                                                    # alternating
        for name, fn in routes.items():
            t[name].append(timed(fn)[0])
        if r < args.spec_reps:
            for name, fn in spec_routes.items():
                t[name].append(timed(fn)[0])
    for name in sorted(t):
        if t[name]:
            lines.append("%-72s %s" % (name, med(t[name])))
    if args.spec_reps:
        want = meshing.mesh_cotangent(verts, faces, "mixed", adj)
        same = [torch.equal(lap[i], want[i]) for i in (0, 1, 2, 4)]
        angle = float((lap[3] - want[3]).abs().max())
        got_c, want_c = hip.mesh_curvature(verts, faces, "mixed", adj, lap, normal_sum), meshing.mesh_curvature(verts, faces, "mixed", adj, lap,
                                                                                                               normal_sum)
        same_c = all(torch.equal(torch.nan_to_num(a.double()), torch.nan_to_num(b.double())) for a, b in zip(got_c, want_c))
        same_a = torch.equal(hip.laplacian_apply(lap[0], adj, verts), meshing.laplacian_apply(lap[0], adj, verts))
        same_s = torch.equal(hip.mesh_smooth(verts, faces, it, adjacency=adj, weights="cotangent"),
                             meshing.mesh_smooth(verts, faces, it, adjacency=adj, weights="cotangent"))
        word = lambda s: "bit-equal" if s else "DIFFER"                            # noqa: E731
        lines.append("kernels against the specification at this size: weight %s, diag %s, area %s, counts %s, angle_sum within %.3g; "
                     "apply %s, curvature (same angle_sum) %s, cotangent smoothing %s"
                     % (tuple(word(s) for s in same) + (angle, word(same_a), word(same_c), word(same_s))))
        for what, kernel, spec in (("operator", "operator   kernels", "operator   spec"), ("apply", "apply      kernel", "apply      spec"),
                                   ("curvature", "curvature  kernel", "curvature  spec"),
                                   ("cotangent smoothing", "smoothing  cotangent  hip", "smoothing  cotangent  spec")):
            k = statistics.median(next(v for n, v in t.items() if n.startswith(kernel)))
            s = statistics.median(next(v for n, v in t.items() if n.startswith(spec)))
            lines.append("%-20s specification / kernels = %.1f x" % (what, s / k))
    u = statistics.median(next(v for n, v in t.items() if n.startswith("smoothing  uniform")))
    k = statistics.median(next(v for n, v in t.items() if n.startswith("smoothing  cotangent  hip")))
    lines.append("%-20s cotangent / uniform = %.1f x" % ("smoothing", k / u))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-side", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--spec-reps", type=int, default=2)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--target-faces", type=int, default=10000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from arah_release_amd import config, geometry, synthetic
    dev = torch.device("cuda:0")
    model, _ = config.build_synthetic_model("zju377_mono", device=dev)
    model.eval()
    inputs = synthetic.SyntheticScene(0).make_inputs(32, 32, frame_idx=0, device=dev)
    lines = ["%s, torch %s, HIP %s" % (torch.cuda.get_device_name(0), torch.__version__, torch.version.hip)]
    with torch.no_grad():
        posed = model.posed_mesh(inputs, n_side=args.n_side, indexed=True)
        verts, faces = posed["verts"].contiguous(), posed["faces"].contiguous()
        measure("posed level set at %d^3" % args.n_side, verts, faces, args, lines)
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
