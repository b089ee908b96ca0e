"""Cost of the device-side adjacency, per-vertex normals and smoothing (hip.mesh_adjacency / hip.vertex_normals / hip.mesh_smooth;
geometry.mesh_adjacency / mesh_topology / vertex_normals / smooth_mesh).

    python tools/mesh_smooth_bench.py [--n-side 256] [--reps 20] [--spec-reps 5] [--iterations 10] [--out profiles/mesh_smooth_bench.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/mesh_smooth_bench.py --reps 5 --spec-reps 0       # per kernel

The synthetic subject's posed level set at n_side^3 as an indexed mesh (what posed_mesh(indexed=True) gives).  After warm-up of
every route at this size, with device events around the calls and the routes alternated in one loop: median time of the adjacency
build, of the normals and of `--iterations` Taubin iterations over a prebuilt adjacency -- the kernels (hip.*), the public calls
(geometry.*, which build their own adjacency unless handed one) and the tensor specification (meshing.*) running on the same GPU
tensors.  The kernels' results are compared with the specification's for equality while at it, at this size."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-side", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--spec-reps", type=int, default=5)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from arah_release_amd import config, geometry, hip, meshing, synthetic
    dev = torch.device("cuda:0")
    model, _ = config.build_synthetic_model("zju377_mono", device=dev)
    model.eval()
    inputs = synthetic.SyntheticScene(0).make_inputs(32, 32, frame_idx=0, device=dev)
    with torch.no_grad():
        posed = model.posed_mesh(inputs, n_side=args.n_side, indexed=True)
    verts, faces = posed["verts"].contiguous(), posed["faces"].contiguous()
    V, F, it = int(verts.shape[0]), int(faces.shape[0]), args.iterations
    topo = geometry.mesh_topology(verts, faces)
    lines = ["%s, torch %s, HIP %s" % (torch.cuda.get_device_name(0), torch.__version__, torch.version.hip),
             "posed level set at %d^3: %d vertices, %d faces; %s" % (args.n_side, V, F, ", ".join("%s %s" % kv for kv in topo.items()))]
    adj = hip.mesh_adjacency(faces, V)
    routes = {
        "adjacency  kernels  hip.mesh_adjacency": lambda: hip.mesh_adjacency(faces, V),
        "adjacency  public   geometry.mesh_topology (with its host read)": lambda: geometry.mesh_topology(verts, faces),
        "normals    kernel   hip.vertex_normals(adjacency=)": lambda: hip.vertex_normals(verts, faces, adjacency=adj),
        "normals    public   geometry.vertex_normals (builds the adjacency)": lambda: geometry.vertex_normals(verts, faces),
        "smoothing  kernel   hip.mesh_smooth(%d, adjacency=)" % it: lambda: hip.mesh_smooth(verts, faces, it, adjacency=adj),
        "smoothing  public   geometry.smooth_mesh(%d) (builds the adjacency)" % it: lambda: geometry.smooth_mesh(verts, faces, it),
    }
    spec_routes = {
        "adjacency  spec     meshing.mesh_adjacency": lambda: meshing.mesh_adjacency(faces, V),
        "normals    spec     meshing.vertex_normals(adjacency=)": lambda: meshing.vertex_normals(verts, faces, adjacency=adj),
        "smoothing  spec     meshing.mesh_smooth(%d, adjacency=)" % it: lambda: meshing.mesh_smooth(verts, faces, it, adjacency=adj),
    }
    with torch.no_grad():
        for _ in range(3):                                                        # warm-up: every route, at this size
            for fn in routes.values():
                fn()
        if args.spec_reps:
            for fn in spec_routes.values():
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in list(routes) + list(spec_routes)}
        for r in range(args.reps):                                                # alternating
            for name, fn in routes.items():
                t[name].append(timed(fn)[0])
            if r < args.spec_reps:
                for name, fn in spec_routes.items():
                    t[name].append(timed(fn)[0])
        for name in sorted(t):
            if t[name]:
                lines.append("%-72s %s" % (name, med(t[name])))
        if args.spec_reps:
            same_adj = all(torch.equal(a, b) for a, b in zip(adj, meshing.mesh_adjacency(faces, V)))
            got_n, want_n = hip.vertex_normals(verts, faces, adjacency=adj), meshing.vertex_normals(verts, faces, adjacency=adj)
            same_n = torch.equal(got_n[0], want_n[0]) and torch.equal(got_n[1], want_n[1])
            same_s = torch.equal(hip.mesh_smooth(verts, faces, it, adjacency=adj), meshing.mesh_smooth(verts, faces, it, adjacency=adj))
            lines.append("kernels against the specification at this size: adjacency %s, normals %s, smoothing %s" %
                         tuple("bit-equal" if s else "DIFFER" for s in (same_adj, same_n, same_s)))
            for what in ("adjacency", "normals", "smoothing"):
                k = statistics.median(next(v for n, v in t.items() if n.startswith(what) and "kernel" in n))
                s = statistics.median(next(v for n, v in t.items() if n.startswith(what) and "spec" in n))
                lines.append("%-10s specification / kernels = %.1f x" % (what, s / k))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
