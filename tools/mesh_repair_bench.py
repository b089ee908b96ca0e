"""Cost of the device-side orientation, boundary loops and hole filling (hip.mesh_orient / hip.mesh_boundary_loops /
hip.mesh_fill_holes; geometry.orient_mesh / boundary_loops / fill_holes / repair_mesh).

    python tools/mesh_repair_bench.py [--n-side 256] [--reps 20] [--spec-reps 3] [--holes 64] [--out profiles/mesh_repair_bench.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/mesh_repair_bench.py --reps 5 --spec-reps 0       # per kernel

The synthetic subject's posed level set at n_side^3 as an indexed mesh with 30 % of its faces reversed (seeded) and the stars of
`--holes` evenly spaced vertices removed, and the same mesh simplified with cells of 2 and of 4 / (n_side - 1) of its longest
side.  For each of them, after
warm-up of every route at this size, with device events around whole calls and the routes alternated in one loop: median time of
the adjacency build, of the orientation ("majority" and "negative") over a prebuilt adjacency, and of the boundary loops and the
hole filling of the ORIENTED mesh over its prebuilt adjacency -- the kernels (hip.*), the public calls (geometry.*, which build
their own adjacency and read their counts back) and the tensor specification (meshing.*) running on the same GPU tensors.  The
lattices (meshing.orient_quant / fill_quant, one host read each) are taken once outside the timed kernel and specification calls.
The kernels' results are compared with the specification's for equality while at it, at this size."""
import argparse
import datetime
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


def same(a, b):
    return all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
               for x, y in zip(a, b))


def damage(verts, faces, n_holes):
    """30 % of the rows reversed, then the stars of n_holes evenly spaced vertices removed."""
    F, V = int(faces.shape[0]), int(verts.shape[0])
    pick = (torch.rand(F, generator=torch.Generator().manual_seed(3)) < 0.3).to(faces.device)
    faces = torch.where(pick[:, None], faces[:, [0, 2, 1]], faces)
    if n_holes > 0 and V > 0:
        gone = torch.zeros(V + 1, dtype=torch.bool, device=faces.device)
        gone[torch.arange(n_holes, device=faces.device) * max(V // n_holes, 1) % V] = True
        faces = faces[~gone[faces.long().clamp(0, V)].any(1)]
    return faces.contiguous()


def bench(label, verts, faces, args, lines):
    from arah_release_amd import geometry, hip, meshing
    V, F = int(verts.shape[0]), int(faces.shape[0])
    topo = geometry.mesh_topology(verts, faces)
    lines.append("")
    lines.append("%s: %d vertices, %d faces; %s" % (label, V, F, ", ".join("%s %s" % kv for kv in topo.items())))
    adj = hip.mesh_adjacency(faces, V)
    oq, fq = meshing.orient_quant(verts), meshing.fill_quant(verts)
    oriented = hip.mesh_orient(V, faces, policy="majority", adjacency=adj)
    fo = oriented[2]
    adj_o = hip.mesh_adjacency(fo, V)
    loops = hip.mesh_boundary_loops(fo, V, adjacency=adj_o)
    c, lc = oriented[7].tolist(), loops[6].tolist()
    fc = hip.mesh_fill_holes(verts, fo, loops=loops, quant=fq)[4].tolist()
    lines.append("orientation: %d components, %d non-orientable, %d faces flipped; oriented mesh: %d boundary edges in %d loops (%d "
                 "simple), %d loops filled with %d faces" % (c[1], c[2], c[5], lc[0], lc[1], lc[2], fc[3], fc[4]))
    routes = {
        "adjacency  kernels  hip.mesh_adjacency": lambda: hip.mesh_adjacency(faces, V),
        "orient     kernels  hip.mesh_orient('majority', adjacency=)": lambda: hip.mesh_orient(V, faces, policy="majority", adjacency=adj),
        "orient-vol kernels  hip.mesh_orient('negative', adjacency=, quant=)":
            lambda: hip.mesh_orient(verts, faces, policy="negative", adjacency=adj, quant=oq),
        "orient     public   geometry.orient_mesh (builds the adjacency, reads the counts)": lambda: geometry.orient_mesh(verts, faces),
        "loops      kernels  hip.mesh_boundary_loops(adjacency=)": lambda: hip.mesh_boundary_loops(fo, V, adjacency=adj_o),
        "loops      public   geometry.boundary_loops (builds the adjacency, reads the counts)": lambda: geometry.boundary_loops(verts, fo),
        "fill       kernels  hip.mesh_fill_holes(loops=, quant=)": lambda: hip.mesh_fill_holes(verts, fo, loops=loops, quant=fq),
        "fill       public   geometry.fill_holes (adjacency, loops, bounds and counts)": lambda: geometry.fill_holes(verts, fo),
        "repair     public   geometry.repair_mesh (orient, fill, topology)": lambda: geometry.repair_mesh(verts, faces),
    }
    spec_routes = {
        "adjacency  spec     meshing.mesh_adjacency": lambda: meshing.mesh_adjacency(faces, V),
        "orient     spec     meshing.mesh_orient('majority')": lambda: meshing.mesh_orient(V, faces, policy="majority"),
        "orient-vol spec     meshing.mesh_orient('negative', quant=)": lambda: meshing.mesh_orient(verts, faces, policy="negative", quant=oq),
        "loops      spec     meshing.mesh_boundary_loops": lambda: meshing.mesh_boundary_loops(fo, V),
        "fill       spec     meshing.mesh_fill_holes(loops=, quant=)": lambda: meshing.mesh_fill_holes(verts, fo, loops=loops, quant=fq),
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
            lines.append("%-84s %s" % (name, med(t[name])))
    if args.spec_reps:
        checks = (("orient", hip.mesh_orient(verts, faces, policy="negative", adjacency=adj, quant=oq),
                   meshing.mesh_orient(verts, faces, policy="negative", quant=oq)),
                  ("loops", loops, meshing.mesh_boundary_loops(fo, V)),
                  ("fill", hip.mesh_fill_holes(verts, fo, loops=loops, quant=fq), meshing.mesh_fill_holes(verts, fo, loops=loops, quant=fq)))
        lines.append("kernels against the specification at this size: " +
                     ", ".join("%s %s" % (what, "bit-equal" if same(a, b) else "DIFFER") for what, a, b in checks))
        for what in ("adjacency", "orient ", "orient-vol", "loops", "fill"):
            k = statistics.median(next(v for n, v in t.items() if n.startswith(what) and "kernels" in n))
            s = statistics.median(next(v for n, v in t.items() if n.startswith(what) and "spec" in n))
            lines.append("%-10s specification / kernels = %.1f x" % (what.strip(), s / k))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-side", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--spec-reps", type=int, default=3)
    ap.add_argument("--holes", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from arah_release_amd import config, geometry, synthetic
    dev = torch.device("cuda:0")
    model, _ = config.build_synthetic_model("zju377_mono", device=dev)
    model.eval()
    inputs = synthetic.SyntheticScene(0).make_inputs(32, 32, frame_idx=0, device=dev)
    with torch.no_grad():
        posed = model.posed_mesh(inputs, n_side=args.n_side, indexed=True)
        verts, faces = posed["verts"].contiguous(), posed["faces"].contiguous()
        lines = ["%s, torch %s, HIP %s; measured %s by tools/mesh_repair_bench.py --n-side %d --reps %d --spec-reps %d --holes %d" % (
            torch.cuda.get_device_name(0), torch.__version__, torch.version.hip, datetime.date.today().isoformat(), args.n_side,
            args.reps, args.spec_reps, args.holes)]
        step = float((verts.amax(0) - verts.amin(0)).max()) / (args.n_side - 1)
        bench("posed level set at %d^3, 30 %% of the faces reversed, %d stars removed" % (args.n_side, args.holes), verts,
              damage(verts, faces, args.holes), args, lines)
        for k in (2, 4):
            simple = geometry.simplify_mesh(verts, faces, cell=k * step)
            bench("the same simplified with cells of %d / %d of its longest side, then 30 %% reversed, %d stars removed" % (
                k, args.n_side - 1, args.holes), simple["verts"],
                  damage(simple["verts"], simple["faces"], args.holes), args, lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
