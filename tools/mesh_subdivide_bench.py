"""Cost and effect of subdivision (hip.mesh_subdivide_round; geometry.subdivide_mesh).

    python tools/mesh_subdivide_bench.py [--n-side 256] [--reps 5] [--out profiles/mesh_subdivide_bench.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/mesh_subdivide_bench.py --reps 1      # per kernel

The synthetic subject's posed level set at n_side^3 as an indexed mesh.  After a warm-up of every route at its size, with
device events around whole calls and the routes alternated in one loop: median time of one uniform midpoint round and one Loop
round (hip.mesh_subdivide_round), of hip.mesh_adjacency alone (every round contains it: its share), of the specification
meshing.mesh_subdivide_round on the same GPU tensors, and of a second round on the first one's result; every kernel result is
compared with the specification for equality at its size.  Then geometry.decimate_mesh(target_faces=2000) followed by two Loop
levels, by two midpoint levels and by max_edge = one lattice step: time of geometry.subdivide_mesh, Chamfer-L1 to the
undecimated mesh (geometry.mesh_metrics) and geometry.mesh_topology of each result."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-side", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from arah_release_amd import config, geometry, hip, meshing, synthetic
    dev = torch.device("cuda:0")
    model, _ = config.build_synthetic_model("zju377_mono", device=dev)
    model.eval()
    inputs = synthetic.SyntheticScene(0).make_inputs(32, 32, frame_idx=0, device=dev)
    lines = ["%s, torch %s, HIP %s; measured %s in one session by tools/mesh_subdivide_bench.py --n-side %d --reps %d" % (
        torch.cuda.get_device_name(0), torch.__version__, torch.version.hip, datetime.date.today().isoformat(), args.n_side, args.reps)]
    names = meshing.SUBDIVIDE_COUNTS

    def same(got, want):
        return "bit-equal" if all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(got, want)) else "DIFFER"

    def rounds(title, verts, faces):
        V, F = int(verts.shape[0]), int(faces.shape[0])
        routes = {"adjacency  hip.mesh_adjacency (inside every round)": lambda: hip.mesh_adjacency(faces, V),
                  "midpoint   hip.mesh_subdivide_round": lambda: hip.mesh_subdivide_round(verts, faces, "midpoint"),
                  "loop       hip.mesh_subdivide_round": lambda: hip.mesh_subdivide_round(verts, faces, "loop"),
                  "midpoint   meshing.mesh_subdivide_round, same tensors": lambda: meshing.mesh_subdivide_round(verts, faces, "midpoint"),
                  "loop       meshing.mesh_subdivide_round, same tensors": lambda: meshing.mesh_subdivide_round(verts, faces, "loop")}
        for _ in range(2):
            for fn in routes.values():
                fn()
        t = {name: [] for name in routes}
        for _ in range(args.reps):
            for name, fn in routes.items():
                t[name].append(timed(fn)[0])
        lines.append("")
        lines.append("%s: %d vertices, %d faces" % (title, V, F))
        for name in routes:
            lines.append("%-56s %s" % (name, med(t[name])))
        adj = statistics.median(t["adjacency  hip.mesh_adjacency (inside every round)"])
        out = {}
        for method in ("midpoint", "loop"):
            key = "%-10s hip.mesh_subdivide_round" % method
            spec_key = "%-10s meshing.mesh_subdivide_round, same tensors" % method
            got, want = hip.mesh_subdivide_round(verts, faces, method), meshing.mesh_subdivide_round(verts, faces, method)
            k, s = statistics.median(t[key]), statistics.median(t[spec_key])
            lines.append("%-10s the adjacency build is %.0f %% of the round; the specification takes %.1f times the kernels' time; "
                         "against it at this size: %s; %s" % (method, 100.0 * adj / k, s / k, same(got, want),
                                                              dict(zip(names, got[4].tolist()))))
            out[method] = got
        return out

    def score(name, res, t, verts, faces):
        m = geometry.mesh_metrics((res["verts"], res["faces"]), (verts, faces), n_samples=200000)
        topo = geometry.mesh_topology(res["verts"], res["faces"])
        rep = res["report"]
        return ("%-28s %s; %d rounds, reached %s, marked %s\n%-28s %6d vertices %6d faces: chamfer-L1 %.4e m; manifold %s, "
                "watertight %s, euler %d, boundary %d, non-manifold %d edges, max valence %d" % (
                    name, med(t), rep["rounds"], rep["reached"], rep["marked"], "", res["n_verts"], res["n_tris"],
                    float(m["chamfer_l1"]), topo["manifold"], topo["watertight"], topo["euler"], topo["boundary_edges"],
                    topo["nonmanifold_edges"], topo["max_valence"]))

    with torch.no_grad():
        posed = model.posed_mesh(inputs, n_side=args.n_side, indexed=True)
        verts, faces = posed["verts"].contiguous(), posed["faces"].contiguous()
        step = float(posed["box"][3]) / (args.n_side - 1)
        topo = geometry.mesh_topology(verts, faces)
        lines.append("posed level set at %d^3: %d vertices, %d faces, lattice step %.5f m; manifold %s, watertight %s, euler %d" % (
            args.n_side, verts.shape[0], faces.shape[0], step, topo["manifold"], topo["watertight"], topo["euler"]))
        first = rounds("first round", verts, faces)
        for method in ("midpoint", "loop"):
            c = dict(zip(names, first[method][4].tolist()))
            rounds("second round, after a %s round" % method, first[method][0][:c["n_verts"]].contiguous(),
                   first[method][1][:c["n_faces"]].contiguous())
        small = geometry.decimate_mesh(verts, faces, target_faces=2000)
        cage_v, cage_f = small["verts"].contiguous(), small["faces"].contiguous()
        m = geometry.mesh_metrics((cage_v, cage_f), (verts, faces), n_samples=200000)
        lines.append("")
        lines.append("geometry.decimate_mesh(target_faces=2000): %d vertices, %d faces, chamfer-L1 %.4e m to the undecimated mesh; then"
                     % (small["n_verts"], small["n_tris"], float(m["chamfer_l1"])))
        ways = {"two Loop levels": {"levels": 2, "method": "loop"}, "two midpoint levels": {"levels": 2},
                "max_edge = one lattice step": {"max_edge": step, "max_rounds": 32}}
        for fn in ways.values():
            geometry.subdivide_mesh(cage_v, cage_f, **fn)
        t = {name: [] for name in ways}
        for _ in range(args.reps):
            for name, how in ways.items():
                t[name].append(timed(lambda: geometry.subdivide_mesh(cage_v, cage_f, **how))[0])
        for name, how in ways.items():
            lines.append(score(name, geometry.subdivide_mesh(cage_v, cage_f, **how), t[name], verts, faces))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
