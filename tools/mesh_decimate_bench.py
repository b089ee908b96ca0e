"""Cost and effect of edge-collapse decimation (hip.mesh_collapse_round; geometry.decimate_mesh) next to vertex clustering at the
same face counts.

    python tools/mesh_decimate_bench.py [--n-side 256] [--reps 5] [--out profiles/mesh_decimate_bench.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/mesh_decimate_bench.py --reps 1      # per kernel

The synthetic subject's posed level set at n_side^3 as an indexed mesh.  Targets: the face counts that
simplify_mesh(position="quadric") reaches with cells of 2 and of 4 lattice steps, and 10000 and 2000 faces.  For each target, after a warm-up of both routes at this size, with device events around whole calls and
the two routes alternated in one loop: median time of geometry.decimate_mesh(target_faces=N) and of the clustering that gives
the same count (a cell, or target_faces=N with position="quadric"); the rounds; then for both results Chamfer-L1
(geometry.mesh_metrics) and the signed-volume ratio against the input, geometry.mesh_topology and
geometry.self_intersections().count.  One round alone (hip.mesh_collapse_round, next to hip.mesh_adjacency, which it contains)
is timed first and compared with its specification for equality at this size."""
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


def volume(verts, faces):
    tri = verts.double()[faces.long()]
    return float((tri[:, 0] * torch.linalg.cross(tri[:, 1], tri[:, 2])).sum() / 6)


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
    lines = ["%s, torch %s, HIP %s; measured %s in one session by tools/mesh_decimate_bench.py --n-side %d --reps %d" % (
        torch.cuda.get_device_name(0), torch.__version__, torch.version.hip, datetime.date.today().isoformat(), args.n_side, args.reps)]

    def score(name, res, verts, faces, vol0):
        m = geometry.mesh_metrics((res["verts"], res["faces"]), (verts, faces), n_samples=200000)
        topo = geometry.mesh_topology(res["verts"], res["faces"])
        hits = geometry.self_intersections(res["verts"], res["faces"], return_pairs=False)["count"]
        return ("%-9s %6d vertices %6d faces: chamfer-L1 %.4e m, volume / input's %.5f; manifold %s, watertight %s, euler %d, "
                "boundary %d, non-manifold %d edges, max valence %d; %d self-intersecting pairs" % (
                    name, res["n_verts"], res["n_tris"], float(m["chamfer_l1"]), volume(res["verts"], res["faces"]) / vol0,
                    topo["manifold"], topo["watertight"], topo["euler"], topo["boundary_edges"], topo["nonmanifold_edges"],
                    topo["max_valence"], hits))

    with torch.no_grad():
        posed = model.posed_mesh(inputs, n_side=args.n_side, indexed=True)
        verts, faces = posed["verts"].contiguous(), posed["faces"].contiguous()
        V, F = int(verts.shape[0]), int(faces.shape[0])
        step = float(posed["box"][3]) / (args.n_side - 1)
        vol0 = volume(verts, faces)
        topo = geometry.mesh_topology(verts, faces)
        lines.append("posed level set at %d^3: %d vertices, %d faces, lattice step %.5f m, signed volume %.6f m^3; "
                     "manifold %s, watertight %s, euler %d" % (args.n_side, V, F, step, vol0, topo["manifold"], topo["watertight"],
                                                               topo["euler"]))
        routes = {"adjacency  hip.mesh_adjacency (inside every round)": lambda: hip.mesh_adjacency(faces, V),
                  "round      hip.mesh_collapse_round": lambda: hip.mesh_collapse_round(verts, faces, F)}
        for _ in range(3):
            for fn in routes.values():
                fn()
        t = {name: [] for name in routes}
        for _ in range(max(args.reps, 5)):
            for name, fn in routes.items():
                t[name].append(timed(fn)[0])
        for name in routes:
            lines.append("%-52s %s" % (name, med(t[name])))
        got = hip.mesh_collapse_round(verts, faces, F, details=True)
        want = meshing.mesh_collapse_round(verts.cpu(), faces.cpu(), F, details=True)
        same = all(torch.equal(a.cpu().view(torch.uint8), b.view(torch.uint8)) for a, b in zip(got, want))
        c = dict(zip(meshing.COLLAPSE_COUNTS, got[4].tolist()))
        n_edges = sum(c[k] for k in meshing.COLLAPSE_COUNTS[4:11])
        lines.append("the first round: %s; %d of %d edges selected (one in %.1f), %.1f %% of the faces go; against the specification at "
                     "this size: %s" % (c, c["selected"], n_edges, n_edges / max(c["selected"], 1), 200.0 * c["selected"] / F,
                                        "bit-equal" if same else "DIFFER"))
        targets = []
        for k in (2, 4):
            res = geometry.simplify_mesh(verts, faces, cell=k * step, position="quadric")
            targets.append(("cell of %d lattice steps" % k, res["n_tris"], {"cell": k * step, "position": "quadric"}))
        targets += [("target_faces", n, {"target_faces": n, "position": "quadric"}) for n in (10000, 2000)]
        for what, n, how in targets:
            lines.append("")
            lines.append("%d faces (%s)" % (n, what))
            both = {"collapse": lambda: geometry.decimate_mesh(verts, faces, target_faces=n),
                    "cluster": lambda: geometry.simplify_mesh(verts, faces, **how)}
            for fn in both.values():
                fn()
            t = {name: [] for name in both}
            for _ in range(args.reps):
                for name, fn in both.items():
                    t[name].append(timed(fn)[0])
            out = {name: fn() for name, fn in both.items()}
            rep = out["collapse"]["report"]
            lines.append("collapse  geometry.decimate_mesh(target_faces=%d): %s; %d rounds, reached %s, %s" % (
                n, med(t["collapse"]), rep["rounds"], rep["reached"], {k: rep[k] for k in ("pinned", "link", "long_edges", "flips",
                                                                                             "fallbacks")}))
            lines.append("cluster   geometry.simplify_mesh(%s): %s" % (", ".join("%s=%r" % kv for kv in how.items()), med(t["cluster"])))
            for name in both:
                lines.append(score(name, out[name], verts, faces, vol0))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
