"""Cost and effect of edge flips and isotropic remeshing (hip.mesh_flip_round; geometry.flip_edges, geometry.isotropic_remesh).

    python tools/mesh_isotropic_bench.py [--n-side 256] [--reps 5] [--out profiles/mesh_isotropic_bench.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/mesh_isotropic_bench.py --reps 1      # per kernel

The synthetic subject's posed level set at n_side^3 as an indexed mesh (its largest component).  After a warm-up of every route
at its size, with device events around whole calls and the routes alternated in one loop: median time of one flip round of
either criterion (hip.mesh_flip_round), of hip.mesh_adjacency alone (every round contains it: its share), and of the specification
meshing.mesh_flip_round on the same GPU tensors, every kernel result compared with the specification for equality at its size.
Then geometry.flip_edges to convergence for both criteria (rounds, flips, time); geometry.isotropic_remesh at a target of one
and of two lattice steps, end to end, with the reads of counts on the host counted; geometry.mesh_quality of the input and of every
result against the same target, and the Chamfer-L1 to the input (geometry.mesh_metrics); and the same quality table for
geometry.remesh at n_side^3 and geometry.decimate_mesh(target_faces=10000), the routes that existed before."""
import argparse
import datetime
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
QUALITY = ("n_faces", "edge_min", "edge_mean", "edge_max", "edges_in_range", "min_angle_min", "min_angle_mean", "small_angle_share",
           "valence6_share", "valence5to7_share")


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def med(v):
    return "median %.3f ms (min %.3f, max %.3f, %d calls)" % (statistics.median(v), min(v), max(v), len(v))


class HostReads:
    """Counts the Tensor.tolist() calls made inside the block: the loops read their counts that way, once per round."""

    def __enter__(self):
        self.n, self.old = 0, torch.Tensor.tolist
        outer = self

        def tolist(t):
            outer.n += 1
            return outer.old(t)
        torch.Tensor.tolist = tolist
        return self

    def __exit__(self, *exc):
        torch.Tensor.tolist = self.old


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
    lines = ["%s, torch %s, HIP %s; measured %s in one session by tools/mesh_isotropic_bench.py --n-side %d --reps %d" % (
        torch.cuda.get_device_name(0), torch.__version__, torch.version.hip, datetime.date.today().isoformat(), args.n_side, args.reps)]

    def same(got, want):
        return "bit-equal" if all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(got, want)) else "DIFFER"

    def table(name, verts, faces, L, ref=None):
        q = geometry.mesh_quality(verts, faces, L)
        row = "%-44s " % name + "  ".join("%s %.4g" % (k, q[k]) for k in QUALITY)
        if ref is not None:
            m = geometry.mesh_metrics((verts, faces), ref, n_samples=200000)
            row += "  chamfer-L1 to the input %.4e m" % float(m["chamfer_l1"])
        topo = geometry.mesh_topology(verts, faces)
        return row + "  watertight %s, euler %d" % (topo["watertight"], topo["euler"])

    with torch.no_grad():
        posed = model.posed_mesh(inputs, n_side=args.n_side, indexed=True, clean="largest")
        verts, faces = posed["verts"].contiguous(), posed["faces"].contiguous()
        V, F = int(verts.shape[0]), int(faces.shape[0])
        step = float(posed["box"][3]) / (args.n_side - 1)
        lines.append("posed level set at %d^3, largest component: %d vertices, %d faces, lattice step %.5f m" % (args.n_side, V, F, step))
        routes = {"adjacency  hip.mesh_adjacency (inside every round)": lambda: hip.mesh_adjacency(faces, V)}
        for crit in ("delaunay", "valence"):
            routes["%-10s hip.mesh_flip_round" % crit] = lambda c=crit: hip.mesh_flip_round(verts, faces, c, 0, details=True)
            routes["%-10s meshing.mesh_flip_round, same tensors" % crit] = lambda c=crit: meshing.mesh_flip_round(verts, faces, c, 0,
                                                                                                             details=True)
        for _ in range(2):
            for fn in routes.values():
                fn()
        t = {name: [] for name in routes}
        for _ in range(args.reps):
            for name, fn in routes.items():
                t[name].append(timed(fn)[0])
        lines.append("")
        lines.append("one flip round, salt 0")
        for name in routes:
            lines.append("%-56s %s" % (name, med(t[name])))
        adj = statistics.median(t["adjacency  hip.mesh_adjacency (inside every round)"])
        for crit in ("delaunay", "valence"):
            got, want = hip.mesh_flip_round(verts, faces, crit, 0, details=True), meshing.mesh_flip_round(verts, faces, crit, 0, details=True)
            k = statistics.median(t["%-10s hip.mesh_flip_round" % crit])
            s = statistics.median(t["%-10s meshing.mesh_flip_round, same tensors" % crit])
            lines.append("%-10s the adjacency build is %.0f %% of the round; the specification takes %.1f times the kernels' time; against "
                         "it at this size: %s; %s" % (crit, 100.0 * adj / k, s / k, same(got, want[:5]),
                                                      dict(zip(meshing.FLIP_COUNTS, got[2].tolist()))))
        lines.append("")
        lines.append("geometry.flip_edges to convergence (max_rounds=64)")
        for crit in ("delaunay", "valence"):
            geometry.flip_edges(verts, faces, crit)
            tt = []
            for _ in range(args.reps):
                ms, res = timed(lambda: geometry.flip_edges(verts, faces, crit))
                tt.append(ms)
            lines.append("%-10s %s; %d rounds, converged %s, %d flips; candidates per round %s" % (
                crit, med(tt), res["rounds"], res["converged"], res["flips"], res["candidates"]))
            lines.append(table("  after flip_edges(%s)" % crit, verts, res["faces"], step))
        lines.append("")
        lines.append("geometry.isotropic_remesh(iterations=5), end to end; quality against the target edge length L of each row")
        for mult in (1, 2):
            L = mult * step
            geometry.isotropic_remesh(verts, faces, edge_length=L)
            tt = []
            for _ in range(max(1, args.reps // 2)):
                with HostReads() as reads:
                    ms, res = timed(lambda: geometry.isotropic_remesh(verts, faces, edge_length=L))
                tt.append(ms)
            lines.append("L = %d lattice steps: %s; %d reads of counts on the host; per iteration %s" % (
                mult, med(tt), reads.n, res["report"]["iterations"]))
            lines.append(table("  input", verts, faces, L))
            lines.append(table("  isotropic_remesh", res["verts"], res["faces"], L, ref=(verts, faces)))
        lines.append("")
        lines.append("the routes that existed before, quality against L = one lattice step (remesh) and against their own mean edge")
        again = geometry.remesh((verts, faces), n_side=args.n_side)
        lines.append(table("  geometry.remesh(n_side=%d)" % args.n_side, again[0], again[1], step, ref=(verts, faces)))
        small = geometry.decimate_mesh(verts, faces, target_faces=10000)
        lines.append(table("  geometry.decimate_mesh(target_faces=10000)", small["verts"], small["faces"], None, ref=(verts, faces)))
        L = geometry.mesh_quality(small["verts"], small["faces"])["edge_mean"]
        res = geometry.isotropic_remesh(verts, faces, edge_length=L)
        lines.append(table("  isotropic_remesh at that mean edge length", res["verts"], res["faces"], L, ref=(verts, faces)))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
