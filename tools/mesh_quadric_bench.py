"""Cost and effect of quadric-error placement and of face-count targets (hip.mesh_quadric_place; geometry.simplify_mesh with
position="quadric" / target_faces=N).

    python tools/mesh_quadric_bench.py [--n-side 256] [--reps 20] [--out profiles/mesh_quadric_bench.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/mesh_quadric_bench.py --reps 5       # per kernel

The synthetic subject's posed level set at n_side^3 as an indexed mesh, clustered with cells of 2 and of 4 lattice steps.  For
each cell, after a warm-up of every route at this size, with device events around whole calls and the routes alternated in one
loop: median time of the clustering alone (hip.mesh_simplify: the yardstick), of the placement stage alone over its results
(hip.mesh_quadric_place), and of the public call for the three positions; then Chamfer-L1 (geometry.mesh_metrics) and the
signed-volume ratio of each result against the input mesh.  Last, simplify_mesh(target_faces=10000 / 2000): time, probes and the
resolution found.  The placement is compared with its specification for equality while at it, at this size."""
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from arah_release_amd import config, geometry, hip, meshing, synthetic
    dev = torch.device("cuda:0")
    model, _ = config.build_synthetic_model("zju377_mono", device=dev)
    model.eval()
    inputs = synthetic.SyntheticScene(0).make_inputs(32, 32, frame_idx=0, device=dev)
    lines = ["%s, torch %s, HIP %s; measured %s by tools/mesh_quadric_bench.py --n-side %d --reps %d" % (
        torch.cuda.get_device_name(0), torch.__version__, torch.version.hip, datetime.date.today().isoformat(), args.n_side, args.reps)]
    with torch.no_grad():
        posed = model.posed_mesh(inputs, n_side=args.n_side, indexed=True)
        verts, faces = posed["verts"].contiguous(), posed["faces"].contiguous()
        V, F = int(verts.shape[0]), int(faces.shape[0])
        lo, hi = verts.amin(0).tolist(), verts.amax(0).tolist()
        step = float(posed["box"][3]) / (args.n_side - 1)
        vol0 = volume(verts, faces)
        lines.append("posed level set at %d^3: %d vertices, %d faces, lattice step %.5f m, signed volume %.6f m^3" % (
            args.n_side, V, F, step, vol0))
        for k in (2, 4):
            cell = k * step
            origin, dims = geometry.simplify_grid_of(lo, hi, cell)
            grid = (origin.tolist(), cell, dims)
            means, _, vert_map, _, _, counts = hip.mesh_simplify(verts, faces, *grid)
            qc = hip.mesh_quadric_place(verts, faces, vert_map, means, counts, cell)[2].tolist()
            lines.append("")
            lines.append("cell = %d lattice steps (%.5f m), grid %s: %d clusters, %d kept faces; %d (face, cluster) pairs, longest "
                         "segment %d, %d fall-backs, status %d" % (k, cell, dims, int(counts[0]), int(counts[1]), qc[1], qc[2], qc[0],
                                                                  qc[3]))
            routes = {
                "cluster  kernels  hip.mesh_simplify (the yardstick)": lambda: hip.mesh_simplify(verts, faces, *grid),
                "place    kernels  hip.mesh_quadric_place": lambda: hip.mesh_quadric_place(verts, faces, vert_map, means, counts, cell),
                "simplify public   geometry.simplify_mesh(position='mean')": lambda: geometry.simplify_mesh(verts, faces, cell=cell),
                "simplify public   geometry.simplify_mesh(position='member')":
                    lambda: geometry.simplify_mesh(verts, faces, cell=cell, position="member"),
                "simplify public   geometry.simplify_mesh(position='quadric')":
                    lambda: geometry.simplify_mesh(verts, faces, cell=cell, position="quadric"),
            }
            for _ in range(3):                                                    # warm-up: every route, at this size
                for fn in routes.values():
                    fn()
            torch.cuda.synchronize()
            t = {name: [] for name in routes}
            for _ in range(args.reps):                                            # alternating
                for name, fn in routes.items():
                    t[name].append(timed(fn)[0])
            for name in routes:
                lines.append("%-72s %s" % (name, med(t[name])))
            ratio = statistics.median(t["place    kernels  hip.mesh_quadric_place"]) / statistics.median(
                t["cluster  kernels  hip.mesh_simplify (the yardstick)"])
            lines.append("placement / clustering = %.2f x" % ratio)
            got = hip.mesh_quadric_place(verts, faces, vert_map, means, counts, cell)
            want = meshing.mesh_quadric_place(verts, faces, vert_map, means, counts, cell)
            lines.append("kernels against the specification at this size: %s" % (
                "bit-equal" if all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got, want)) else "DIFFER"))
            for position in ("mean", "member", "quadric"):
                res = geometry.simplify_mesh(verts, faces, cell=cell, position=position)
                m = geometry.mesh_metrics((res["verts"], res["faces"]), (verts, faces), n_samples=200000)
                lines.append("%-8s %6d vertices %6d faces: chamfer-L1 %.4e m, accuracy %.4e, completeness %.4e, volume / input's %.5f" % (
                    position, res["n_verts"], res["n_tris"], float(m["chamfer_l1"]), float(m["accuracy"]), float(m["completeness"]),
                    volume(res["verts"], res["faces"]) / vol0))
        lines.append("")
        for target in (10000, 2000):
            for position in ("mean", "quadric"):
                fn = lambda: geometry.simplify_mesh(verts, faces, target_faces=target, position=position)
                fn()
                times = [timed(fn)[0] for _ in range(max(args.reps // 4, 3))]
                res = fn()
                lines.append("target_faces=%5d position=%-7s -> resolution %3d, %5d faces, %2d probes, reached %s: %s" % (
                    target, position, res["resolution"], res["n_tris"], len(res["probes"]), res["reached"], med(times)))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
