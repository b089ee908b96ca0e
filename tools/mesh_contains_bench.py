"""Cost of point-in-mesh against large meshes (hip.contains_index / hip.mesh_contains / hip.mesh_contains_grid; geometry.voxelize).

    python tools/mesh_contains_bench.py [--n-side 256] [--reps 11] [--points 100000,1000000,10000000] [--resolutions 512]
                                        [--out profiles/mesh_contains_bench.txt]

The synthetic subject's posed level set at `--n-side`^3 as an indexed mesh and its simplified meshes (geometry.simplify_mesh at 128
and 64 cells along the longest side); uniform float32 points in the mesh's box widened by 5 %; a `--n-side`^3 voxelize.  Whole calls:
the index build is timed on the host around a synchronised call (it contains the one read-back), the queries with device events after
warm-up; medians of `--reps` calls, the routes alternating in one loop.  Reported per mesh and resolution: references, candidates per
point (mean, max), the share of ambiguous points; hip.mesh_query (the brute force of the training samplers) and the specification
meshing.mesh_contains on the same tensors where they finish in seconds; and, for the unsimplified mesh, how often `inside` disagrees
with the sign of model.query_posed's SDF as a function of |sdf| in lattice steps."""
import argparse
import os
import statistics
import sys
import time

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


def host_timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def med(v):
    return "median %.3f ms (min %.3f, max %.3f, %d calls)" % (statistics.median(v), min(v), max(v), len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-side", type=int, default=256)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--points", type=str, default="100000,1000000,10000000")
    ap.add_argument("--resolutions", type=str, default="512")
    ap.add_argument("--brute-pairs", type=float, default=2.5e10, help="hip.mesh_query runs where points x faces stays below this")
    ap.add_argument("--spec-pairs", type=float, default=2.5e10, help="... and the specification")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from arah_release_amd import config, geometry, hip, meshing, synthetic
    dev = torch.device("cuda:0")
    model, _ = config.build_synthetic_model("zju377_mono", 64, 16, 16, device=dev)
    model.eval()
    inputs = synthetic.SyntheticScene(0).make_inputs(32, 32, frame_idx=0, device=dev)
    with torch.no_grad():
        full = model.posed_mesh(dict(inputs), n_side=args.n_side, indexed=True)
    meshes = [("posed %d^3" % args.n_side, full["verts"].contiguous(), full["faces"].contiguous())]
    for cells in (128, 64):
        s = geometry.simplify_mesh(full["verts"], full["faces"], resolution=cells)
        meshes.append(("simplified %d" % cells, s["verts"].contiguous(), s["faces"].to(torch.int32).contiguous()))
    lo, hi = full["verts"].double().amin(0), full["verts"].double().amax(0)
    lo, hi = lo - 0.05 * (hi - lo), hi + 0.05 * (hi - lo)
    counts = [int(x) for x in args.points.split(",")]
    gen = torch.Generator(device=dev).manual_seed(0)
    clouds = {n: (lo + torch.rand(n, 3, dtype=torch.float64, device=dev, generator=gen) * (hi - lo)).float().contiguous() for n in counts}
    lines = ["mesh_contains_bench: %s, torch %s, n_side %d, %d reps, points uniform in the posed mesh's box + 5 %%" % (
        torch.cuda.get_device_name(0), torch.__version__, args.n_side, args.reps)]
    for name, verts, faces in meshes:
        F = int(faces.shape[0])
        for res in (int(r) for r in args.resolutions.split(",")):
            hip.contains_index(verts, faces, res)                                                    # warm-up
            build = []
            for _ in range(args.reps):
                ms, index = host_timed(lambda: hip.contains_index(verts, faces, res))
                build.append(ms)
            head = hip._contains_header(index.buf)
            lines.append("")
            lines.append("%s: %d vertices, %d faces; resolution %d: %d references (%.2f a face), %d faces on the workgroup list, %d on the "
                         "several-workgroups list, index %.1f MB + references %.1f MB" % (
                             name, verts.shape[0], F, res, index.n_refs, index.n_refs / max(F, 1), head["n_med"], head["n_huge"],
                             index.buf.numel() / 2 ** 20, index.n_refs * 4 / 2 ** 20))
            lines.append("  index build (count, read-back, fill; host-timed)   %s" % med(build))
            for n in counts:
                pts = clouds[n]
                inside, ambiguous, tested = hip.mesh_contains(index, pts, True, True)               # warm-up, and the figures
                brute_ok, spec_ok = float(n) * F <= args.brute_pairs, float(n) * F <= args.spec_pairs
                t_q, t_b, t_s = [], [], []
                if brute_ok:
                    hip.mesh_query(verts, faces, pts[:1024])
                for rep in range(args.reps):
                    t_q.append(timed(lambda: hip.mesh_contains(index, pts))[0])
                    if brute_ok and rep < 3:
                        ms, out = timed(lambda: hip.mesh_query(verts, faces, pts))
                        t_b.append(ms)
                        brute_inside = out[4]
                    if spec_ok and rep < 2:
                        ms, out = timed(lambda: meshing.mesh_contains(verts, faces, pts, res))
                        t_s.append(ms)
                        spec_inside = out[0]
                lines.append("  %9d points: query %s; inside %.4f, ambiguous %.2e of the points; candidates per point mean %.2f max %d" % (
                    n, med(t_q), float(inside.double().mean()), float(ambiguous.double().mean()), float(tested.double().mean()),
                    int(tested.max())))
                if t_b:
                    lines.append("             hip.mesh_query (brute force, closest point too) %s; build + query is %.1f x faster; inside differs "
                                 "at %d points" % (med(t_b), statistics.median(t_b) / (statistics.median(build) + statistics.median(t_q)),
                                                   int((brute_inside != inside).sum())))
                if t_s:
                    lines.append("             the specification on the same tensors %s; inside differs at %d points" % (
                        med(t_s), int((spec_inside != inside).sum())))
            if name.startswith("posed"):
                dims = (args.n_side,) * 3
                geometry.voxelize((verts, faces), dims=dims, hash_resolution=res, index=index, bounds=(lo.tolist(), hi.tolist()))
                t_v, t_p = [], []
                for _ in range(args.reps):
                    ms, vox = timed(lambda: geometry.voxelize((verts, faces), dims=dims, hash_resolution=res, index=index,
                                                              bounds=(lo.tolist(), hi.tolist())))
                    t_v.append(ms)
                grid = torch.stack(torch.meshgrid(vox["xs"], vox["ys"], vox["zs"], indexing="ij"), dim=-1).reshape(-1, 3).contiguous()
                for _ in range(3):
                    ms, out = timed(lambda: hip.mesh_contains(index, grid))
                    t_p.append(ms)
                lines.append("  voxelize %d^3 (index given): %s; occupied %.4f, ambiguous %d; the point kernel on the same %d points %s, "
                             "differs at %d" % (args.n_side, med(t_v), float(vox["occupancy"].double().mean()), int(vox["ambiguous"]),
                                                grid.shape[0], med(t_p), int((out[0] != vox["occupancy"].reshape(-1)).sum())))
    # inside against the sign of the posed SDF, by |sdf| in lattice steps (a reported figure, not a test)
    name, verts, faces = meshes[0]
    res = int(args.resolutions.split(",")[0])
    index = hip.contains_index(verts, faces, res)
    n = min(counts)
    pts = clouds[n]
    with torch.no_grad():
        q = model.query_posed(dict(inputs), pts)
    inside = hip.mesh_contains(index, pts)[0]
    step = float(full["box"][3]) / (args.n_side - 1) if full.get("box") is not None else float((hi - lo).max()) / (args.n_side - 1)
    sdf, ok = q["sdf"].double(), q["converged"]
    lines.append("")
    lines.append("inside(%s) against sdf < 0 of model.query_posed at %d points (%d converged; lattice step %.5f m):" % (name, n, int(ok.sum()), step))
    edges = [0.0, 0.25, 0.5, 1.0, 2.0, 4.0, float("inf")]
    for a, b in zip(edges[:-1], edges[1:]):
        sel = ok & (sdf.abs() >= a * step) & (sdf.abs() < b * step)
        bad = sel & (inside != (sdf < 0))
        lines.append("  |sdf| in [%.2f, %.2f) steps: %8d points, %6d disagree (%.4f)" % (a, b, int(sel.sum()), int(bad.sum()),
                                                                                      int(bad.sum()) / max(int(sel.sum()), 1)))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
