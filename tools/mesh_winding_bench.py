"""Cost and error of generalized winding numbers on the device (hip.winding_index / hip.mesh_winding / hip.mesh_winding_grid).

    python tools/mesh_winding_bench.py [--n-side 256] [--reps 7] [--points 100000,1000000,10000000] [--depths 3,4,5,6,7]
                                       [--exact-pairs 3e10] [--out profiles/mesh_winding_bench.txt]

The synthetic subject's posed level set at `--n-side`^3 as an indexed mesh and its simplified meshes (geometry.simplify_mesh at 128
and 64 cells along the longest side); uniform float32 points in the mesh's box widened by 5 %; a `--n-side`^3 lattice of cell centres
in the same box.  Whole calls: the index build is timed on the host around a synchronised call (it contains the one read-back), the
queries with device events after warm-up; medians of `--reps` calls, the routes alternating in one loop; the clocks before and after.
Reported per mesh: the tree (depth, nodes, largest leaf), the build, per point count and accuracy (2, 3) the query, mean n_exact and
n_far per point, and -- where points x faces stays below `--exact-pairs` -- the accuracy = inf route (the exact sum) and max |w -
w(inf)|; the parity route (hip.contains_index + hip.mesh_contains at resolution 512) alongside; a sweep of `depth` at the smallest
point count; the lattice through hip.mesh_winding_grid and hip.mesh_contains_grid."""
import argparse
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
INF = float("inf")


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


class Lines(list):
    """The report; every line is printed as it is found."""

    def append(self, line):
        print(line, flush=True)
        list.append(self, line)


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=60).stdout
        keep = [" ".join(l.split()) for l in out.splitlines() if "GPU[0]" in l and ("sclk" in l or "mclk" in l)]
        return "; ".join(keep) if keep else "clocks: rocm-smi printed none"
    except Exception as e:   # the figure is a note, not a requirement
        return "clocks: not available (%s)" % type(e).__name__


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-side", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--points", type=str, default="100000,1000000,10000000")
    ap.add_argument("--depths", type=str, default="3,4,5,6,7")
    ap.add_argument("--exact-pairs", type=float, default=3e10, help="accuracy = inf runs where points x faces stays below this")
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
    axes = geometry._cell_centres(lo.cpu(), (hi - lo).cpu(), (args.n_side,) * 3, dev)
    lines = Lines()
    lines.append("mesh_winding_bench: %s, torch %s, n_side %d, %d reps, points uniform in the posed mesh's box + 5 %%; accuracy = inf where "
                 "points x faces <= %.1e" % (torch.cuda.get_device_name(0), torch.__version__, args.n_side, args.reps, args.exact_pairs))
    lines.append("before: " + clocks())
    for name, verts, faces in meshes:
        F = int(faces.shape[0])
        hip.winding_index(verts, faces)                                                              # warm-up
        build, build_c = [], []
        for _ in range(args.reps):
            ms, index = host_timed(lambda: hip.winding_index(verts, faces))
            build.append(ms)
            ms, cindex = host_timed(lambda: hip.contains_index(verts, faces, 512))
            build_c.append(ms)
        leaf = index.node_i[index.node_i[:, 2] == index.depth, 1]
        lines.append("")
        lines.append("%s: %d vertices, %d faces, orient %+d; depth %d (the rule of depth=None): %d nodes, %d leaves, largest leaf %d, mean "
                     "%.1f; tables %.1f MB" % (name, verts.shape[0], F, index.orient, index.depth, index.n_nodes, leaf.numel(), int(leaf.max()),
                                               float(leaf.double().mean()),
                                               (index.node_i.numel() * 4 + index.node_f.numel() * 8 + index.tris.numel() * 4) / 2 ** 20))
        lines.append("  index build (count, read-back, fill; host-timed)   %s" % med(build))
        lines.append("  parity route: hip.contains_index at 512            %s" % med(build_c))
        for n in counts:
            pts = clouds[n]
            exact_ok = float(n) * F <= args.exact_pairs
            w_inf = hip.mesh_winding(index, pts, INF)[0] if exact_ok else None
            t = {2.0: [], 3.0: [], INF: [], "parity": []}
            hip.mesh_contains(cindex, pts)
            out = {a: hip.mesh_winding(index, pts, a, want_counts=True) for a in (2.0, 3.0)}
            for rep in range(args.reps):
                for a in (2.0, 3.0):
                    t[a].append(timed(lambda: hip.mesh_winding(index, pts, a))[0])
                t["parity"].append(timed(lambda: hip.mesh_contains(cindex, pts))[0])
                if exact_ok and rep < 3:
                    t[INF].append(timed(lambda: hip.mesh_winding(index, pts, INF))[0])
            parity_in = hip.mesh_contains(cindex, pts)[0]
            lines.append("  %9d points: parity route hip.mesh_contains %s" % (n, med(t["parity"])))
            for a in (2.0, 3.0):
                w, inside, n_exact, n_far = out[a]
                err = "max |w - w(inf)| %.4f" % float((w - w_inf).abs().max()) if exact_ok else "w(inf) not run"
                lines.append("             accuracy %g: %s; n_exact mean %.1f, n_far mean %.1f; %s; inside differs from parity at %d points"
                             % (a, med(t[a]), float(n_exact.double().mean()), float(n_far.double().mean()), err,
                                int((inside != parity_in).sum())))
            if exact_ok:
                inside_inf = meshing.winding_inside(w_inf, index.orient)
                lines.append("             accuracy inf (the exact sum, %d terms a point): %s; inside differs from parity at %d points"
                             % (F, med(t[INF]), int((inside_inf != parity_in).sum())))
        # the depth of the tree, at the smallest point count and accuracy 3
        n = min(counts)
        pts = clouds[n]
        for depth in (int(d) for d in args.depths.split(",")):
            ms_b, ix = host_timed(lambda: hip.winding_index(verts, faces, depth))
            hip.mesh_winding(ix, pts, 3.0)
            tq = [timed(lambda: hip.mesh_winding(ix, pts, 3.0))[0] for _ in range(args.reps)]
            _, _, n_exact, n_far = hip.mesh_winding(ix, pts, 3.0, want_counts=True)
            lines.append("  depth %d%s: %d nodes, build %.3f ms (one call); %d points at accuracy 3: %s; n_exact mean %.1f, n_far mean %.1f"
                         % (depth, " (auto)" if depth == index.depth else "", ix.n_nodes, ms_b, n, med(tq), float(n_exact.double().mean()),
                            float(n_far.double().mean())))
        # the lattice
        hip.mesh_winding_grid(index, *axes, 3.0)
        hip.mesh_contains_grid(cindex, *axes)
        tg = {2.0: [], 3.0: [], "parity": []}
        for rep in range(min(args.reps, 5)):
            for a in (2.0, 3.0):
                ms, res = timed(lambda: hip.mesh_winding_grid(index, *axes, a))
                tg[a].append(ms)
                if a == 3.0:
                    occ = res[1]
            ms, (occ_p, amb) = timed(lambda: hip.mesh_contains_grid(cindex, *axes))
            tg["parity"].append(ms)
        lines.append("  %d^3 lattice: hip.mesh_winding_grid accuracy 2 %s; accuracy 3 %s; occupied %.4f" % (
            args.n_side, med(tg[2.0]), med(tg[3.0]), float(occ.double().mean())))
        lines.append("                hip.mesh_contains_grid (parity) %s; occupied %.4f, ambiguous %d; winding (accuracy 3) differs at %d nodes"
                     % (med(tg["parity"]), float(occ_p.double().mean()), int(amb), int((occ != occ_p).sum())))
    lines.append("")
    lines.append("after: " + clocks())
    lines.append("not measured: other rules for depth=None than meshing.winding_depth (the sweep above is the evidence for it), other "
                 "thread mappings than one lane per point, accuracy = inf on the larger point counts and on the lattice.")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
