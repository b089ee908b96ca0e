"""Cost of the exact nearest-point query over large clouds (hip.point_index / hip.point_nearest; geometry.mesh_metrics against a
scan).

    python tools/cloud_metrics_bench.py [--queries 100000] [--sizes 100000,1000000,5000000] [--reps 10] [--brute-reps 2]
                                        [--brute-queries 10000] [--no-kdtree] [--out profiles/cloud_metrics.txt]

Sheet-like clouds of the sizes a scan has: points on an ellipsoid of body proportions (semi-axes 0.3 x 0.2 x 0.9 m) with 1 mm of
noise, from a seeded generator.  The queries lie on the same surface moved by 5 mm of noise -- what the samples of a good
reconstruction look like to the index.  Per size, after warm-up, in wall time (host clock around calls that end in a device
synchronise), medians over --reps:

    the index build and the indexed query, alternated in one loop with
    the same query by chunked float64 brute force in torch on the device (--brute-reps; for clouds above 10^6 points on the
        first --brute-queries queries only, the time scaled to all of them and said so), and
    the same query by scipy.spatial.cKDTree on the host (float64 copies of the float32 points, 16 workers; build and query),

the grid, the measured dimension, mean and largest number of points per occupied cell, mean and largest number of point tests
per query, and whether the three routes agree on d2 and on the nearest index (ties aside)."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def med(v):
    return "median %.3f ms (min %.3f, max %.3f, %d calls)" % (statistics.median(v), min(v), max(v), len(v))


def sheet(n, gen, dev, noise):
    d = torch.randn(n, 3, device=dev, generator=gen)
    d = d / d.norm(dim=1, keepdim=True)
    p = d * torch.tensor([0.3, 0.2, 0.9], device=dev) + torch.randn(n, 3, device=dev, generator=gen) * noise
    return p.float().contiguous()


def brute(cloud, pts, budget=1 << 28):
    """Float64 brute force in chunks of queries: (d2, the lowest index at the minimum)."""
    cx, cy, cz = (cloud[:, k].double().contiguous() for k in range(3))
    step = max(1, budget // cloud.shape[0])
    d2 = torch.empty(pts.shape[0], dtype=torch.float64, device=pts.device)
    idx = torch.empty(pts.shape[0], dtype=torch.int64, device=pts.device)
    for s in range(0, pts.shape[0], step):
        q = pts[s:s + step].double()
        dx, dy, dz = q[:, 0:1] - cx[None], q[:, 1:2] - cy[None], q[:, 2:3] - cz[None]
        m = (dx * dx + dy * dy) + dz * dz
        best, arg = m.min(1)
        d2[s:s + step], idx[s:s + step] = best, arg
    return d2, idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=100000)
    ap.add_argument("--sizes", default="100000,1000000,5000000")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--brute-reps", type=int, default=2)
    ap.add_argument("--brute-queries", type=int, default=10000)
    ap.add_argument("--no-kdtree", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from arah_release_amd import hip
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    pts = sheet(args.queries, gen, dev, 5e-3)
    lines = ["%s, torch %s, HIP %s" % (torch.cuda.get_device_name(0), torch.__version__, torch.version.hip),
             "%d queries on the sheet (5 mm of noise); wall time, device synchronised" % args.queries]
    for n in [int(s) for s in args.sizes.split(",")]:
        cloud = sheet(n, gen, dev, 1e-3)
        nb = args.queries if n <= 1000000 else min(args.queries, args.brute_queries)
        for _ in range(3):   # warm-up: every kernel, this shape
            index = hip.point_index(cloud)
            hip.point_nearest(index, pts, want_tested=True)
        if args.brute_reps:
            brute(cloud, pts[:max(1, nb // 10)])
        t = {"build": [], "query": [], "brute": []}
        for r in range(args.reps):
            t["build"].append(wall(lambda: hip.point_index(cloud))[0])
            ms, got = wall(lambda: hip.point_nearest(index, pts))
            t["query"].append(ms)
            if r < args.brute_reps:   # the brute-force route, alternated with the indexed one
                ms, ref = wall(lambda: brute(cloud, pts[:nb]))
                t["brute"].append(ms * args.queries / nb)
        h = index.header()
        counts = index.cell_counts()
        occ = counts[counts > 0].double()
        tested = hip.point_nearest(index, pts, want_tested=True)[2].double()
        lines.append("")
        lines.append("cloud of %d points: grid %d x %d x %d cells of %.5f m (coarse lattice: %d occupied cells, %d occupied 2x2x2 blocks, "
                     "dimension %.2f), %d occupied cells with mean %.2f / max %d points, index %.1f MB" %
                     (n, h["n"][0], h["n"][1], h["n"][2], h["h"], h["c_occ"], h["c_occ2"], h["dim"], occ.numel(), occ.mean().item(),
                      int(occ.max()), index.buf.numel() / 1e6))
        lines.append("  point tests per query: mean %.1f max %d" % (tested.mean().item(), int(tested.max())))
        lines.append("  index build      %s" % med(t["build"]))
        lines.append("  indexed query    %s" % med(t["query"]))
        if t["brute"]:
            same_d2 = torch.equal(got[0][:nb], ref[0])
            differ = int((got[1][:nb].long() != ref[1]).sum())
            note = "" if nb == args.queries else " (measured on %d queries, scaled to %d)" % (nb, args.queries)
            b, q = statistics.median(t["brute"]), statistics.median(t["query"])
            lines.append("  brute force      %s%s" % (med(t["brute"]), note))
            lines.append("  indexed query against brute force: %.1f x; with the index build: %.1f x; d2 %s, %d of %d indices differ" %
                         (b / q, b / (q + statistics.median(t["build"])), "bit-equal" if same_d2 else "DIFFER", differ, nb))
        if not args.no_kdtree:
            from scipy.spatial import cKDTree
            c64, q64 = cloud.double().cpu().numpy(), pts.double().cpu().numpy()
            t0 = time.perf_counter()
            tree = cKDTree(c64)
            t1 = time.perf_counter()
            kd, ki = tree.query(q64, k=1, workers=16)
            t2 = time.perf_counter()
            agree = int((torch.from_numpy(ki).to(dev) == got[1].long()).sum())
            worst = float((torch.from_numpy(kd * kd).to(dev) - got[0]).abs().max())
            lines.append("  cKDTree (host, 16 workers): build %.1f ms, query %.1f ms; %d of %d indices equal, largest |d2 difference| %.3g" %
                         ((t1 - t0) * 1e3, (t2 - t1) * 1e3, agree, args.queries, worst))
        del index, cloud
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
