"""Cost of the device-side geometry scores (hip.mesh_index / hip.mesh_closest / hip.surface_metrics; geometry.mesh_metrics).

    python tools/geometry_metrics_bench.py [--samples 100000] [--reps 20] [--brute-reps 3] [--cumsum-repeats 50]
                                           [--frames 20 --passes 3] [--out profiles/geometry_metrics.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/geometry_metrics_bench.py --reps 5 --brute-reps 0    # per kernel

Two meshes of the size posed_mesh gives at 256^3: the synthetic subject's posed level set on its default lattice (A) and on
a lattice moved by a fraction of a voxel (B: the same surface, triangulated differently -- what a ground truth of similar
size looks like to the index), `--samples` area-weighted samples each way.  After warm-up, with device events around the
calls: median time of the index build (per mesh), of the indexed query (per direction) and of the reduction; mean and maximum
point-triangle tests per query; and the same queries through hip.mesh_query, the brute-force route, alternated with the
indexed ones in the same loop.  The two routes' d2 and face are compared for equality while at it.
--cumsum-repeats N: how many of N repeats of torch.cumsum over mesh A's face areas (float64, and float32 as
data.sample_surface forms them by default) differ in any bit from the first, next to the same count for hip.face_area_cumsum.
--frames N --passes K: N benchmark frames (512^2 x 64) through renderer.map_in_flight as validate does it, passes alternating:
(a) validation_step(metrics="device") alone, (b) the same step followed by model.geometry_metrics against a ground-truth mesh
(validate --geometry's step), (c) geometry_metrics alone, in flight, (d) geometry_metrics alone, one frame at a time."""
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


def med(v):
    return "median %.3f ms (min %.3f, max %.3f, %d calls)" % (statistics.median(v), min(v), max(v), len(v))


def cumsum_repro(a, repeats):
    """Lines: of `repeats` repeats of each cumulative sum of a's face areas, how many differ bitwise from the first."""
    from arah_release_amd import hip
    e1, e2 = (a[:, 1] - a[:, 0]).double(), (a[:, 2] - a[:, 0]).double()
    area64 = torch.linalg.cross(e1, e2).norm(dim=-1) * 0.5
    area32 = torch.linalg.cross(a[:, 1] - a[:, 0], a[:, 2] - a[:, 0]).norm(dim=-1) * 0.5
    routes = (("torch.cumsum float64", lambda: torch.cumsum(area64, 0)), ("torch.cumsum float32", lambda: torch.cumsum(area32, 0)),
              ("hip.face_area_cumsum", lambda: hip.face_area_cumsum(a)))
    lines = ["cumulative areas of mesh A (%d faces), %d repeats each, repeats that differ in any bit from the first:" %
             (a.shape[0], repeats)]
    for name, fn in routes:
        first = fn().clone()
        differ, worst = 0, 0
        for _ in range(repeats):
            c = fn()
            if not torch.equal(c, first):
                differ += 1
                worst = max(worst, int((c != first).sum()))
        lines.append("  %-22s %d of %d differ%s" % (name, differ, repeats, " (up to %d entries)" % worst if differ else ""))
    return lines


def scored_frames_in_flight(dev, n_frames, passes, n_samples):
    """Lines: ms per frame of validate's step without and with the geometry scores, and of the scores alone."""
    from arah_release_amd import config, renderer, synthetic
    model, cfg = config.build_synthetic_model("zju377_mono", 64, 16, 16, device=dev)
    lm = config.LightningModel(model, cfg).eval()
    lm.compose_inputs = lambda data, eval: dict(data["model_inputs"])    # bench.py's frames are composed model inputs
    scene = synthetic.SyntheticScene(0)
    items = []
    gen = torch.Generator(device=dev).manual_seed(1)
    with torch.no_grad():
        for k in range(n_frames):
            inp = scene.make_inputs(512, 512, frame_idx=k, device=dev)
            n = int(inp["ray_dirs"].shape[1])
            items.append({"model_inputs": inp, "inputs.image_mask": inp["image_mask"],
                          "inputs": torch.rand(1, n, 3, device=dev, generator=gen),
                          "gt": model.posed_mesh(dict(inp), n_side=256)["tris"].contiguous()})

    def image_only(it):
        return lm.validation_step({k: v for k, v in it.items() if k != "gt"}, metrics="device")

    def scores_only(it):
        return model.geometry_metrics(lm.compose_inputs(it, eval=True), it["gt"], n_side=256, n_samples=n_samples, seed=0)

    def both(it):
        out = image_only(it)
        out["geometry"] = scores_only(it)
        return out

    variants = {"a validation_step(metrics='device')": (image_only, None), "b a + geometry_metrics (validate --geometry)": (both, None),
                "c geometry_metrics alone, in flight": (scores_only, None), "d geometry_metrics alone, one at a time": (scores_only, 1)}
    for fn, ns in variants.values():                                     # warm-up: every shape, every variant
        renderer.map_in_flight(fn, items[:4], n_streams=ns, owner=model)
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(passes):
        for name, (fn, ns) in variants.items():                          # alternating
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs = renderer.map_in_flight(fn, items, n_streams=ns, owner=model)
            torch.cuda.synchronize()
            times[name].append(1e3 * (time.perf_counter() - t0) / n_frames)
            del outs
    lines = ["%d frames 512^2 x 64 through map_in_flight (%d in flight), ground truth = the frame's own posed mesh at 256^3, "
             "%d alternating passes, ms per frame:" % (n_frames, renderer.frames_in_flight(n_frames), passes)]
    for name, t in times.items():
        lines.append("  (%s) median %.2f  min %.2f  max %.2f  passes %s" % (name, statistics.median(t), min(t), max(t),
                                                                             " ".join("%.2f" % v for v in t)))
    a, b, c, d = (statistics.median(times[k]) for k in variants)
    lines.append("  (b) - (a) = %+.2f ms per scored frame; the scores alone %.2f in flight, %.2f one at a time: %.2f ms of a scored "
                 "frame's %.2f + %.2f run under other frames" % (b - a, c, d, a + d - b, a, d))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--brute-reps", type=int, default=3)
    ap.add_argument("--n-side", type=int, default=256)
    ap.add_argument("--cumsum-repeats", type=int, default=0)
    ap.add_argument("--frames", type=int, default=0)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from arah_release_amd import config, data, geometry, hip, synthetic
    dev = torch.device("cuda:0")
    model, _ = config.build_synthetic_model("zju377_mono", device=dev)
    model.eval()
    inputs = synthetic.SyntheticScene(0).make_inputs(32, 32, frame_idx=0, device=dev)
    with torch.no_grad():
        mesh_a = model.posed_mesh(inputs, n_side=args.n_side)
        box = mesh_a["box"].cpu()
        vox = float(box[3]) / (args.n_side - 1)
        lo, hi = box[:3] - 0.37 * vox, box[:3] + box[3] + 0.21 * vox
        mesh_b = model.posed_mesh(inputs, n_side=args.n_side, bounds=(lo, hi))
    a, b = mesh_a["tris"].contiguous(), mesh_b["tris"].contiguous()
    gen = torch.Generator(device=dev).manual_seed(0)
    n = args.samples

    def soup_faces(t):
        return torch.arange(t.shape[0] * 3, device=dev).reshape(-1, 3)
    pa, fa = data.sample_surface(a.reshape(-1, 3), soup_faces(a), n, generator=gen)
    pb, fb = data.sample_surface(b.reshape(-1, 3), soup_faces(b), n, generator=gen)
    pa, pb, fa, fb = pa.contiguous(), pb.contiguous(), fa.to(torch.int32), fb.to(torch.int32)
    va, vb = a.reshape(-1, 3).contiguous(), b.reshape(-1, 3).contiguous()
    ia, ib = soup_faces(a).to(torch.int32), soup_faces(b).to(torch.int32)
    lines = ["%s, torch %s, HIP %s" % (torch.cuda.get_device_name(0), torch.__version__, torch.version.hip),
             "mesh A %d triangles, mesh B %d triangles (posed level sets at %d^3), %d samples each way" %
             (a.shape[0], b.shape[0], args.n_side, n)]
    for _ in range(3):   # warm-up: every kernel, every shape
        index_a, index_b = hip.mesh_index(a), hip.mesh_index(b)
        qab = hip.mesh_closest(index_b, pa, want_closest=False, want_tested=True)
        qba = hip.mesh_closest(index_a, pb, want_closest=False, want_tested=True)
        hip.surface_metrics(a, fa, qab[0], qab[1], b, fb, qba[0], qba[1])
        geometry.mesh_metrics(a, b, n_samples=n, seed=0)
    if args.brute_reps:
        hip.mesh_query(vb, ib, pa[:1024].contiguous())
    torch.cuda.synchronize()
    for name, idx in (("A", index_a), ("B", index_b)):
        h = idx.header()
        lines.append("index %s: grid %d x %d x %d cells of %.4f m, %d references (%.2f per triangle), %d triangles on the big list, "
                     "%.1f MB" % (name, h["n"][0], h["n"][1], h["n"][2], h["h"], h["n_refs"], h["n_refs"] / idx.tris.shape[0],
                                  h["n_big"], idx.buf.numel() / 1e6))
    t = {k: [] for k in ("build A", "build B", "query A->B", "query B->A", "reduce", "mesh_metrics", "brute A->B", "brute B->A")}
    for r in range(args.reps):
        t["build A"].append(timed(lambda: hip.mesh_index(a))[0])
        t["build B"].append(timed(lambda: hip.mesh_index(b))[0])
        ms, qab = timed(lambda: hip.mesh_closest(index_b, pa, want_closest=False))
        t["query A->B"].append(ms)
        ms, qba = timed(lambda: hip.mesh_closest(index_a, pb, want_closest=False))
        t["query B->A"].append(ms)
        t["reduce"].append(timed(lambda: hip.surface_metrics(a, fa, qab[0], qab[1], b, fb, qba[0], qba[1]))[0])
        t["mesh_metrics"].append(timed(lambda: geometry.mesh_metrics(a, b, n_samples=n, seed=0))[0])
        if r < args.brute_reps:   # the brute-force route, alternated with the indexed one
            ms, bab = timed(lambda: hip.mesh_query(vb, ib, pa))
            t["brute A->B"].append(ms)
            ms, bba = timed(lambda: hip.mesh_query(va, ia, pb))
            t["brute B->A"].append(ms)
            same = (torch.equal(bab[0], qab[0]) and torch.equal(bab[1], qab[1]) and torch.equal(bba[0], qba[0])
                    and torch.equal(bba[1], qba[1]))
            lines.append("pass %d: indexed and brute-force d2 / face %s" % (r, "bit-equal" if same else "DIFFER"))
    for k, v in t.items():
        if v:
            lines.append("%-13s %s" % (k, med(v)))
    tab = hip.mesh_closest(index_b, pa, want_closest=False, want_tested=True)[3].double()
    tba = hip.mesh_closest(index_a, pb, want_closest=False, want_tested=True)[3].double()
    lines.append("point-triangle tests per query: A->B mean %.1f max %d of %d triangles (%.4f %%); B->A mean %.1f max %d of %d (%.4f %%)" %
                 (tab.mean().item(), int(tab.max()), b.shape[0], 100 * tab.mean().item() / b.shape[0], tba.mean().item(), int(tba.max()),
                  a.shape[0], 100 * tba.mean().item() / a.shape[0]))
    if t["brute A->B"]:
        q = statistics.median(t["query A->B"]) + statistics.median(t["query B->A"])
        full = q + statistics.median(t["build A"]) + statistics.median(t["build B"])
        br = statistics.median(t["brute A->B"]) + statistics.median(t["brute B->A"])
        lines.append("both directions: brute force %.1f ms, indexed queries %.3f ms (%.0f x), with both index builds %.3f ms (%.0f x)" %
                     (br, q, br / q, full, br / full))
    res = geometry.mesh_metrics(a, b, n_samples=n, seed=0)
    lines.append("scores: " + ", ".join("%s %.6g" % (k, float(res[k])) for k in geometry.METRIC_KEYS))
    if args.cumsum_repeats:
        lines += cumsum_repro(a, args.cumsum_repeats)
    if args.frames:
        del index_a, index_b, qab, qba
        lines += scored_frames_in_flight(dev, args.frames, args.passes, n)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
