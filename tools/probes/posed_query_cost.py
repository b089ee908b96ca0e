"""Run from the repository root: `timeout -k 10 600 python tools/probes/posed_query_cost.py` (one GPU).
Cost of the posed queries on the synthetic zju377_mono subject, frame 0, both engines: arah_query_posed on 1e6 surface points
jittered by +-3 cm and on 1e6 points uniform in the SMPL box; posed_mesh's lattice at n_side 256, banded and full (lattice +
marching cubes), with the evaluated fraction, the triangles and the unconverged count.  Torch events; medians of 5."""
import json, os, sys
sys.path.insert(0, os.getcwd())
import torch
from arah_release_amd import config, hip, renderer, synthetic

dev = torch.device("cuda:0")
scene = synthetic.SyntheticScene(0)


def timed(fn, reps=5):
    fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); r = fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2], r


res = {}
for eng in ("split", "fp32"):
    os.environ["ARAH_PRECISION"] = eng
    model, _ = config.build_synthetic_model("zju377_mono", device=dev)
    model.eval()
    inputs = scene.make_inputs(512, 512, frame_idx=0, device=dev)
    with torch.no_grad():
        out = model.forward_maps(inputs)
        frame, ws = model._posed_frame(inputs, "probe")
        acc, depth = out["acc_values"][0], out["depth_values"][0]
        surf = (inputs["cam_loc"][0].reshape(1, 3) + depth[:, None] * inputs["ray_dirs"][0])[acc > 0.99]
        g = torch.Generator(device="cpu").manual_seed(0)
        pick = torch.randint(0, surf.shape[0], (1 << 20,), generator=g).to(dev)
        jit = (surf[pick] + ((torch.rand(1 << 20, 3, generator=g) * 2 - 1) * 0.03).to(dev)).contiguous()
        v = inputs["smpl_verts"][0]
        lo, hi = v.min(0).values, v.max(0).values
        uni = (lo + (hi - lo) * torch.rand(1 << 20, 3, generator=g).to(dev)).contiguous()
        occ = ws.occupancy(frame)
        r = {}
        for name, pts in (("jittered_surface", jit), ("uniform_box", uni)):
            for cert in (False, True):
                ms, q = timed(lambda: hip.query_posed(frame, ws, pts, occ=occ if cert else None))
                st = q["state"]
                r["query_%s%s" % (name, "_certify" if cert else "")] = {
                    "ms": round(ms, 3), "points_per_s": round(pts.shape[0] / ms * 1e3),
                    "converged": int((st == 1).sum()), "unconverged": int((st == 0).sum()), "certified": int((st == 2).sum())}
        for band in (True, False):
            def mesh():
                sdf, box, counts = hip.sdf_grid_posed(frame, ws, 256, occ=occ, band=band)
                tris, n = hip.marching_cubes(sdf, 0.0, 1 << 21)
                return counts, n, box
            ms, (counts, n, box) = timed(mesh)
            ms_grid, _ = timed(lambda: hip.sdf_grid_posed(frame, ws, 256, occ=occ, band=band))
            c = counts.tolist()
            r["posed_mesh_256_%s" % ("band" if band else "full")] = {
                "ms": round(ms, 3), "lattice_ms": round(ms_grid, 3), "evaluated": c[0], "evaluated_fraction": round(c[0] / 256 ** 3, 4),
                "converged": c[1], "unconverged": c[0] - c[1], "skipped": c[2], "triangles": int(n.item()),
                "box": [round(x, 4) for x in box.tolist()]}
        info = ws.occupancy_info()
        r["bitmap_box_m"] = [info["dims"][a] * info["voxel"] for a in range(3)]
        r["body_box_m"] = (hi - lo).tolist()
    res[eng] = r
print(json.dumps(res, indent=1))
