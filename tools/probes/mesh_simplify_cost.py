"""Run from the repository root: `timeout -k 10 600 python tools/probes/mesh_simplify_cost.py [out.txt]` (one GPU).
Cost of simplifying an indexed mesh by vertex clustering (csrc/meshsimp.hpp) on the 256^3 posed mesh of the synthetic zju377_mono
subject, frame 0, at cells of 2 and 4 lattice steps, both positions.  Device events around each call, 5 warm-up passes, then 30 passes
that alternate the calls in one process; median and the 10 % / 90 % quantiles in ms:

  kernels        hip.mesh_simplify alone: the launches of arah_mesh_simplify, nothing read back
  spec_on_device meshing.mesh_simplify (the tensor specification: torch.unique, index_add_, scatter_reduce ...) on the same GPU
                 tensors; it reads sizes back as it goes
  simplify_mesh  geometry.simplify_mesh with the bounds given: kernels, removal of unreferenced clusters, ONE read of the sizes
  simplify_mesh_own_bounds   the same with the vertices' box for bounds: one more read
  extraction     hip.marching_cubes_indexed of the same volume, for scale

Before timing, the script asserts that the kernels' outputs are the specification's, bit for bit.  Next to the times: the sizes
before and after, and geometry.mesh_metrics of the simplified mesh against the original (Chamfer-L1 and Hausdorff distances in
metres and in lattice steps)."""
import json, os, sys
sys.path.insert(0, os.getcwd())
import torch
from arah_release_amd import config, geometry, hip, meshing, synthetic

dev = torch.device("cuda:0")
args = [a for a in sys.argv[1:] if not a.startswith("--")]


def events(fns, warm=5, reps=30):
    for _ in range(warm):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); f(); b.record(); torch.cuda.synchronize()
            ts[k].append(a.elapsed_time(b))
    return {k: quantiles(v) for k, v in ts.items()}


def quantiles(v):
    v = sorted(v)
    return {"median_ms": round(v[len(v) // 2], 4), "p10_ms": round(v[len(v) // 10], 4), "p90_ms": round(v[(9 * len(v)) // 10], 4)}


model, _ = config.build_synthetic_model("zju377_mono", device=dev)
model.eval()
inputs = synthetic.SyntheticScene(0).make_inputs(512, 512, frame_idx=0, device=dev)
N = 256
res = {}
with torch.no_grad():
    frame, ws = model._posed_frame(inputs, "probe")
    occ = ws.occupancy(frame)
    sdf, box, _ = hip.sdf_grid_posed(frame, ws, N, occ=occ, box=None, band=True)
    sdf = sdf.clone()
    mesh = model.posed_mesh(inputs, n_side=N, indexed=True)
    verts, faces = mesh["verts"].contiguous(), mesh["faces"].contiguous()
    step = float(box[3]) / (N - 1)
    lo, hi = verts.min(0).values.tolist(), verts.max(0).values.tolist()
    res["mesh"] = {"n_verts": mesh["n_verts"], "n_faces": mesh["n_tris"], "lattice_step_m": step}
    for mult in (2.0, 4.0):
        cell = mult * step
        origin, dims = geometry.simplify_grid_of(lo, hi, cell)
        grid = (origin.tolist(), float(cell), dims)
        for position in ("mean", "member"):
            got = hip.mesh_simplify(verts, faces, *grid, position=position)
            ref = meshing.mesh_simplify(verts, faces, *grid, position=position)
            for a, b in zip(got, ref):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        r = events({"extraction": lambda: hip.marching_cubes_indexed(sdf, 0.0, 1 << 19, 1 << 20),
                    "kernels": lambda: hip.mesh_simplify(verts, faces, *grid),
                    "kernels_member_no_dedup": lambda: hip.mesh_simplify(verts, faces, *grid, position="member", dedup=False),
                    "spec_on_device": lambda: meshing.mesh_simplify(verts, faces, *grid),
                    "simplify_mesh": lambda: geometry.simplify_mesh(verts, faces, cell=cell, bounds=(lo, hi)),
                    "simplify_mesh_own_bounds": lambda: geometry.simplify_mesh(verts, faces, cell=cell)})
        r["spec_over_kernels"] = round(r["spec_on_device"]["median_ms"] / r["kernels"]["median_ms"], 1)
        for position in ("mean", "member"):
            small = geometry.simplify_mesh(verts, faces, cell=cell, position=position)
            m = geometry.mesh_metrics((small["verts"], small["faces"]), (verts, faces), n_samples=100000)
            r[position] = {"n_verts": small["n_verts"], "n_faces": small["n_tris"], "removed": small["removed"], "dims": small["dims"],
                           "faces_kept_share": round(small["n_tris"] / mesh["n_tris"], 4)}
            for k in ("chamfer_l1", "hausdorff_ab", "hausdorff_ba"):
                r[position][k + "_m"] = float(m[k])
                r[position][k + "_steps"] = round(float(m[k]) / step, 3)
        res["cell_%gx" % mult] = r
text = json.dumps(res, indent=1)
print(text)
if args:
    with open(args[0], "w") as f:
        f.write(text + "\n")
