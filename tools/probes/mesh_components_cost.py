"""Run from the repository root: `timeout -k 10 600 python tools/probes/mesh_components_cost.py [out.txt]` (one GPU).
Cost of arah_mesh_components and arah_mesh_select (csrc/meshcc.hpp) on two indexed meshes: the 256^3 canonical level set of the
synthetic zju377_mono subject, frame 0 (one body, one component), and the level set of a 128^3 volume of seeded white noise (more
than 10^4 components).  Device events around each call, 5 warm-up passes, then 30 passes that alternate the calls in one process;
median and the 10 % / 90 % quantiles in ms.  Next to them the same labelling through the host -- faces copied out,
scipy.sparse.csgraph.connected_components, labels copied back, a host clock around it all ending in a device synchronise -- and the
extraction that produced the mesh (hip.marching_cubes_indexed on the same volume; profiles/indexed_mesh.txt has 0.57 ms for the body).
components_reversed_faces is the labelling with the faces in reverse order (chain depth depends on the order of arrival).
Before timing, the script asserts that the kernels' labels are scipy's partition, in both orders.

`--kernels=body_256` / `--kernels=noise_128`: no timing, 20 plain passes of the two calls on that mesh, to be run under
`rocprofv3 --kernel-trace --stats` in a run of its own for the per-kernel times (which stage dominates)."""
import json, os, sys, time
sys.path.insert(0, os.getcwd())
import numpy as np
import torch
from arah_release_amd import config, hip, synthetic

dev = torch.device("cuda:0")
args = [a for a in sys.argv[1:] if not a.startswith("--")]
kernels_only = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--kernels=")]


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


def host_labels(faces, V):
    """The host round trip: faces out, scipy, labels back."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    f = faces.cpu().numpy().astype(np.int64)
    graph = coo_matrix((np.ones(2 * f.shape[0], np.int8), (np.concatenate([f[:, 0], f[:, 0]]), np.concatenate([f[:, 1], f[:, 2]]))),
                       shape=(V, V))
    n, lab = connected_components(graph, directed=False)
    return n, torch.from_numpy(lab).to(dev)


def noise(n, seed=11):
    v = torch.randn(n, n, n, generator=torch.Generator().manual_seed(seed))
    v[0], v[-1], v[:, 0], v[:, -1], v[:, :, 0], v[:, :, -1] = 1, 1, 1, 1, 1, 1
    return v


model, _ = config.build_synthetic_model("zju377_mono", device=dev)
model.eval()
inputs = synthetic.SyntheticScene(0).make_inputs(512, 512, frame_idx=0, device=dev)
res = {}
with torch.no_grad():
    frame, ws = model._posed_frame(inputs, "probe")
    volumes = {"body_256": hip.sdf_grid_band(frame, ws, 256)[0].clone(), "noise_128": noise(128).to(dev)}
    for name, sdf in volumes.items():
        if kernels_only and name not in kernels_only:
            continue
        caps = (1 << 19, 1 << 20) if name == "body_256" else (1 << 22, 1 << 23)
        verts, faces, counts = hip.marching_cubes_indexed(sdf, 0.0, *caps)
        V, F = counts.tolist()
        assert V <= caps[0] and F <= caps[1]
        faces = faces[:F].contiguous()
        labels, comp_verts, comp_faces, cc = hip.mesh_components(faces, V)
        keep = (torch.arange(V, device=dev) == cc[2]).to(torch.int32)            # "largest"
        kept = hip.mesh_select(faces, V, labels, keep)[4]
        C, n_valid, largest = cc.tolist()
        n_host, lab_host = host_labels(faces, V)
        first = torch.full((n_host,), V, dtype=torch.int64, device=dev).scatter_reduce(0, lab_host.long(), torch.arange(V, device=dev), "amin")
        rank = torch.empty(n_host, dtype=torch.int64, device=dev)
        rank[torch.argsort(first)] = torch.arange(n_host, device=dev)
        assert n_host == C and n_valid == F and torch.equal(rank[lab_host.long()], labels.long())
        if name == "noise_128":
            assert C >= 10 ** 4, C
        if kernels_only:
            for _ in range(20):
                hip.mesh_components(faces, V)
                hip.mesh_select(faces, V, labels, keep)
            torch.cuda.synchronize()
            continue
        reversed_faces = faces.flip(0).contiguous()                              # the order that builds the deepest chains one by one
        assert torch.equal(hip.mesh_components(reversed_faces, V)[0], labels)
        r = events({"extraction": lambda: hip.marching_cubes_indexed(sdf, 0.0, *caps),
                    "components": lambda: hip.mesh_components(faces, V),
                    "components_reversed_faces": lambda: hip.mesh_components(reversed_faces, V),
                    "select_largest": lambda: hip.mesh_select(faces, V, labels, keep)})
        host = []
        for i in range(25):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host_labels(faces, V)
            torch.cuda.synchronize()
            if i >= 5:
                host.append(1e3 * (time.perf_counter() - t0))
        r["host_scipy_round_trip"] = quantiles(host)
        r["host_over_components"] = round(r["host_scipy_round_trip"]["median_ms"] / r["components"]["median_ms"], 1)
        r["components_over_extraction"] = round(r["components"]["median_ms"] / r["extraction"]["median_ms"], 2)
        r.update({"n_verts": V, "n_faces": F, "n_components": C, "largest_faces": int(comp_faces[largest]),
                  "kept_by_largest": kept.tolist()})
        res[name] = r
if not kernels_only:
    text = json.dumps(res, indent=1)
    print(text)
    if args:
        with open(args[0], "w") as f:
            f.write(text + "\n")
