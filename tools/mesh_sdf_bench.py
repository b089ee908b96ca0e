"""Cost of the truncated signed distance field of a mesh on a lattice (hip.mesh_sdf_grid; geometry.mesh_sdf_grid, geometry.remesh).

    python tools/mesh_sdf_bench.py [--n-side 256] [--reps 11] [--sides 128,256,512] [--steps 1,3,8] [--out profiles/mesh_sdf_bench.txt]

The synthetic subject's posed level set at `--n-side`^3 as an indexed mesh and its simplified meshes (geometry.simplify_mesh at 128
and 64 cells along the longest side).  For each mesh the cube lattice of geometry.mesh_sdf_grid(nodes="corners") at every side of
`--sides` and every band of `--steps` lattice steps: the lattice call hip.mesh_sdf_grid alone (occupancy given, no face; and with the
face), the band's share of the lattice and the point-triangle tests per band node from its counters.  At `--n-side`^3 the same field
the only way the code before this kernel could compute it: hip.mesh_closest on the meshgrid plus hip.mesh_contains_grid -- UNTRUNCATED,
so it does more work: it answers the exact distance at every node, the lattice call only inside the band --, the two routes alternating
in one loop, both with their indices built beforehand, and the number of nodes at which the two disagree inside the band.  The
specification on the same tensors at one small size, and geometry.remesh end to end (host clock: it reads two sizes back).  Whole
calls, device events after warm-up, medians of `--reps` calls; the clocks as rocm-smi reports them when the run starts."""
import argparse
import os
import statistics
import subprocess
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
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--sides", type=str, default="128,256,512")
    ap.add_argument("--steps", type=str, default="1,3,8")
    ap.add_argument("--old-reps", type=int, default=3, help="calls of the untruncated route")
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
    sides = [int(x) for x in args.sides.split(",")]
    steps = [float(x) for x in args.steps.split(",")]
    lines = Lines()
    lines.append("mesh_sdf_bench: %s, torch %s, n_side %d, %d reps; %s" % (torch.cuda.get_device_name(0), torch.__version__, args.n_side,
                                                                          args.reps, clocks()))
    for name, verts, faces in meshes:
        tris = verts[faces.long()].contiguous()
        F = int(tris.shape[0])
        cindex = hip.contains_index(verts, faces, 512)
        lines.append("")
        lines.append("%s: %d vertices, %d faces" % (name, verts.shape[0], F))
        for n in sides:
            if name != meshes[0][0] and n != args.n_side:
                continue
            lat = geometry.mesh_sdf_grid((verts, faces), n_side=n, nodes="corners", padding=0.05, index=cindex)       # the axes; warm-up
            axes, h = (lat["xs"], lat["ys"], lat["zs"]), lat["step"]
            occ, _ = hip.mesh_contains_grid(cindex, *axes)
            t_occ = [timed(lambda: hip.mesh_contains_grid(cindex, *axes))[0] for _ in range(args.reps)]
            lines.append("  %d^3 corners, step %.5f m; hip.mesh_contains_grid %s" % (n, h, med(t_occ)))
            compare = n == args.n_side and name == meshes[0][0]
            if compare:
                index = hip.mesh_index(tris)

                def old_route():
                    grid = torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1).reshape(-1, 3)
                    d2_all = hip.mesh_closest(index, grid, want_closest=False)[0]
                    inside = hip.mesh_contains_grid(cindex, *axes)[0]
                    return d2_all.reshape(n, n, n), inside

                def new_route(trunc):
                    inside = hip.mesh_contains_grid(cindex, *axes)[0]
                    return hip.mesh_sdf_grid(tris, *axes, trunc, occupancy=inside)[0], inside
                old_route()
                for k in steps:
                    new_route(k * h)
                t_old, t_both = [], {k: [] for k in steps}
                for _ in range(args.old_reps):
                    ms, (d2_old, _) = timed(old_route)
                    t_old.append(ms)
                    for k in steps:
                        t_both[k].append(timed(lambda: new_route(k * h))[0])
                lines.append("    the route before this kernel (meshgrid, hip.mesh_closest, hip.mesh_contains_grid; UNTRUNCATED: the exact distance "
                             "at every node, whatever the band) %s" % med(t_old))
            for k in steps:
                trunc = k * h
                hip.mesh_sdf_grid(tris, *axes, trunc, occupancy=occ, want_face=True)
                t_new, t_face = [], []
                for _ in range(args.reps):
                    t_new.append(timed(lambda: hip.mesh_sdf_grid(tris, *axes, trunc, occupancy=occ, want_info=True))[0])
                    t_face.append(timed(lambda: hip.mesh_sdf_grid(tris, *axes, trunc, occupancy=occ, want_face=True))[0])
                d2, _, sdf, info = hip.mesh_sdf_grid(tris, *axes, trunc, occupancy=occ, want_info=True)
                got = hip.read_sdf_grid_info(info)
                lines.append("    trunc %g steps: hip.mesh_sdf_grid %s; with the face %s" % (k, med(t_new), med(t_face)))
                lines.append("        band %d nodes = %.4f of the lattice, %.1f tests per band node (%.3e tests); triangles lane %d, wave %d, "
                             "workgroup %d, several workgroups %d" % (got["band"], got["band"] / n ** 3, got["tests"] / max(got["band"], 1),
                                                                      got["tests"], got["lane"], got["wave"], got["group"], got["huge"]))
                if compare:
                    t = meshing.check_trunc(trunc)
                    cut = torch.where(d2_old > t * t, torch.full_like(d2_old, float("inf")), d2_old)
                    lines.append("        hip.mesh_contains_grid + hip.mesh_sdf_grid, alternating with the route above: %s: %.1f x faster; d2 differs "
                                 "inside the band at %d nodes" % (med(t_both[k]), statistics.median(t_old) / statistics.median(t_both[k]),
                                                                  int((cut != d2).sum())))
                    del cut
                del d2, sdf
            if compare:
                del d2_old
            del occ, lat
    # the specification on the same tensors, one small size
    name, verts, faces = meshes[-1]
    tris = verts[faces.long()].contiguous()
    lat = geometry.mesh_sdf_grid((verts, faces), n_side=32, nodes="corners", padding=0.05)
    axes = (lat["xs"], lat["ys"], lat["zs"])
    t_spec = []
    for _ in range(2):
        ms, spec = timed(lambda: meshing.mesh_sdf_grid(tris, *axes, lat["trunc"], chunk_pairs=1 << 23))
        t_spec.append(ms)
    t_k = [timed(lambda: hip.mesh_sdf_grid(tris, *axes, lat["trunc"], want_face=True))[0] for _ in range(args.reps)]
    got = hip.mesh_sdf_grid(tris, *axes, lat["trunc"], want_face=True)
    lines.append("")
    lines.append("specification (meshing.mesh_sdf_grid, brute force in torch) on %s at 32^3, trunc 3 steps: %s; the kernel with the face %s; "
                 "d2 differs at %d nodes, face at %d" % (name, med(t_spec), med(t_k), int((spec[0] != got[0]).sum()), int((spec[1] != got[1]).sum())))
    # remesh end to end
    name, verts, faces = meshes[0]
    geometry.remesh((verts, faces), n_side=args.n_side)
    t_r = []
    for _ in range(min(args.reps, 5)):
        ms, out = host_timed(lambda: geometry.remesh((verts, faces), n_side=args.n_side))
        t_r.append(ms)
    topo = geometry.mesh_topology(out[0], out[1])
    lines.append("geometry.remesh(%s, n_side=%d) end to end (both indices, lattice, extraction, two read-backs; host clock) %s -> %d vertices, "
                 "%d faces, watertight %s, Euler characteristic %d" % (name, args.n_side, med(t_r), out[0].shape[0], out[1].shape[0],
                                                                      topo["watertight"], topo["euler"]))
    text = "\n".join(lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
