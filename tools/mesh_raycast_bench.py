"""Cost of casting rays against indexed meshes on the device (hip.mesh_raycast; geometry.cast_rays / ambient_occlusion), against the
brute-force specification on the same device tensors and against drawing the same pixels (geometry.render_mesh).

    python tools/mesh_raycast_bench.py [--n-side 256] [--sizes 512,1024] [--reps 20] [--spec-reps 1] [--out profiles/mesh_raycast_bench.txt]

The synthetic subject's posed level set at n_side^3 as an indexed mesh (what posed_mesh(indexed=True) gives), (a) as it is and (b)
after geometry.simplify_mesh with cells of 4 and 16 lattice steps -- the meshes of tools/mesh_render_bench.py -- seen along the
rays through the pixel centres of the frame's camera at size^2 (geometry.camera_rays), and the V x 64 rays of
geometry.ambient_occlusion.  After warm-up, with device events around the whole calls: median, min and max.

    kernel  hip.mesh_raycast on an index built beforehand: the allocation of the outputs and one launch; first hit, any hit, and the
            first hit at workgroups of 64, 128 and 256 threads
    index   hip.mesh_index of the mesh (needed once per mesh)
    spec    meshing.mesh_raycast on the same tensors, chunked to 2 GiB of temporaries; --spec-reps calls after one warm-up call on a
            slice of the rays (it is seconds to minutes per call)
    raster  geometry.render_mesh of the same mesh, camera and pixels (projection + hip.mesh_rasterize), for the camera rays

and, per set of rays: the mean and the largest number of ray-triangle tests per ray, the share of rays that miss the index's
box, the share that hit, and whether kernel and specification agree bit for bit."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SPEC_CHUNK = 1 << 31


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def med(v):
    return "median %.3f ms (min %.3f, max %.3f, %d calls)" % (statistics.median(v), min(v), max(v), len(v))


def run(routes, reps, warm=3):
    for _ in range(warm):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in routes}
    for _ in range(reps):
        for name, fn in routes.items():
            t[name].append(timed(fn)[0])
    return t


def misses_box(hdr, o, d):
    """share of rays that do not meet the index's bounding box at t >= 0 (float64 slabs; the figure is a statistic)"""
    lo = torch.tensor(hdr["lo"], dtype=torch.float64, device=o.device)
    hi = torch.tensor(hdr["hi"], dtype=torch.float64, device=o.device)
    o, d = o.double(), d.double()
    inv = 1.0 / d
    t0, t1 = (lo - o) * inv, (hi - o) * inv
    near, far = torch.minimum(t0, t1), torch.maximum(t0, t1)
    still = d == 0
    near = torch.where(still, torch.full_like(near, -float("inf")), near)
    far = torch.where(still, torch.full_like(far, float("inf")), far)
    out = (still & ((o < lo) | (o > hi))).any(1)
    return float((out | (near.max(1).values.clamp_min(0) > far.min(1).values)).float().mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-side", type=int, default=256)
    ap.add_argument("--sizes", default="512,1024")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--spec-reps", type=int, default=1)
    ap.add_argument("--ao-rays", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from arah_release_amd import config, geometry, hip, meshing, synthetic
    dev = torch.device("cuda:0")
    model, _ = config.build_synthetic_model("zju377_mono", device=dev)
    model.eval()
    scene = synthetic.SyntheticScene(0)
    inputs = scene.make_inputs(32, 32, frame_idx=0, device=dev)
    with torch.no_grad():
        posed = model.posed_mesh(inputs, n_side=args.n_side, indexed=True)
    verts, faces = posed["verts"].contiguous(), posed["faces"].contiguous()
    lattice_step = float(posed["box"][3]) / (args.n_side - 1)
    meshes = {"(a) level set": (verts, faces)}
    for k in (4, 16):
        s = geometry.simplify_mesh(verts, faces, cell=k * lattice_step)
        meshes["(b) cells of %d steps" % k] = (s["verts"].contiguous(), s["faces"].contiguous())
    lines = []

    def say(line=""):
        lines.append(line)
        print(line, flush=True)
    say("%s, torch %s, HIP %s" % (torch.cuda.get_device_name(0), torch.__version__, torch.version.hip))
    say("posed level set at %d^3; " % args.n_side + "; ".join("%s: %d vertices, %d faces" % (k, v.shape[0], f.shape[0])
                                                              for k, (v, f) in meshes.items()))
    sizes = [int(s) for s in args.sizes.split(",")]

    def measure(title, index, tris, o, d, kw, extra=None):
        """one set of rays against one index: the kernel's routes, the specification, the statistics"""
        hdr = index.header()
        say("")
        say("%s: %d rays, %d faces, grid %s, %d references, %d on the big list" % (title, o.shape[0], tris.shape[0], hdr["n"], hdr["n_refs"],
                                                                                hdr["n_big"]))
        routes = {"kernel  first hit": lambda: hip.mesh_raycast(index, o, d, **kw),
                  "kernel  any hit": lambda: hip.mesh_raycast(index, o, d, mode="any", **kw)}
        for wg in (64, 128, 256):
            routes["kernel  first hit, workgroup %d" % wg] = lambda wg=wg: hip.mesh_raycast(index, o, d, workgroup=wg, **kw)
        routes["index   hip.mesh_index"] = lambda: hip.mesh_index(tris)
        routes.update(extra or {})
        t = run(routes, args.reps)
        for k in t:
            say("  %-64s %s" % (k, med(t[k])))
        got = hip.mesh_raycast(index, o, d, want_tested=True, **kw)
        tested_any = hip.mesh_raycast(index, o, d, mode="any", want_tested=True, **kw)[1]
        say("  tests per ray: first hit mean %.1f, max %d; any hit mean %.1f, max %d; %.4f of the rays miss the box, %.4f hit"
            % (float(got[3].float().mean()), int(got[3].max()), float(tested_any.float().mean()), int(tested_any.max()),
               misses_box(hdr, o, d), float((got[1] >= 0).float().mean())))
        if args.spec_reps:
            spec = lambda: meshing.mesh_raycast(tris, o, d, chunk_bytes=SPEC_CHUNK, **kw)
            meshing.mesh_raycast(tris, o[:4096], d[:4096], chunk_bytes=SPEC_CHUNK, **kw)      # warm-up on a slice
            torch.cuda.synchronize()
            ts, want = [], None
            for _ in range(args.spec_reps):
                ms, want = timed(spec)
                ts.append(ms)
            say("  %-64s %s" % ("spec    meshing.mesh_raycast, chunked", med(ts)))
            same = all(torch.equal(a.view(torch.int64) if a.is_floating_point() else a, b.view(torch.int64) if b.is_floating_point() else b)
                       for a, b in zip(got[:3], want))
            say("  spec / kernel (first hit) = %.0f x; kernel against the specification: %s"
                % (statistics.median(ts) / statistics.median(t["kernel  first hit"]), "bit-equal" if same else "DIFFER"))

    with torch.no_grad():
        for name, (v, f) in meshes.items():
            tris = v[f.long()].contiguous()
            index = hip.mesh_index(tris)
            for size in sizes:
                # the frame's camera at this size (synthetic.make_inputs: focal 1.2 H, principal point at the image centre, R = I, t = 0)
                cam = {"cam_rot": inputs["cam_rot"][0], "cam_trans": inputs["cam_trans"][0].reshape(3),
                       "K": torch.tensor([[1.2 * size, 0, size / 2.0], [0, 1.2 * size, size / 2.0], [0, 0, 1]], device=dev)}
                o, d = geometry.camera_rays(cam, size, size)
                extra = {"raster  geometry.render_mesh, the same pixels": lambda: geometry.render_mesh(v, f, size, size, camera=cam),
                         "whole   geometry.cast_rays (index given)": lambda: geometry.cast_rays((v, f), o, d, index=index)}
                measure("%s, camera rays %d x %d" % (name, size, size), index, tris, o, d, {}, extra)
            if name.startswith("(a)") or "4 steps" in name:
                # the level set is wound with its normals into the body: reversed, the hemispheres look out of it
                fo = f.flip(1).contiguous()
                v32 = v.to(torch.float32).contiguous()
                o, d = geometry.ao_rays(v32, fo, args.ao_rays, 0, 1e-4)
                o, d = o.contiguous(), d.contiguous()
                tris_o = v32[fo.long()].contiguous()
                index_o = hip.mesh_index(tris_o)
                extra = {"whole   geometry.ambient_occlusion": lambda: geometry.ambient_occlusion(v32, fo, n_rays=args.ao_rays)}
                measure("%s, ambient occlusion %d rays per vertex" % (name, args.ao_rays), index_o, tris_o, o, d, {}, extra)
                ao = geometry.ambient_occlusion(v32, fo, n_rays=args.ao_rays)
                say("  ambient occlusion: mean %.3f, min %.3f, %.3f of the vertices fully open" % (float(ao.mean()), float(ao.min()),
                                                                                               float((ao == 1).float().mean())))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
