"""Cost of drawing indexed meshes on the device (hip.mesh_rasterize / hip.mesh_interpolate; geometry.render_mesh), against the
triangle-soup rasteriser of the gen_cano_mesh branch (hip.rasterize, unchanged) and against the tensor specification.

    python tools/mesh_render_bench.py [--n-side 256] [--sizes 512,1024] [--reps 20] [--spec-reps 3] [--out profiles/mesh_render_bench.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/mesh_render_bench.py --reps 5 --spec-reps 0 --no-sweep    # per kernel

The synthetic subject's posed level set at n_side^3 as an indexed mesh (what posed_mesh(indexed=True) gives), projected through the
frame's camera into size^2 images: (a) as it is, (b) after geometry.simplify_mesh with cells of 4 and 16 lattice steps (large
triangles), (c) as it is plus two triangles that cover the whole image behind it; (d) interpolation of 3 and 24 channels over (a).
After warm-up of every route at its size, with device events around the calls and the routes alternated in one loop: median, min
and max.  `new` is the whole call (key buffer, init, pass A, its lists, pass B: four launches and three outputs), `old` the whole
hip.rasterize call (its key fill, k_raster, the decode: pix_to_face only), `spec` meshing.mesh_rasterize on the same GPU tensors.
The three thresholds of pass A are swept on (a) and (b).  Last: the silhouette IoU and the median absolute depth
difference between the drawn mesh and the volume render (forward_maps, opacity > 0.5) of the same frame -- reported, not asserted."""
import argparse
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


def run(routes, reps, spec_routes=None, spec_reps=0):
    """Warm every route up, then time them alternately: -> {name: [ms]}."""
    spec_routes = spec_routes or {}
    for _ in range(3):
        for fn in routes.values():
            fn()
    if spec_reps:
        for fn in spec_routes.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in list(routes) + (list(spec_routes) if spec_reps else [])}
    for r in range(reps):
        for name, fn in routes.items():
            t[name].append(timed(fn)[0])
        if r < spec_reps:
            for name, fn in spec_routes.items():
                t[name].append(timed(fn)[0])
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-side", type=int, default=256)
    ap.add_argument("--sizes", default="512,1024")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--spec-reps", type=int, default=3)
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--maps-size", type=int, default=256, help="image size of the comparison with forward_maps (0: skip it)")
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
    lines = ["%s, torch %s, HIP %s" % (torch.cuda.get_device_name(0), torch.__version__, torch.version.hip),
             "posed level set at %d^3; " % args.n_side + "; ".join("%s: %d vertices, %d faces" % (k, v.shape[0], f.shape[0])
                                                                   for k, (v, f) in meshes.items())]
    sizes = [int(s) for s in args.sizes.split(",")]
    with torch.no_grad():
        for size in sizes:
            # the frame's camera at this size (synthetic.make_inputs: focal 1.2 H, principal point at the image centre, R = I, t = 0)
            cam = {"cam_rot": inputs["cam_rot"][0], "cam_trans": inputs["cam_trans"][0].reshape(3),
                   "K": torch.tensor([[1.2 * size, 0, size / 2.0], [0, 1.2 * size, size / 2.0], [0, 0, 1]], device=dev)}
            drawn = {}
            for name, (v, f) in meshes.items():
                drawn[name] = (geometry.project_mesh(v, cam, size, size).contiguous(), f)
            uvz, f = drawn["(a) level set"]
            far = float(uvz[:, 2].max()) * 2.0
            quad = torch.tensor([[-1.0, -1.0, far], [size + 1.0, -1.0, far], [size + 1.0, size + 1.0, far], [-1.0, size + 1.0, far]], device=dev)
            V = uvz.shape[0]
            two = torch.tensor([[V, V + 1, V + 2], [V, V + 2, V + 3]], dtype=f.dtype, device=dev)
            drawn["(c) level set + 2 covering faces"] = (torch.cat([uvz, quad]).contiguous(), torch.cat([f, two]).contiguous())
            for name, (uvz, f) in drawn.items():
                soup = uvz[f.long()].contiguous()
                box = (soup[..., :2].max(1).values - soup[..., :2].min(1).values).clamp_min(0)
                area = ((box[:, 0] + 1) * (box[:, 1] + 1))
                lines.append("")
                lines.append("%d x %d  %s: %d faces; bounding boxes of about %.1f pixels in the median, %.0f at the most"
                             % (size, size, name, f.shape[0], float(area.median()), float(area.max().clamp_max(size * size))))
                routes = {"new   hip.mesh_rasterize (pass A + B, three outputs)": lambda: hip.mesh_rasterize(uvz, f, size, size),
                          "old   hip.rasterize on the soup (pix_to_face only)": lambda: hip.rasterize(soup, size, size)}
                spec_routes = {"spec  meshing.mesh_rasterize on the same tensors": lambda: meshing.mesh_rasterize(uvz, f, size, size)}
                t = run(routes, args.reps, spec_routes, args.spec_reps)
                for k in t:
                    lines.append("  %-64s %s" % (k, med(t[k])))
                new, old = (statistics.median(t[k]) for k in routes)
                lines.append("  old / new = %.2f x" % (old / new))
                got = hip.mesh_rasterize(uvz, f, size, size)
                if args.spec_reps:
                    want = meshing.mesh_rasterize(uvz, f, size, size)
                    same = all(torch.equal(a.view(torch.int32) if a.is_floating_point() else a,
                                           b.view(torch.int32) if b.is_floating_point() else b) for a, b in zip(got, want))
                    lines.append("  kernels against the specification at this size: %s" % ("bit-equal" if same else "DIFFER"))
                p_old = hip.rasterize(soup, size, size)
                lines.append("  pixels drawn: new %d, old %d; the same face in %.4f of the pixels either draws"
                             % (int((got[0] >= 0).sum()), int((p_old >= 0).sum()),
                                float((got[0].long() == p_old)[(got[0] >= 0) | (p_old >= 0)].float().mean())))
                if not args.no_sweep and not name.startswith("(c)"):
                    sweep, big = {}, 1 << 30
                    for small, wave, huge in ((16, 64, 4096), (0, 64, 4096), (4, 64, 4096), (64, 64, 4096), (16, 16, 4096), (16, 256, 4096),
                                              (16, 1024, 4096), (16, 4096, 4096), (16, 64, 1024), (16, 64, 16384), (16, 64, big),
                                              (16, big, big), (big, big, big)):
                        sweep["lane <= %d < wave <= %d < workgroup <= %d < 64 workgroups" % (small, wave, huge)] = \
                            (lambda s=small, w=wave, h=huge: hip.mesh_rasterize(uvz, f, size, size, thresholds=(s, w, h)))
                    t = run(sweep, args.reps)
                    for k in t:
                        lines.append("    %-84s %s" % (k, med(t[k])))
                if name.startswith("(a)"):
                    p2f, _, bary = got
                    for n_ch in (3, 24):
                        attr = torch.rand(uvz.shape[0], n_ch, device=dev)
                        t = run({"(d) hip.mesh_interpolate, %d channels" % n_ch: lambda: hip.mesh_interpolate(p2f, bary, f, attr)}, args.reps,
                                {"(d) meshing.interpolate_attributes, %d channels" % n_ch: lambda: meshing.interpolate_attributes(p2f, bary, f, attr)},
                                args.spec_reps)
                        for k in t:
                            lines.append("  %-64s %s" % (k, med(t[k])))
        if args.maps_size:
            # the volume render of the same frame: its rays go through the pixel CORNERS (u = x, v = y), so the mesh is drawn with the
            # principal point moved by half a pixel; depth_values is the distance along the unit ray, sum w t, acc_values sum w
            S = args.maps_size
            big = scene.make_inputs(S, S, frame_idx=0, device=dev)
            out = model.forward_maps(big, eval=True)
            acc, dist = out["acc_values"][0], out["depth_values"][0]
            K = big["intrinsics"][0].clone()
            K[0, 2] += 0.5
            K[1, 2] += 0.5
            res = geometry.render_mesh(verts, faces, S, S, camera={"cam_rot": big["cam_rot"][0], "cam_trans": big["cam_trans"][0].reshape(3),
                                                                    "K": K})
            rays = big["image_mask"][0].reshape(-1)
            vol = torch.zeros(S * S, dtype=torch.bool, device=dev)
            vol[rays] = acc > 0.5
            vol_z = torch.zeros(S * S, device=dev)
            vol_z[rays] = dist / acc.clamp_min(1e-6) * big["ray_dirs"][0][:, 2]      # distance along the ray -> view depth
            mesh_mask, mesh_z = res["mask"].reshape(-1), res["depth"].reshape(-1)
            both = vol & mesh_mask
            iou = float(both.sum()) / max(float((vol | mesh_mask).sum()), 1.0)
            lines.append("")
            lines.append("mesh against volume render at %d x %d: silhouette IoU %.4f (mesh %d, volume %d, both %d pixels); "
                         "median |depth difference| %.3g m, 95 %% below %.3g m"
                         % (S, S, iou, int(mesh_mask.sum()), int(vol.sum()), int(both.sum()),
                            float((mesh_z - vol_z)[both].abs().median()), float((mesh_z - vol_z)[both].abs().quantile(0.95))))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
