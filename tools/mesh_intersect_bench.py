"""Cost of finding the self-intersections of indexed meshes on the device (hip.mesh_intersections; geometry.self_intersections),
against the index build alone and against the chunked brute-force specification on the same device tensors.

    python tools/mesh_intersect_bench.py [--n-side 256] [--reps 20] [--spec-reps 1] [--spec-max-faces 120000] [--out profiles/mesh_intersect_bench.txt]

The synthetic subject at n_side^3: (a) the posed level set as an indexed mesh (posed_mesh(indexed=True): the level set of the posed
SDF), (b) its skinned counterpart, the canonical level set skinned forward (canonical_mesh(...)["verts_posed"]: what render_mesh and
cast_rays work on), and (c) geometry.simplify_mesh of (b) with cells of 2 and 4 lattice steps, position "mean" and "quadric".  After
warm-up, with device events around the whole calls: median, min and max, all in one session.

    kernel  hip.mesh_intersections with the quantisation given and trim=False: the allocation of the outputs and the launches, no host
            read; at the default max_pairs and with max_pairs=0 (no pair list: the count pass alone)
    whole   geometry.self_intersections: the bounds' host read, the kernels, the counts' host read
    index   hip.mesh_index of the quantised soup alone (the kernel builds the same index inside its scratch)
    spec    meshing.mesh_intersections on the same tensors, chunked to 2^26 pairs of temporaries; --spec-reps calls after one warm-up
            call on a slice of the faces; for meshes of at most --spec-max-faces faces (it is F^2 box tests)

and, per mesh: the pairs, the faces and vertices hit, the pairs that reach the six tests per face (both sides counted), the index's
grid and big list, and whether kernel and specification agree bit for bit."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SPEC_CHUNK = 1 << 26


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-side", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--spec-reps", type=int, default=1)
    ap.add_argument("--spec-max-faces", type=int, default=120000)
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
        skinned = model.canonical_mesh(inputs, n_side=args.n_side, attributes=("verts_posed",))
    lattice_step = float(posed["box"][3]) / (args.n_side - 1)
    sv, sf = skinned["verts_posed"].contiguous(), skinned["faces"].contiguous()
    meshes = {"(a) posed level set": (posed["verts"].contiguous(), posed["faces"].contiguous()), "(b) skinned canonical level set": (sv, sf)}
    for k in (2, 4):
        for position in ("mean", "quadric"):
            s = geometry.simplify_mesh(sv, sf, cell=k * lattice_step, position=position)
            meshes["(c) cells of %d steps, %s" % (k, position)] = (s["verts"].contiguous(), s["faces"].contiguous())
    lines = []

    def say(line=""):
        lines.append(line)
        print(line, flush=True)
    say("%s, torch %s, HIP %s" % (torch.cuda.get_device_name(0), torch.__version__, torch.version.hip))
    say("the synthetic subject at %d^3, lattice step %.5f m" % (args.n_side, lattice_step))
    with torch.no_grad():
        for name, (v, f) in meshes.items():
            v = v.to(torch.float32).contiguous()
            F = int(f.shape[0])
            quant = meshing.orient_quant(v)
            q, void = meshing.intersect_soup(v, f, quant)
            soup = q.float().contiguous()
            hdr = hip.mesh_index(soup).header()
            say("")
            say("%s: %d vertices, %d faces, grid %s, %d references, %d on the big list" % (name, v.shape[0], F, hdr["n"], hdr["n_refs"], hdr["n_big"]))
            routes = {"kernel  hip.mesh_intersections, quant given, no host read": lambda: hip.mesh_intersections(v, f, quant=quant, trim=False),
                      "kernel  the same, max_pairs=0 (counts only)": lambda: hip.mesh_intersections(v, f, quant=quant, max_pairs=0, trim=False),
                      "whole   geometry.self_intersections": lambda: geometry.self_intersections(v, f),
                      "index   hip.mesh_index of the quantised soup": lambda: hip.mesh_index(soup)}
            t = run(routes, args.reps)
            for k in t:
                say("  %-64s %s" % (k, med(t[k])))
            got = hip.mesh_intersections(v, f, quant=quant, want_tested=True)
            c = got[4].tolist()
            rows = got[2][1:] - got[2][:-1]
            say("  %d pairs on %d faces and %d vertices, %d void faces; %.2f pairs reach the six tests per face; longest row %d"
                % (c[0], c[1], c[2], c[3], int(got[5]) / max(F, 1), int(rows.max()) if F else 0))
            kernel = statistics.median(t["kernel  hip.mesh_intersections, quant given, no host read"])
            say("  kernel / index build = %.1f x" % (kernel / statistics.median(t["index   hip.mesh_index of the quantised soup"])))
            if args.spec_reps and F <= args.spec_max_faces:
                meshing.mesh_intersections(v, f[:2048], quant=quant, chunk_pairs=SPEC_CHUNK)        # warm-up on a slice
                torch.cuda.synchronize()
                ts, want = [], None
                for _ in range(args.spec_reps):
                    ms, want = timed(lambda: meshing.mesh_intersections(v, f, quant=quant, chunk_pairs=SPEC_CHUNK))
                    ts.append(ms)
                say("  %-64s %s" % ("spec    meshing.mesh_intersections, chunked", med(ts)))
                same = all(a.shape == b.shape and torch.equal(a, b) for a, b in zip(got[:5], want))
                say("  spec / kernel = %.0f x; kernel against the specification: %s" % (statistics.median(ts) / kernel, "bit-equal" if same else "DIFFER"))
            elif args.spec_reps:
                say("  spec    skipped: more than %d faces" % args.spec_max_faces)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
