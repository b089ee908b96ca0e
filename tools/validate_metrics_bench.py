"""Cost of the device-side validation metrics (hip.image_metrics / LightningModel.validation_step(metrics="device")).

    python tools/validate_metrics_bench.py [--frames 20] [--passes 5] [--out profiles/validate_metrics.txt]

1. arah_image_metrics alone, full-image rectangle, at 512 x 512 and 1002 x 1000: median of 100 calls after 20 warm-up calls,
   (i) device events around one call, (ii) host clock over 100 back-to-back calls ending in a synchronise, per call.
2. Twenty frames of the benchmark workload (512^2 pixels x 64 samples, bench.py's frames) through renderer.map_in_flight,
   passes alternating on one box: (a) LightningModel.render_image only, (b) validation_step(metrics="device"),
   (c) validation_step(ssim_fn=<float64 SSIM through scipy.ndimage.uniform_filter>), the host route.  ms per frame per pass,
   their medians and the pass-to-pass spread of each variant."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_ssim(pred, gt, box, data_range=2.0):
    """scikit-image 0.18.1's structural_similarity (multichannel, float64) on the mask's bounding rectangle."""
    from scipy.ndimage import uniform_filter
    ys, xs = np.where(box != 0)
    a = pred[ys.min():ys.max() + 1, xs.min():xs.max() + 1].astype(np.float64)
    b = gt[ys.min():ys.max() + 1, xs.min():xs.max() + 1].astype(np.float64)
    C1, C2, k, vals = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2, 49.0 / 48.0, []
    for c in range(3):
        X, Y = a[..., c], b[..., c]
        ux, uy = uniform_filter(X, size=7), uniform_filter(Y, size=7)
        uxx, uyy, uxy = uniform_filter(X * X, size=7), uniform_filter(Y * Y, size=7), uniform_filter(X * Y, size=7)
        vx, vy, vxy = k * (uxx - ux * ux), k * (uyy - uy * uy), k * (uxy - ux * uy)
        S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
        vals.append(S[3:-3, 3:-3].mean())
    return float(np.mean(vals))


def kernel_alone(dev, H, W, calls=100, warmup=20):
    from arah_release_amd import hip
    gen = torch.Generator(device=dev).manual_seed(0)
    pred, gt = torch.rand(H, W, 3, device=dev, generator=gen), torch.rand(H, W, 3, device=dev, generator=gen)
    box = torch.ones(H, W, dtype=torch.bool, device=dev)
    for _ in range(warmup):
        hip.image_metrics(pred, gt, box)
    torch.cuda.synchronize()
    ev = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        hip.image_metrics(pred, gt, box)
        b.record()
        b.synchronize()
        ev.append(1e3 * a.elapsed_time(b))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        hip.image_metrics(pred, gt, box)
    torch.cuda.synchronize()
    host = 1e6 * (time.perf_counter() - t0) / calls
    return ("arah_image_metrics %4d x %4d full rectangle: device events median %.1f us (min %.1f, max %.1f) over %d calls; "
            "host clock %.1f us per call over %d back-to-back calls" % (H, W, statistics.median(ev), min(ev), max(ev), calls, host,
                                                                         calls))


def frames_in_flight(dev, n_frames, passes):
    from arah_release_amd import config, renderer, synthetic
    model, cfg = config.build_synthetic_model("zju377_mono", 64, 16, 16, device=dev)
    lm = config.LightningModel(model, cfg).eval()
    lm.compose_inputs = lambda data, eval: data["model_inputs"]       # bench.py's frames are composed model inputs
    scene = synthetic.SyntheticScene(0)
    items = []
    gen = torch.Generator(device=dev).manual_seed(1)
    for k in range(n_frames):
        inp = scene.make_inputs(512, 512, frame_idx=k, device=dev)
        n = int(inp["ray_dirs"].shape[1])
        items.append({"model_inputs": inp, "inputs.image_mask": inp["image_mask"],
                      "inputs": torch.rand(1, n, 3, device=dev, generator=gen)})
    variants = {"a render_image only": lambda it: lm.render_image(it),
                "b validation_step(metrics='device')": lambda it: lm.validation_step(it, metrics="device"),
                "c validation_step(ssim_fn=float64 host SSIM)": lambda it: lm.validation_step(it, ssim_fn=host_ssim)}
    for fn in variants.values():                                         # warm-up: every shape, every variant
        renderer.map_in_flight(fn, items[:4], owner=lm.model)
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(passes):
        for name, fn in variants.items():                                # alternating
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs = renderer.map_in_flight(fn, items, owner=lm.model)
            torch.cuda.synchronize()
            times[name].append(1e3 * (time.perf_counter() - t0) / n_frames)
            del outs
    lines = ["%d frames 512^2 x 64 through map_in_flight (%d in flight), %d alternating passes, ms per frame:" %
             (n_frames, renderer.frames_in_flight(n_frames), passes)]
    for name, t in times.items():
        lines.append("  (%s) median %.2f  min %.2f  max %.2f  passes %s" % (name, statistics.median(t), min(t), max(t),
                                                                             " ".join("%.2f" % v for v in t)))
    med = {k: statistics.median(v) for k, v in times.items()}
    a, b, c = (med[k] for k in variants)
    lines.append("  (b) - (a) = %+.2f ms per frame; spread of (a) over its passes %.2f ms; (c) / (b) = %.2f x, (c) - (a) = %+.2f ms" %
                 (b - a, max(times[list(variants)[0]]) - min(times[list(variants)[0]]), c / b, c - a))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    lines = ["%s, torch %s, HIP %s" % (torch.cuda.get_device_name(0), torch.__version__, torch.version.hip)]
    lines.append(kernel_alone(dev, 512, 512))
    lines.append(kernel_alone(dev, 1002, 1000))
    lines += frames_in_flight(dev, args.frames, args.passes)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
