"""arah_image_metrics (csrc/metrics.hpp): PSNR and SSIM of an image pair on the device, held to a float64 restatement of the
reference's im2mesh/utils/eval.py:6-18 (scikit-image 0.18.1's structural_similarity + cv2.boundingRect) written here with
scipy.ndimage.uniform_filter.

Bounds (derived, not measured): both sides are float64 on the same fp32 pixels and differ only in the order of their sums
(<= 1e-16 relative per term; the variance's cancellation is amplified by at most 1 / C2 ~ 280 at R = 2), hence
|d ssim| <= 1e-10 and |d psnr| <= 1e-9 dB.  Against the float32 host formula of validation_step: float32 pairwise summation
of <= 1e6 terms is good to ~2e-6 relative, x 10 / ln 10 -> 1e-5 dB."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import REPO

gpu = pytest.mark.gpu
SSIM_TOL, PSNR_TOL, PSNR_HOST_TOL = 1e-10, 1e-9, 1e-5


# ---------------------------------------------------------------------------------------------- the float64 restatement
def bounding_rect(box):
    ys, xs = np.where(np.asarray(box) != 0)
    if len(ys) == 0:
        return 0, 0, 0, 0
    return int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)


def ssim_restatement(pred, gt, box, data_range=2.0):
    """ssim_metric (eval.py:11-18) with structural_similarity(multichannel=True) of scikit-image 0.18.1 spelled out: float64,
    7 x 7 uniform filter, sample covariance, the 3-pixel border cropped from the mean, mean over the channels."""
    from scipy.ndimage import uniform_filter
    x, y, w, h = bounding_rect(box)
    if w < 7 or h < 7:
        raise ValueError("win_size exceeds image extent")
    a = np.asarray(pred)[y:y + h, x:x + w].astype(np.float64)
    b = np.asarray(gt)[y:y + h, x:x + w].astype(np.float64)
    cov_norm = 49.0 / 48.0
    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    vals = []
    for c in range(3):
        X, Y = a[..., c], b[..., c]
        ux, uy = uniform_filter(X, size=7), uniform_filter(Y, size=7)
        uxx, uyy, uxy = uniform_filter(X * X, size=7), uniform_filter(Y * Y, size=7), uniform_filter(X * Y, size=7)
        vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
        S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
        vals.append(S[3:-3, 3:-3].mean(dtype=np.float64))
    return float(np.mean(vals))


def psnr_restatement(pred, gt, box):
    """psnr_metric (eval.py:6-9) over the ray list = the masked pixels, in float64."""
    m = np.asarray(box) != 0
    d = np.asarray(pred)[m].astype(np.float64) - np.asarray(gt)[m].astype(np.float64)
    mse = float(np.mean(d * d))
    return float("inf") if mse == 0 else -10.0 * np.log10(mse)


def psnr_host_formula(pred, gt, box):
    """What LightningModel.validation_step computes on the host today: float32 numpy on the (n, 3) ray list."""
    m = np.asarray(box) != 0
    p, g = np.asarray(pred, np.float32)[m], np.asarray(gt, np.float32)[m]
    with np.errstate(divide="ignore"):
        return float(-10 * np.log(np.mean((p - g) ** 2)) / np.log(10))


# ---------------------------------------------------------------------------------------------- inputs
def make_images(kind, H, W, seed=0):
    rng = np.random.RandomState(seed)
    if kind == "noise":
        return rng.rand(H, W, 3).astype(np.float32), rng.rand(H, W, 3).astype(np.float32)
    if kind == "identical":
        a = rng.rand(H, W, 3).astype(np.float32)
        return a, a.copy()
    assert kind == "render"          # black outside a blob, smooth colours inside, the prediction a perturbed ground truth
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    blob = ((yy - 0.5 * H) / (0.42 * H)) ** 2 + ((xx - 0.48 * W) / (0.3 * W)) ** 2 < 1
    gt = np.stack([0.5 + 0.4 * np.sin(xx / 9.0), 0.5 + 0.4 * np.cos(yy / 7.0), 0.3 + 0.2 * np.sin((xx + yy) / 13.0)], -1)
    gt = (gt * blob[..., None]).astype(np.float32)
    pred = np.clip(gt + 0.05 * rng.randn(H, W, 3) * blob[..., None], 0, 1).astype(np.float32)
    return pred, gt


def make_mask(kind, H, W, seed=0):
    m = np.zeros((H, W), bool)
    if kind == "full":
        m[:] = True
    elif kind == "left":
        m[H // 4:H - H // 4, 0:W // 2] = True
    elif kind == "right":
        m[H // 4:H - H // 4, W // 2:W] = True
    elif kind == "top":
        m[0:H // 2, W // 4:W - W // 4] = True
    elif kind == "bottom":
        m[H // 2:H, W // 4:W - W // 4] = True
    elif kind == "seven":                       # a 7 x 7 rectangle: exactly one window per channel
        m[H // 2 - 3:H // 2 + 4, W // 2 - 3:W // 2 + 4] = True
    elif kind == "odd":                         # neither extent a multiple of the 32 x 16 tile, origin off the tile grid
        m[3:min(H, 3 + 17), 5:min(W, 5 + 15)] = True
        if H > 64:
            m[3:3 + 16 * 3 + 9, 5:5 + 32 * 2 + 11] = True
    elif kind == "across":                      # a rectangle a few pixels either side of tile boundaries of the crop
        m[max(0, H // 2 - 13):min(H, H // 2 + 14), max(0, W // 2 - 9):min(W, W // 2 + 30)] = True
    elif kind == "sparse":                      # scattered pixels: the rectangle is set by its extremes, PSNR by the pixels
        rng = np.random.RandomState(seed)
        m[1:H - 2, 2:W - 1] = rng.rand(H - 3, W - 3) < 0.03
        m[1, 2] = m[H - 3, W - 2] = True
    else:
        raise ValueError(kind)
    return m


def run(pred, gt, box, data_range=2.0):
    from arah_release_amd import hip
    dev = torch.device("cuda:0")
    out, rect = hip.image_metrics(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev), torch.from_numpy(box).to(dev),
                                  data_range=data_range)
    assert out.dtype == torch.float64 and out.is_cuda and rect.dtype == torch.int32 and rect.is_cuda
    return out.cpu().numpy(), rect.cpu().numpy()


def check_against_restatement(pred, gt, box, data_range, label):
    out, rect = run(pred, gt, box, data_range)
    want_rect = bounding_rect(box)
    want_ssim, want_psnr = ssim_restatement(pred, gt, box, data_range), psnr_restatement(pred, gt, box)
    d_ssim = abs(out[1] - want_ssim)
    d_psnr = 0.0 if (np.isinf(want_psnr) and out[0] == want_psnr) else abs(out[0] - want_psnr)
    host = psnr_host_formula(pred, gt, box)
    d_host = 0.0 if (np.isinf(host) and out[0] == host) else abs(out[0] - host)
    print("%-40s ssim %.15f (d %.2e)  psnr %.10f dB (d %.2e, vs host f32 %.2e)  rect %s" %
          (label, out[1], d_ssim, out[0], d_psnr, d_host, tuple(rect)))
    assert tuple(rect[:4]) == want_rect and rect[4] == 0, (label, tuple(rect), want_rect)
    assert out[3] == np.count_nonzero(box)
    assert d_ssim <= SSIM_TOL, (label, out[1], want_ssim)
    assert d_psnr <= PSNR_TOL, (label, out[0], want_psnr)
    assert d_host <= PSNR_HOST_TOL, (label, out[0], host)
    return out


SIZES = [(24, 20), (128, 128), (512, 512), (1002, 1000)]
MASKS = ["full", "left", "right", "top", "bottom", "seven", "odd", "across", "sparse"]


# ---------------------------------------------------------------------------------------------- CPU
def test_restatement_valid_windows_equal_filtered_and_cropped():
    """The kernel's form -- only windows wholly inside the crop -- is the restatement's uniform_filter (reflect) + 3-pixel crop."""
    for H, W in ((7, 7), (24, 20), (301, 187)):
        pred, gt = make_images("noise", H, W, seed=H)
        a, b = pred.astype(np.float64), gt.astype(np.float64)
        vals = []
        for c in range(3):
            win = lambda z: np.lib.stride_tricks.sliding_window_view(z, (7, 7)).mean(axis=(2, 3))
            X, Y = a[..., c], b[..., c]
            ux, uy, uxx, uyy, uxy = win(X), win(Y), win(X * X), win(Y * Y), win(X * Y)
            k = 49.0 / 48.0
            vx, vy, vxy = k * (uxx - ux * ux), k * (uyy - uy * uy), k * (uxy - ux * uy)
            C1, C2 = 0.02 ** 2, 0.06 ** 2
            vals.append((((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))).mean())
        assert abs(np.mean(vals) - ssim_restatement(pred, gt, np.ones((H, W), bool), 2.0)) <= 1e-13


def test_shipped_metric_kernels_do_not_spill(tmp_path):
    """The code object's notes: no private segment (scratch) and no spilled registers in the four kernels of metrics.hpp."""
    import shutil
    import __graft_entry__
    objdump, readelf = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("llvm-objdump / llvm-readelf not found")
    __graft_entry__.build()
    lib = shutil.copy(os.path.join(REPO, "arah_release_amd", "libarah_hip.so"), tmp_path / "lib.so")
    subprocess.run([objdump, "--offloading", str(lib)], check=True, capture_output=True, cwd=tmp_path)
    cos = [f for f in os.listdir(tmp_path) if "gfx950" in f]
    assert len(cos) == 1, cos
    notes = subprocess.run([readelf, "--notes", str(tmp_path / cos[0])], check=True, capture_output=True, text=True).stdout
    seg = re.findall(r"\.name:\s+(\S*k_metrics_\S*)\s+\.private_segment_fixed_size:\s+(\d+)", notes)
    assert sorted(re.search(r"k_metrics_[a-z]+", n).group(0) for n, _ in seg) == \
        ["k_metrics_finish", "k_metrics_mse", "k_metrics_rect", "k_metrics_ssim"], seg
    assert all(int(b) == 0 for _, b in seg), seg
    for name, _ in seg:
        block = notes[notes.index(name):]
        block = block[:block.index(".wavefront_size")]
        assert re.search(r"\.vgpr_spill_count:\s+0\b", block) and re.search(r"\.sgpr_spill_count:\s+0\b", block), block


# ---------------------------------------------------------------------------------------------- GPU
@gpu
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_metrics_match_float64_restatement(size):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    H, W = size
    k = 0
    for mask_kind in MASKS:
        box = make_mask(mask_kind, H, W, seed=k)
        for img_kind in ("noise", "render"):
            for R in (2.0, 1.0):
                if (H, W) == (1002, 1000) and (img_kind, R) not in (("noise", 2.0), ("render", 1.0)):
                    continue            # the large size takes two of the four combinations per mask (host time of the restatement)
                pred, gt = make_images(img_kind, H, W, seed=k)
                check_against_restatement(pred, gt, box, R, "%dx%d %s %s R=%g" % (H, W, mask_kind, img_kind, R))
                k += 1


@gpu
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_identical_images_give_ssim_one_and_infinite_psnr(size):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    H, W = size
    for mask_kind in ("full", "across", "sparse"):
        for R in (2.0, 1.0):
            pred, gt = make_images("identical", H, W, seed=3)
            out = check_against_restatement(pred, gt, make_mask(mask_kind, H, W), R, "%dx%d %s identical R=%g" % (H, W, mask_kind, R))
            assert abs(out[1] - 1.0) <= 1e-15 and out[0] == np.inf and out[2] == 0.0


@gpu
def test_rectangle_and_status():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    rng = np.random.RandomState(5)
    for trial in range(12):                                          # random sparse masks: numpy's min / max
        H, W = int(rng.randint(8, 200)), int(rng.randint(8, 200))
        box = rng.rand(H, W) < rng.choice([0.002, 0.02, 0.3])
        pred, gt = make_images("noise", H, W, seed=trial)
        out, rect = run(pred, gt, box)
        x, y, w, h = bounding_rect(box)
        n = np.count_nonzero(box)
        want_status = 1 if n == 0 else (2 if (w < 7 or h < 7) else 0)
        assert tuple(rect) == (x, y, w, h, want_status), (trial, tuple(rect), (x, y, w, h, want_status))
        assert out[3] == n
        if want_status == 0:
            assert abs(out[1] - ssim_restatement(pred, gt, box)) <= SSIM_TOL
        if n:
            assert abs(out[0] - psnr_restatement(pred, gt, box)) <= PSNR_TOL
    H, W = 40, 52
    pred, gt = make_images("noise", H, W, seed=1)
    for (py, px) in ((0, 0), (H - 1, W - 1), (17, 33)):              # single pixels
        box = np.zeros((H, W), bool)
        box[py, px] = True
        out, rect = run(pred, gt, box)
        assert tuple(rect) == (px, py, 1, 1, 2) and np.isnan(out[1]) and out[3] == 1
        assert abs(out[0] - psnr_restatement(pred, gt, box)) <= PSNR_TOL
    out, rect = run(pred, gt, np.zeros((H, W), bool))               # empty mask
    assert tuple(rect) == (0, 0, 0, 0, 1) and np.isnan(out[0]) and np.isnan(out[1]) and out[3] == 0
    for shape in ((slice(5, 30), slice(10, 16)), (slice(20, 26), slice(3, 40))):    # 6 wide / 6 high
        box = np.zeros((H, W), bool)
        box[shape] = True
        out, rect = run(pred, gt, box)
        assert rect[4] == 2 and tuple(rect[:4]) == bounding_rect(box) and np.isnan(out[1])
        assert abs(out[0] - psnr_restatement(pred, gt, box)) <= PSNR_TOL
        with pytest.raises(ValueError):
            ssim_restatement(pred, gt, box)
    # the Python layer raises when such a result is READ, not when it is launched
    from arah_release_amd import hip
    dev = torch.device("cuda:0")
    o, r = hip.image_metrics(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev), torch.from_numpy(box).to(dev))
    with pytest.raises(ValueError):
        hip.read_image_metrics(o, r)
    full = hip.read_image_metrics(*hip.image_metrics(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev),
                                                     torch.ones(H, W, dtype=torch.bool, device=dev)))
    assert full["rect"] == (0, 0, W, H) and full["n"] == H * W and abs(full["ssim"] - ssim_restatement(pred, gt, np.ones((H, W)))) <= SSIM_TOL


@gpu
def test_bit_reproducible_across_calls_and_streams_and_blind_outside_the_rectangle():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from arah_release_amd import hip
    dev = torch.device("cuda:0")
    H, W = 512, 512
    pred, gt = make_images("render", H, W, seed=7)
    box = make_mask("across", H, W)
    box[200:330, 180:400] = True
    other = [torch.from_numpy(a).to(dev) for a in make_images("noise", 1002, 1000, seed=8)]
    other_box = torch.ones(1002, 1000, dtype=torch.bool, device=dev)
    P, G, B = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev), torch.from_numpy(box).to(dev)
    results = [hip.image_metrics(P, G, B) for _ in range(3)]
    side = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    busy = [hip.image_metrics(other[0], other[1], other_box) for _ in range(4)]      # another frame's calls in flight on this stream
    with torch.cuda.stream(side):
        results.append(hip.image_metrics(P, G, B))
    torch.cuda.synchronize()
    first = (results[0][0].cpu().numpy().tobytes(), results[0][1].cpu().numpy().tobytes())
    for o, r in results[1:]:
        assert (o.cpu().numpy().tobytes(), r.cpu().numpy().tobytes()) == first
    assert all(torch.equal(b[0], busy[0][0]) for b in busy)
    # nothing outside the crop is read: NaN there changes no bit of the result
    x, y, w, h = bounding_rect(box)
    pn, gn = np.full_like(pred, np.nan), np.full_like(gt, np.nan)
    pn[y:y + h, x:x + w], gn[y:y + h, x:x + w] = pred[y:y + h, x:x + w], gt[y:y + h, x:x + w]
    o, r = hip.image_metrics(torch.from_numpy(pn).to(dev), torch.from_numpy(gn).to(dev), B)
    assert (o.cpu().numpy().tobytes(), r.cpu().numpy().tobytes()) == first
    assert abs(float(o[1]) - ssim_restatement(pred, gt, box)) <= SSIM_TOL


@gpu
def test_abi_errors_launch_nothing():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from arah_release_amd import hip
    lib = hip.load_library()
    dev = torch.device("cuda:0")
    H, W = 32, 48
    P, G = torch.rand(H, W, 3, device=dev), torch.rand(H, W, 3, device=dev)
    B = torch.ones(H, W, dtype=torch.uint8, device=dev)
    out = torch.full((4,), -7.0, dtype=torch.float64, device=dev)
    rect = torch.full((5,), -7, dtype=torch.int32, device=dev)
    nbytes = int(lib.arah_image_metrics_bytes(H, W))
    assert nbytes > 0 and lib.arah_image_metrics_bytes(0, W) == 0 and lib.arah_image_metrics_bytes(H, -1) == 0
    scratch = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call(pred=P, gt=G, box=B, h=H, w=W, R=2.0, o=out, r=rect, s=scratch, n=nbytes):
        return lib.arah_image_metrics(p(pred) if pred is not None else None, p(gt) if gt is not None else None,
                                      p(box) if box is not None else None, C.c_int32(h), C.c_int32(w), C.c_double(R),
                                      p(o) if o is not None else None, p(r) if r is not None else None,
                                      p(s) if s is not None else None, C.c_size_t(n), stream)

    E_BADARG, E_WORKSPACE = -1, -3
    for kw in (dict(pred=None), dict(gt=None), dict(box=None), dict(o=None), dict(r=None), dict(s=None), dict(h=0), dict(w=0),
               dict(h=-3), dict(R=0.0)):
        assert call(**kw) == E_BADARG, kw
    assert call(n=nbytes - 1) == E_WORKSPACE and call(n=0) == E_WORKSPACE
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((rect == -7).all()) and int(scratch.sum()) == 0      # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert float(out[3]) == H * W and rect.tolist() == [0, 0, W, H, 0]
