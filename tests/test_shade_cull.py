"""The shading cull of loop D (ArahSampling.shade_cull; csrc/arah_hip.hip: k_shade_split, k_composite_cull).

Exact lazy shading shades every sample with density > 0.  Deep behind the surface w = alpha * trans is below half an ulp of
the accumulated colour, r += c * w returns r whatever c in [0, 1] is, and the sample's normal and colour are dead values.  The
cull guesses those samples from the densities (`ws + 8 w == ws`), leaves them unshaded, and the compositing walk verifies the
guess on its own accumulators (`r + 2 w == r`, and g, b); a ray that fails has its tail shaded after all and is composited
again.  What must hold: the image with the cull equals the image without it BIT FOR BIT, on either path, whatever the guess
was worth -- and n_col + n_shade_culled = the number of sigma > 0 samples.
"""
import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu


# ---- CPU: the inequality the check rests on ----------------------------------------------------------------------------------
def test_a_passed_check_means_the_colour_cannot_change_the_sum():
    """r >= 0, w >= 0, c in [0, 2] (fp32): whenever fl(r + 2 w) == r, both fl(r + fl(c w)) and the fused fl(r + c w) are r.
    The fused form is emulated in float64: c w (two 24-bit factors) is exact there, and r + c w is at most half an ulp of r
    above r and -- when r is odd, where the tie would round up -- away from that midpoint by more than 2^-24 of it (2 w is an
    fp32 number strictly below the midpoint), so the float64 sum's own rounding cannot carry it across."""
    rng = np.random.default_rng(7)
    n = 400000
    f32 = np.float32
    r = (rng.uniform(1.0, 2.0, n) * 2.0 ** rng.integers(-60, 2, n)).astype(f32)
    r[:1000] = 0.0
    # weights around the threshold: 2 w from a quarter of an ulp of r to two ulps, plus exact zeros and exact midpoints
    w = (r * 2.0 ** rng.uniform(-28.0, -23.0, n)).astype(f32)
    w[1000:2000] = 0.0
    w[2000:3000] = (np.spacing(r[2000:3000]) / f32(4.0)).astype(f32)   # 2 w = half an ulp: the tie
    w[:1000] = (rng.uniform(0, 1e-30, 1000) * (rng.uniform(0, 1, 1000) < 0.5)).astype(f32)   # r = 0: only w = 0 passes
    c = rng.uniform(0.0, 2.0, n).astype(f32)
    c[::7] = 2.0
    c[1::7] = 0.0
    c[2::7] = np.nextafter(f32(1.0), f32(2.0))   # a sigmoid that rounds a hair above 1
    passed = (r + f32(2.0) * w).astype(f32) == r
    assert 10000 < int(passed.sum()) < n - 10000   # both sides of the threshold are populated
    plain = (r + (c * w).astype(f32)).astype(f32)
    fused = (r.astype(np.float64) + c.astype(np.float64) * w.astype(np.float64)).astype(f32)
    assert np.array_equal(plain[passed], r[passed])
    assert np.array_equal(fused[passed], r[passed])
    # ... and the check is not vacuous: among the samples that fail it some colours do change the sum
    assert int((plain[~passed] != r[~passed]).sum()) > 1000


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def _subject(scene, name, beta, S=64, hw=64, frame_idx=4, bias=None):
    """(frame, cam, dirs, near_far, pose, cano_view_dirs) of `name` at VolSDF beta; bias: added to the colour head's last-layer
    bias (3 values).  Built once per key and left unchanged."""
    from arah_release_amd import config, renderer
    key = (name, beta, S, hw, frame_idx, bias)
    if key not in _CACHE:
        dev = torch.device("cuda:0")
        model, cfg = config.build_synthetic_model(name, S, 16 if S >= 33 else 8, 16 if S >= 33 else 8, device=dev)
        inputs = scene.make_inputs(hw, hw, frame_idx=frame_idx, device=dev)
        with torch.no_grad():
            model.deviation_decoder.variance.fill_(beta)
            if bias is not None:
                model.color_decoder.lin5.bias.add_(torch.tensor(bias, device=dev))
            renderer.invalidate_caches(model)
            dec = model.sdf_decoder({"coords": torch.zeros(1, 1, 3, device=dev), "rots": inputs["rots"][:1],
                                     "Jtrs": inputs["Jtrs"][:1], "latent": model.latent(inputs["geo_latent_code_idx"])})
            pose_cond = dict(inputs["pose_cond"])
            pose_cond["latent_code"] = model.latent(pose_cond["latent_code_idx"])
            frame = renderer.build_frame(dec["decoder"], model.skinning_model, model.color_decoder,
                                         model.deviation_decoder, pose_cond, inputs["smpl_verts"],
                                         inputs["skinning_weights"], inputs["bone_transforms"], inputs["trans"],
                                         inputs["coord_min"], inputs["coord_max"], inputs["center"])
        pose = torch.eye(4, device=dev)[:3].contiguous()
        _CACHE[key] = (frame, inputs["cam_loc"], inputs["ray_dirs"][0].contiguous(),
                       inputs["body_bounds_intersections"][0].contiguous(), pose, cfg["model"]["cano_view_dirs"], model)
    return _CACHE[key][:6]


def _render(sub, S, cull, tiered=False, last=False, rays=None, ws=None):
    """hip.render of the subject's rays (or of the subset `rays`): (rgb, points_cam, vol_mask, acc), counters, workspace."""
    from arah_release_amd import hip
    frame, cam, d, nf, pose, cano = sub
    dev = d.device
    if rays is not None:
        d, nf = d[rays].contiguous(), nf[rays].contiguous()
    near = 16 if S >= 33 else 8
    samp = hip.Sampling(dev, S, near, near, cano, last, shade_cull=cull)
    ws = ws if ws is not None else hip.Workspace(dev)
    ws.ensure(d.shape[0], S)
    ws.reset_counters()
    rgb, pcam, vol, acc, _, _ = hip.render(frame, ws, samp, cam, d, nf, pose, tiered=tiered)
    torch.cuda.synchronize()
    return (rgb, pcam, vol, acc), ws.counters(), ws


def _assert_equal(on, off, label):
    for name, a, b in zip(("rgb", "points_cam", "mask", "acc"), on, off):
        assert torch.equal(a, b), "%s: %s differs on %d rays" % (label, name, int((a != b).reshape(a.shape[0], -1).any(-1).sum()))


@gpu
@pytest.mark.parametrize("beta", [1e-3, 3e-3, 1e-2])
@pytest.mark.parametrize("name", ["zju377_mono", "h36m"])
def test_cull_on_equals_cull_off(scene, name, beta):
    """64 x 64 rays x 64 samples, both subjects (h36m: the IDR colour network), render_last_pt both ways, tiered and untiered:
    rgb, acc, mask and points_cam are equal, and the samples the cull sets aside are exactly the ones missing from n_col."""
    sub = _subject(scene, name, beta)
    n_col = set()
    for last in (False, True):
        for tiered in (False, True):
            label = "%s beta %g last %d tiered %d" % (name, beta, last, tiered)
            off, c_off, ws = _render(sub, 64, False, tiered, last)
            on, c_on, _ = _render(sub, 64, True, tiered, last, ws=ws)
            print(label, "n_col off %d, on %d, culled %d, rescued %d" % (c_off["n_col"], c_on["n_col"], c_on["n_shade_culled"],
                                                                        c_on["n_shade_rescued"]))
            _assert_equal(on, off, label)
            assert c_off["n_shade_culled"] == 0 and c_off["n_shade_rescued"] == 0, label
            assert c_on["n_col"] + c_on["n_shade_culled"] == c_off["n_col"], label
            assert c_off["n_col"] > 0
            if beta == 1e-3:
                assert c_on["n_shade_culled"] > 0, label
            n_col.add((last, c_on["n_col"]))
    assert len(n_col) == 2   # the tiered and the untiered forward decide alike (one count per render_last_pt)


@gpu
@pytest.mark.parametrize("bias,partial", [((-40.0, 0.0, 0.0), False), ((0.0, -4.0, 0.0), True)])
def test_the_rescue_path_runs_and_restores_the_image(scene, bias, partial):
    """A colour head whose last-layer bias of one channel is pushed down: that channel's running colour is far below the eighth
    of the weight sum the guess assumes, the check on it must fail and the tails are shaded after all -- the image is still
    the uncut one bit for bit.  Bias -40 (colour 4e-18): every ray with a tail fails.  Bias -4 (colour about 1/60 of the weight
    sum, where the guess assumes 1/8): a tail fails only if its weight lies in the factor-8 band between the two thresholds,
    while successive tail weights are a factor of several hundred apart -- some rays are rescued, the others keep their cull."""
    sub = _subject(scene, "zju377_mono", 1e-3, bias=bias)
    for tiered in (False, True):
        off, c_off, ws = _render(sub, 64, False, tiered)
        on, c_on, _ = _render(sub, 64, True, tiered, ws=ws)
        print("bias", bias, "tiered", tiered, "n_col off %d, on %d, culled %d, rescued %d" % (
            c_off["n_col"], c_on["n_col"], c_on["n_shade_culled"], c_on["n_shade_rescued"]))
        _assert_equal(on, off, "bias %s tiered %d" % (bias, tiered))
        assert c_on["n_shade_rescued"] > 0
        assert c_on["n_col"] + c_on["n_shade_culled"] == c_off["n_col"]
        if partial:
            assert c_on["n_shade_culled"] > 0
        else:
            assert c_on["n_shade_culled"] == 0


@gpu
def test_small_and_odd_ray_sets(scene):
    """One ray (a surface ray with tail samples), and 131 rays (partial waves and a partial block), tiered and untiered."""
    sub = _subject(scene, "zju377_mono", 1e-3)
    _, _, ws = _render(sub, 64, False)
    _, pos = ws.tier_debug(sub[2].shape[0], 64)   # (the rays of the 64 x 64 image that meet the body's box)
    hit = torch.nonzero(pos == 1).reshape(-1)
    assert hit.numel() > 131
    one = hit[hit.numel() // 2: hit.numel() // 2 + 1]
    start = max(int(hit[0]) - 3, 0)   # a run of consecutive pixels that starts outside the body and enters it
    some = torch.arange(start, start + 131, device=hit.device)
    for rays, label in ((one, "one ray"), (some, "131 rays")):
        for tiered in (False, True):
            off, c_off, w2 = _render(sub, 64, False, tiered, rays=rays)
            on, c_on, _ = _render(sub, 64, True, tiered, rays=rays, ws=w2)
            _assert_equal(on, off, label)
            assert c_on["n_col"] + c_on["n_shade_culled"] == c_off["n_col"] and c_on["n_shade_culled"] > 0, label


@gpu
def test_steps_off_the_chunked_walk(scene):
    """n_steps = 36 is no multiple of 8: the compositing kernels walk sample by sample instead of by 128-byte lines."""
    sub = _subject(scene, "zju377_mono", 1e-3, S=36)
    for tiered in (False, True):
        off, c_off, ws = _render(sub, 36, False, tiered)
        on, c_on, _ = _render(sub, 36, True, tiered, ws=ws)
        _assert_equal(on, off, "36 steps, tiered %d" % tiered)
        assert c_on["n_col"] + c_on["n_shade_culled"] == c_off["n_col"] and c_on["n_shade_culled"] > 0


@gpu
def test_crafted_masks_through_shade_composite(scene):
    """arah_shade_composite on the samples of a rendered frame with masks cut down to the walk's corner cases: rays with a
    single valid sample, a frame without any sigma > 0 sample (empty head list), rays whose sigma > 0 samples are all head."""
    from arah_release_amd import hip
    sub = _subject(scene, "zju377_mono", 1e-3)
    frame, cam, d, nf, pose, cano = sub
    dev, N, S = d.device, d.shape[0], 64
    _, _, ws = _render(sub, S, False)
    smp = {k: v.clone() for k, v in ws.debug_samples(N, S, which=("z", "pts", "T", "mask")).items()}
    z, pts, T, mask = smp["z"].reshape(N, S), smp["pts"], smp["T"], smp["mask"].reshape(N, S)

    def both(m):
        res = []
        for cull in (False, True):
            samp = hip.Sampling(dev, S, 16, 16, cano, False, shade_cull=cull)
            ws.reset_counters()
            out = hip.shade_composite(frame, ws, samp, d, z, pts, T, m.contiguous())
            torch.cuda.synchronize()
            res.append((out, ws.counters()))
        (off, c_off), (on, c_on) = res
        for a, b in zip(on, off):
            assert torch.equal(a, b)
        assert c_on["n_col"] + c_on["n_shade_culled"] == c_off["n_col"]
        return c_off, c_on

    c_off, c_on = both(mask)   # the whole frame through this entry point: its densities come from the kernels used below
    assert c_on["n_shade_culled"] > 0
    sigma = ws.debug_samples(N, S, which=("shaded",))["shaded"][:, 3].reshape(N, S).clone()
    pos = (mask != 0) & (sigma > 0)
    assert int(pos.sum()) == c_off["n_col"]
    order = torch.cumsum(pos.int(), dim=1)
    first = (pos & (order == 1)).to(torch.uint8)
    c_off, c_on = both(first)                       # a single valid sample per ray, with sigma > 0
    assert c_off["n_col"] == int(first.sum()) > 0
    c_off, c_on = both(((mask != 0) & ~pos).to(torch.uint8))   # no sigma > 0 sample at all
    assert c_off["n_col"] == 0 and c_on["n_col"] == 0 and c_on["n_shade_culled"] == 0
    # all head: the first two sigma > 0 samples of the rays on which 1e-5 <= sigma_1 (z_2 - z_1) <= 1 and sigma_2 >= 1e-3.  Then
    # alpha_1 <= 0.64, so w_1 <= 0.64 and the transmittance behind it is >= 0.36; the last sample's interval is 1 / 64, so
    # alpha_2 >= 1.5e-5 and w_2 >= 5e-6, three orders above the 2^-27 w_1 <= 5e-9 at which it would be a tail; the first
    # sample meets ws = 0 and is a tail only with w_1 == 0, which alpha_1 >= 1 - exp(-1e-5) > 0 excludes.
    # The other rays get no valid sample at all.
    i1, i2 = (pos & (order == 1)).int().argmax(dim=1, keepdim=True), (pos & (order == 2)).int().argmax(dim=1, keepdim=True)
    s1, s2 = sigma.gather(1, i1), sigma.gather(1, i2)
    dz = z.gather(1, i2) - z.gather(1, i1)
    ok = ((order[:, -1:] >= 2) & (s1 * dz <= 1.0) & (s1 * dz >= 1e-5) & (s2 >= 1e-3)).reshape(-1)
    assert int(ok.sum()) > 0
    two = (pos & (order <= 2) & ok[:, None]).to(torch.uint8)
    c_off, c_on = both(two)
    assert c_on["n_shade_culled"] == 0 and c_on["n_col"] == int(two.sum()) == 2 * int(ok.sum())


@gpu
def test_forward_maps_keeps_the_rgb(scene):
    """The maps forward ignores the cull (k_composite_maps sums signed normals: the check's bound does not hold there); its rgb
    is the plain forward's, which culls."""
    from arah_release_amd import config
    dev = torch.device("cuda:0")
    model, _ = config.build_synthetic_model("zju377_mono", 64, 16, 16, device=dev)
    assert model.idhr_network.ray_tracer.shade_cull is True
    inputs = scene.make_inputs(64, 64, frame_idx=2, device=dev)
    with torch.no_grad():
        a = model(dict(inputs), eval=True)
        torch.cuda.synchronize()
        culled = model.idhr_network.ray_tracer.workspace(dev).counters()["n_shade_culled"]
        b = model.forward_maps(dict(inputs), eval=True)
        torch.cuda.synchronize()
        after = model.idhr_network.ray_tracer.workspace(dev).counters()["n_shade_culled"]
    assert culled > 0 and after == culled
    assert torch.equal(a["rgb_values"], b["rgb_values"]) and torch.equal(a["network_body_mask"], b["network_body_mask"])
