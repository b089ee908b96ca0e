"""The frame's non-MFMA helpers that exist twice -- a serial kernel that is the specification, and the cooperative kernel
the frame runs -- and the list append of k_tier_finalize (csrc/arah_hip.hip, csrc/tier.hpp).

* depth samples (RT:313-350, eval mode): wave per ray (variant 1) == thread per ray (variant 0) in the BITS of z and in the
  mask, and the z the tiered frame's classifier writes == variant 1 on the tracer's own rays;
* per-cell candidate lists of the nearest-vertex search: wave per cell == thread per cell byte for byte, the overflow record
  included, and the search on the new tables == a brute-force search;
* k_tier_finalize's density list, appended once per workgroup: the same samples, once each.
"""
import copy

import numpy as np
import pytest
import torch

from conftest import get_model, golden

gpu = pytest.mark.gpu


# ---- depth samples ---------------------------------------------------------------------------------------------------------
# the three built-in configs all sample 64 / 16 / 16 (config.py); bench.py's other shapes are n_steps / 4 near and far
DEPTH_CASES = [(64, 16, 16), (32, 8, 8), (128, 32, 32), (64, 0, 0), (64, 16, 0), (64, 0, 16), (128, 16, 16)]
SURFACE_RANGE = 0.05   # kSurfaceRange


def _depth_rays(seed, n=1000):
    """near_far, conv, start, end of n rays: the first ten hand-made (all surface rays), the rest random with conv at 50 %."""
    g = torch.Generator().manual_seed(seed)
    near = 0.5 + 1.5 * torch.rand(n, generator=g)
    far = near + 0.2 + 1.3 * torch.rand(n, generator=g)
    start = near + (far - near) * torch.rand(n, generator=g)
    conv = (torch.rand(n, generator=g) < 0.5).to(torch.uint8)
    start[0] = near[0]                                  # surface at the near bound: span < 0, clamped
    start[1] = near[1] + 0.03                           # start - range - near < 0: the far run collapses onto near (duplicates)
    start[2] = near[2] + SURFACE_RANGE                  # span == 0 up to rounding
    start[3] = near[3] + SURFACE_RANGE + 1e-5           # span at the clamp
    near[4] = far[4] = start[4] = 1.25                  # empty interval
    start[5] = far[5]                                   # surface at the far bound
    start[6] = near[6] + 2 * SURFACE_RANGE              # far run ends where the surface run begins: ties between the runs
    start[7] = near[7] + 3 * SURFACE_RANGE              # the runs interleave on a common lattice: more ties
    near[8], far[8], start[8] = 1.0, 2.0, 1.5           # round numbers
    near[9], far[9], start[9] = 0.0, 4.0, 0.1           # near = 0
    conv[:10] = 1
    end = far.clone()
    return torch.stack([near, far], 1).contiguous(), conv, start, end


@gpu
@pytest.mark.parametrize("S,n_near,n_far", DEPTH_CASES)
def test_wave_per_ray_depths_are_the_serial_kernels_bits(S, n_near, n_far):
    from arah_release_amd import hip
    dev = torch.device("cuda:0")
    samp = hip.Sampling(dev, S, n_near, n_far)
    nf, conv, start, end = (t.to(dev) for t in _depth_rays(100 + S + n_near * 3 + n_far * 7))
    for n in (1, 63, 64, 65, 1000):
        z0, m0 = hip.sample_depths_debug(0, samp, nf[:n], conv[:n], start[:n], end[:n])
        z1, m1 = hip.sample_depths_debug(1, samp, nf[:n], conv[:n], start[:n], end[:n])
        diff = int((z0.view(torch.int32) != z1.view(torch.int32)).sum())
        assert diff == 0, "S %d near %d far %d, %d rays: %d depths differ in their bits" % (S, n_near, n_far, n, diff)
        assert torch.equal(m0, m1)
    # the hand-made rays do what they were made for (n = 1000 is still in z0): rows ascend, and ties exist where they should
    z = z0.cpu()
    nc = n_near + 1 + n_far
    if n_near or n_far:
        assert bool((z[:10, 1:nc] >= z[:10, :nc - 1]).all())
        assert int(m0[:10, nc:].sum()) == 0 and int(m0[:10, :nc].min()) == 1
        if n_far > 1:   # the collapsed far run: n_far values within the clamped span (1e-5) of near, among the surface run's
            near1 = float(nf[1, 0])
            assert int(((z[1, :nc] >= near1) & (z[1, :nc] <= near1 + 1.1e-5)).sum()) >= n_far


def _render_captured(monkeypatch, model, inputs):
    """One tiered eval forward through the model entry; returns what the renderer handed to / got from arah_render."""
    from arah_release_amd import hip
    seen = {}
    real = hip.render

    def spy(frame, ws, sampling, cam_loc, dirs, near_far, pose34, **kw):
        out = real(frame, ws, sampling, cam_loc, dirs, near_far, pose34, **kw)
        seen.update(ws=ws, sampling=sampling, near_far=near_far, dists=out[4], conv=out[5], tiered=kw.get("tiered", False))
        return out
    monkeypatch.setattr(hip, "render", spy)
    idhr = model.idhr_network
    keep = (idhr.tiering, idhr.adaptive_shading)
    idhr.tiering, idhr.adaptive_shading = True, False
    try:
        with torch.no_grad():
            seen["out"] = model(dict(inputs), eval=True)
    finally:
        idhr.tiering, idhr.adaptive_shading = keep
        monkeypatch.setattr(hip, "render", real)
    assert seen["tiered"]
    return seen


@gpu
@pytest.mark.parametrize("name,H,W,fi,S,near,far", [("zju377_mono", 64, 64, 0, 64, 16, 16),      # f7_forward_zju377_mono_64x64_s64
                                                    ("h36m", 48, 48, 2, 32, 8, 8),              # f7_forward_h36m_48x48_s32
                                                    ("h36m", 48, 48, 2, 128, 32, 32)])          # bench's h36m config, --n-steps 128
def test_the_classifier_writes_the_depths_of_the_stand_alone_kernel(scene, monkeypatch, name, H, W, fi, S, near, far):
    """k_tier_classify<0> computes the depths itself (one lane per sample, two for n_steps = 128): the z it leaves in the
    workspace == arah_sample_depths_debug on the tracer's conv / start / end, variant 1 and variant 0, bit for bit."""
    from arah_release_amd import config, hip
    dev = torch.device("cuda:0")
    model, _ = config.build_synthetic_model(name, S, near, far, device=dev)
    inputs = scene.make_inputs(H, W, frame_idx=fi, device=dev)
    seen = _render_captured(monkeypatch, model, inputs)
    n = int(seen["near_far"].shape[0])
    smp = seen["ws"].debug_samples(n, S, which=("z", "state"))
    nf = seen["near_far"].reshape(n, 2).float().contiguous()
    z1, m1 = hip.sample_depths_debug(1, seen["sampling"], nf, seen["conv"], seen["dists"], nf[:, 1].contiguous())
    z0, m0 = hip.sample_depths_debug(0, seen["sampling"], nf, seen["conv"], seen["dists"], nf[:, 1].contiguous())
    zf = smp["z"].reshape(n, S)
    assert int(seen["conv"].sum()) > 0 and int((seen["conv"] == 0).sum()) > 0   # surface and other rays
    assert int((zf.view(torch.int32) != z1.view(torch.int32)).sum()) == 0
    assert int((z0.view(torch.int32) != z1.view(torch.int32)).sum()) == 0 and torch.equal(m0, m1)
    # the state the classifier starts from is the mask: TS_NONE exactly where the sampler masks a sample off
    assert torch.equal(smp["state"].reshape(n, S) != 0, m1 != 0)


# ---- cell candidate lists ----------------------------------------------------------------------------------------------------
def _bodies(scene, dev):
    inputs = scene.make_inputs(64, 64, frame_idx=0, device=dev)
    posed = inputs["smpl_verts"][0].float().contiguous()
    g = torch.Generator().manual_seed(3)
    d = torch.randn(posed.shape[0], 3, generator=g)
    ball = d / d.norm(dim=1, keepdim=True) * (0.05 * torch.rand(posed.shape[0], 1, generator=g) ** (1.0 / 3.0))
    ball = (ball + torch.tensor([0.1, -0.2, 0.3])).to(dev).contiguous()   # every vertex inside a 5 cm ball
    return inputs, {"posed": posed, "ball": ball}


def _brute_nearest(verts, pts, idx, chunk=2000):
    """Brute-force search in float64 (squared distances of fp32 inputs, exact to 2^-52), the first (lowest) index on ties.
    The kernels compare fp32 squared distances -- three roundings of <= 1/2 ulp on either side -- so fp32 RESOLVES a query
    when the runner-up's exact squared distance is more than 4 * 2^-24 (relative) above the minimum.  Returns per point: the
    reference index, whether the query is resolved, and whether `idx` is wrong: on a resolved query anything but the
    reference; on an unresolved one a vertex beyond that margin, or one at exactly the minimum with a higher index."""
    v = verts.astype(np.float64)
    eps = 4.0 * 2.0 ** -24
    ref = np.empty(pts.shape[0], np.int64)
    resolved = np.empty(pts.shape[0], bool)
    wrong = np.empty(pts.shape[0], bool)
    for i in range(0, pts.shape[0], chunk):
        p = pts[i:i + chunk].astype(np.float64)
        d2 = ((p[:, None, :] - v[None, :, :]) ** 2).sum(-1)
        r = np.argmin(d2, axis=1)
        rows = np.arange(r.shape[0])
        best = d2[rows, r]
        got = d2[rows, idx[i:i + chunk]]
        d2[rows, r] = np.inf
        runner_up = d2.min(axis=1)
        ref[i:i + chunk] = r
        resolved[i:i + chunk] = runner_up > best * (1.0 + eps)
        wrong[i:i + chunk] = (idx[i:i + chunk] != r) & ~((got > best) & (got <= best * (1.0 + eps)))
    return ref, resolved, wrong


@gpu
@pytest.mark.parametrize("which", ["posed", "ball"])
def test_wave_per_cell_lists_are_the_serial_kernels_bytes(scene, which):
    from arah_release_amd import hip, renderer
    dev = torch.device("cuda:0")
    inputs, bodies = _bodies(scene, dev)
    verts = bodies[which]
    tables = hip.BodyTables(verts)
    torch.cuda.synchronize()
    serial = hip.cell_clusters_debug(0, tables.buf)
    wave = hip.cell_clusters_debug(1, tables.buf)
    n_cells = serial.shape[0]
    built = tables.buf[hip.BODY_OFF_CELLS:hip.BODY_OFF_CELLS + n_cells * hip.BODY_CELL_BYTES].reshape(n_cells, hip.BODY_CELL_BYTES)
    bad = int((serial != wave).any(dim=1).sum())
    assert bad == 0, "%s: %d of %d cell records differ" % (which, bad, n_cells)
    assert torch.equal(built, serial)          # arah_prepare_body runs the wave-per-cell kernel
    # the grid header read at hip.BODY_OFF_GRID is the grid of THESE vertices: the box + 8 cm, dims whose product is n_cells
    hdr = tables.buf[hip.BODY_OFF_GRID:hip.BODY_OFF_GRID + 48].cpu()
    origin, dims = hdr.view(torch.float32)[:3], hdr.view(torch.int32)[5:8]
    assert int(dims.prod()) == n_cells == int(hdr.view(torch.int32)[8])
    assert torch.allclose(origin, verts.cpu().min(0).values - 0.08, atol=1e-6)
    spheres = tables.buf[hip.BODY_OFF_SPHERES:hip.BODY_OFF_GRID].view(torch.float32).reshape(256, 4).cpu()
    assert bool((spheres[:, 3] > 0).all()) and bool((spheres[:, 3] < 1.0).all())   # radii of 26-27 clustered vertices
    counts = serial[:, 0].cpu().numpy()
    assert n_cells > 1000 and counts.min() >= 1
    if which == "ball":
        assert int((counts == 255).sum()) > 0  # the overflow record: more than 63 clusters qualify
        assert bool((serial[serial[:, 0] == 255][:, 1:].to(torch.int32).sum(dim=1) > 0).all())
    assert counts[counts != 255].max(initial=0) <= 63

    # the search on these tables against brute force: 20 000 points, a fifth of them outside the grid
    model, _ = get_model("zju377_mono", dev)
    with torch.no_grad():
        dec = model.sdf_decoder({"coords": torch.zeros(1, 1, 3, device=dev), "rots": inputs["rots"][:1],
                                 "Jtrs": inputs["Jtrs"][:1], "latent": model.latent(inputs["geo_latent_code_idx"])})
        pose_cond = dict(inputs["pose_cond"])
        pose_cond["latent_code"] = model.latent(pose_cond["latent_code_idx"])
        frame = renderer.build_frame(dec["decoder"], model.skinning_model, model.color_decoder, model.deviation_decoder,
                                     pose_cond, verts[None], inputs["skinning_weights"], inputs["bone_transforms"],
                                     inputs["trans"], inputs["coord_min"], inputs["coord_max"], inputs["center"],
                                     body_tables=tables)
    g = torch.Generator().manual_seed(17)
    v = verts.cpu()
    lo, hi = v.min(0).values, v.max(0).values
    inside = lo - 0.07 + (hi - lo + 0.14) * torch.rand(16000, 3, generator=g)          # the grid is the box + 8 cm
    side = torch.where(torch.rand(4000, 3, generator=g) < 0.5, -1.0, 1.0)
    outside = 0.5 * (lo + hi) + side * (0.5 * (hi - lo) + 0.1 + 2.0 * torch.rand(4000, 3, generator=g))
    pts = torch.cat([inside, outside])[torch.randperm(20000, generator=g)].contiguous()
    idx, x_new, T_new = hip.nearest_inverse_lbs(frame, hip.Workspace(dev), pts.to(dev))
    # ... and the same search on tables whose lists the SERIAL kernel wrote: the same answers
    tables0 = copy.copy(tables)
    tables0.buf = tables.buf.clone()
    tables0.buf[hip.BODY_OFF_CELLS:hip.BODY_OFF_CELLS + n_cells * hip.BODY_CELL_BYTES] = serial.reshape(-1)
    with torch.no_grad():
        frame0 = renderer.build_frame(dec["decoder"], model.skinning_model, model.color_decoder, model.deviation_decoder,
                                      pose_cond, verts[None], inputs["skinning_weights"], inputs["bone_transforms"],
                                      inputs["trans"], inputs["coord_min"], inputs["coord_max"], inputs["center"],
                                      body_tables=tables0)
    idx0, x0, T0 = hip.nearest_inverse_lbs(frame0, hip.Workspace(dev), pts.to(dev))
    assert torch.equal(idx, idx0) and torch.equal(x_new, x0) and torch.equal(T_new, T0)
    got = idx.cpu().numpy().astype(np.int64)
    ref, resolved, wrong = _brute_nearest(v.numpy(), pts.numpy(), got)
    n_unresolved, n_wrong = int((~resolved).sum()), int(wrong.sum())
    n_diff = int((got != ref).sum())
    assert n_wrong == 0, "%s: %d of 20000 nearest vertices differ from the brute-force search" % (which, n_wrong)
    # equality wherever fp32 can tell the nearest from the runner-up; the queries where it cannot are few
    assert int(((got != ref) & resolved).sum()) == 0
    assert n_diff <= n_unresolved <= 20, (which, n_diff, n_unresolved)


# ---- k_tier_finalize's density list --------------------------------------------------------------------------------------------
def _tiered_and_exact(model, inputs, other, S):
    """Render `inputs` untiered, then `other` tiered (different rays or another frame: what it leaves in the workspace's per-sample
    arrays is NOT this frame's answer), then `inputs` tiered: a sample the density list dropped keeps a stale density, one
    appended twice shows in the counter."""
    idhr = model.idhr_network
    dev = inputs["ray_dirs"].device
    n = int(inputs["ray_dirs"].shape[1])
    keep = (idhr.tiering, idhr.adaptive_shading)
    idhr.adaptive_shading = False
    res = {}
    try:
        for label, on, inp in (("exact", False, inputs), ("other", True, other), ("tiered", True, inputs)):
            idhr.tiering = on
            with torch.no_grad():
                ws = idhr.ray_tracer.workspace(dev)
                if ws.buf is not None:
                    ws.reset_counters()
                out = model(dict(inp), eval=True)
                if label == "other":
                    continue
                ws = idhr.ray_tracer.workspace(dev)
                smp = ws.debug_samples(n, S, which=("mask", "shaded", "state"))
                torch.cuda.synchronize()
                res[label] = {"rgb": out["rgb_values"].clone(), "ctr": ws.counters(), "mask": smp["mask"].clone(),
                              "sigma": smp["shaded"][:, 3].clone(), "state": smp["state"].clone()}
    finally:
        idhr.tiering, idhr.adaptive_shading = keep
    return res


def _slice_rays(inputs, sel):
    n = int(inputs["ray_dirs"].shape[1])
    out = dict(inputs)
    for k, v in inputs.items():
        if torch.is_tensor(v) and v.dim() >= 2 and v.shape[1] == n and k != "smpl_verts":
            out[k] = v[:, sel].contiguous()
    return out


def _check_density_list(res, label):
    e, t = res["exact"], res["tiered"]
    ev = t["mask"] == 1                      # what the tiers evaluated and found converged
    # every such sample carries the exact path's density, bit for bit: the listed ones from the density pass, the certified
    # ones the +0 k_tier_finalize writes -- none kept the other render's value, so the list holds every expected id
    assert bool((e["mask"][ev] == 1).all()), label
    assert torch.equal(e["sigma"][ev].view(torch.int32), t["sigma"][ev].view(torch.int32)), label
    assert torch.equal(e["rgb"], t["rgb"]), label
    return t["ctr"]


@gpu
def test_finalize_appends_every_converged_sample_once(scene):
    """The tiered render of the 64 x 64 fixture frame (f7_forward_zju377_mono_64x64_s64: 2475 rays).  n_density counts the
    entries the density pass takes off k_tier_finalize's list; the figures below are those of the parent commit, whose
    k_tier_finalize appended with one atomic per wave:

        n_density = 12968, n_tier_samples_p1 = 22466 (phase 1's list: 87 * 256 + 194 entries), n_tier_samples_p2 = 6053

    The same count, and the same density on every evaluated sample as the untiered path, is the same SET, each id once."""
    from arah_release_amd import config
    dev = torch.device("cuda:0")
    g = golden("f7_forward_zju377_mono_64x64_s64.npz")
    S = int(g["n_steps"])
    model, _ = config.build_synthetic_model("zju377_mono", S, int(g["n_near"]), int(g["n_far"]), device=dev)
    inputs = scene.make_inputs(int(g["H"]), int(g["W"]), frame_idx=int(g["frame_idx"]), device=dev)
    other = scene.make_inputs(int(g["H"]), int(g["W"]), frame_idx=5, device=dev)
    c = _check_density_list(_tiered_and_exact(model, inputs, other, S), "64x64")
    print("n_density %d n_tier_samples_p1 %d n_tier_samples_p2 %d" % (c["n_density"], c["n_tier_samples_p1"], c["n_tier_samples_p2"]))
    assert c["n_tier_samples_p1"] % 256 != 0 and c["n_tier_samples_p1"] == N_P1_PARENT
    assert c["n_density"] == N_DENSITY_PARENT
    assert c["n_density_p2"] == 0


@gpu
def test_finalize_appends_a_list_of_one(scene):
    """One ray with ONE depth sample (n_steps = 1): a surface ray's only sample is the surface point itself, phase 1's list
    has length 1 and so has the density list."""
    from arah_release_amd import config
    dev = torch.device("cuda:0")
    model, _ = config.build_synthetic_model("zju377_mono", 1, 0, 0, device=dev)
    full = scene.make_inputs(64, 64, frame_idx=0, device=dev)
    n = int(full["ray_dirs"].shape[1])
    res = _tiered_and_exact(model, _slice_rays(full, slice(n // 2, n // 2 + 1)), _slice_rays(full, slice(n // 2 + 40, n // 2 + 41)), 1)
    c = _check_density_list(res, "one sample")
    assert c["n_tier_rays"] == 1 and c["n_tier_rays_surface"] == 1 and c["n_tier_samples_p1"] == 1
    assert c["n_density"] == 1 and int(res["tiered"]["mask"].sum()) == 1


N_DENSITY_PARENT = 12968
N_P1_PARENT = 22466
