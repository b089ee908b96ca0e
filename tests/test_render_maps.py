"""Normal, depth and opacity maps of the eval forward (arah_render_maps, MetaAvatarRender.forward_maps).

Definition (include/arah_hip.h): for every valid shaded sample i, n_i = normalize(T_i[:3,:3] . d sdf / d x_norm),
and with the compositing weights w_i of the rgb, per ray normal_world = sum w_i n_i, depth = sum w_i z_i, acc = sum w_i.

The expected values come from `shade_composite_maps` below: oracle.shade_composite (IDR:261-396) with the two sums added.
Its rgb and acc are the oracle's bit for bit (CPU test), so its weights are the reference's.
"""
import os
import re

import numpy as np
import pytest
import torch

from conftest import golden, get_model
from oracle import arah_oracle as O

gpu = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F7_SMALL = [("f7_forward_zju377_mono_64x64_s64.npz", "zju377_mono"), ("f7_forward_zju313_64x64_s64.npz", "zju313"),
            ("f7_forward_h36m_48x48_s32.npz", "h36m")]
F7_ALL = F7_SMALL + [("f7_forward_zju377_mono_128x128_s32.npz", "zju377_mono"), ("f7_forward_h36m_40x40_s128.npz", "h36m"),
                     ("f7_forward_h36m_128x128_s128.npz", "h36m"), ("f7_forward_zju377_mono_256x256_s32.npz", "zju377_mono"),
                     ("f7_forward_zju377_mono_512x512_s64.npz", "zju377_mono")]
MAP_KEYS = ("normal_values", "depth_values", "acc_values")


def shade_composite_maps(fr, pts, z, T, mask, view_dirs, n_steps, cano_view_dirs, render_last_pt=False):
    """oracle.shade_composite, statement for statement, plus the maps.  pts (n,S,3) normalised canonical, z (n,S), T (n,S,4,4),
    mask (n,S), view_dirs (n,3), every ray with >= 1 valid sample.  Returns rgb (n,3), acc (n,1), normal_world (n,3), depth (n,)."""
    n, S = z.shape
    lengths = mask.sum(-1)
    packed = torch.arange(S)[None, :] < lengths[:, None]
    vp = pts[mask]
    vT = T[mask]
    vd = view_dirs[:, None, :].expand(n, S, 3)[mask]
    if cano_view_dirs:
        Rinv = torch.linalg.inv(vT)[:, :3, :3]
        vin = torch.einsum("pij,pj->pi", Rinv, -vd)
    else:
        vin = -vd
    sdf, feat, grad = O.sdf_forward_grad(fr, vp)
    normal = grad
    if not cano_view_dirs:
        normal = torch.einsum("pij,pj->pi", vT[:, :3, :3], normal)
    sdf = sdf * fr.sdf_scale
    rgb = O.color_forward(fr, vp, normal, vin, feat)
    beta = min(max(abs(fr.beta), 1e-6), 1e6)
    inv_beta = 1.0 / beta
    dens = torch.relu(inv_beta * (0.5 + 0.5 * torch.sign(-sdf) * (1 - torch.exp(-sdf.abs() * inv_beta))))
    rgb_s = torch.zeros(n, S, 3)
    den_s = torch.zeros(n, S)
    z_s = torch.full((n, S), 1e10)
    rgb_s[packed], den_s[packed], z_s[packed] = rgb, dens, z[mask]
    delta = z_s[:, 1:] - z_s[:, :-1]
    if render_last_pt:
        delta = torch.cat([delta, torch.full((n, 1), 1e10)], dim=-1)
    else:
        delta = torch.cat([delta, torch.full((n, 1), 1.0 / n_steps)], dim=-1)
        delta[torch.arange(n), lengths - 1] = 1.0 / n_steps
    alpha = 1.0 - torch.exp(-den_s * delta)
    trans = torch.cumprod(torch.cat([torch.ones(n, 1), 1.0 - alpha + 1e-7], dim=-1), dim=-1)[:, :-1]
    w = alpha * trans
    acc = (w * packed).sum(-1, keepdim=True).clamp(0, 1)
    rgb_out = (rgb_s * (w * packed)[..., None]).sum(1)
    # the maps: the posed unit normal and the depth of every packed sample, with the same weights
    n_s = torch.zeros(n, S, 3)
    n_s[packed] = torch.nn.functional.normalize(torch.einsum("pij,pj->pi", vT[:, :3, :3], grad), dim=-1, eps=1e-12)
    wp = w * packed
    normal_world = (n_s * wp[..., None]).sum(1)
    depth = (torch.where(packed, z_s, torch.zeros_like(z_s)) * wp).sum(1)
    return rgb_out, acc, normal_world, depth


def restated_maps(cpu_model, cfg, inputs_cpu, smp, n, S):
    """shade_composite_maps on the per-sample arrays a GPU render left in its workspace (z, normalised canonical points, T,
    mask: loop D's inputs), so that only loop D is compared.  -> acc (n,), normal_world (n,3), depth (n,) (zeros off vol)."""
    fr = O.frame_from_model(cpu_model, inputs_cpu)
    z = smp["z"].cpu().reshape(n, S)
    pts = smp["pts"].cpu().reshape(n, S, 3)
    T = smp["T"].cpu().reshape(n, S, 4, 4)
    mask = smp["mask"].cpu().reshape(n, S).bool()
    d = inputs_cpu["ray_dirs"][0].float()
    vol = mask.any(-1)
    acc, nw, dep = torch.zeros(n), torch.zeros(n, 3), torch.zeros(n)
    ids = vol.nonzero()[:, 0]
    for c in range(0, ids.numel(), 4096):
        k = ids[c:c + 4096]
        _, a, nn_, dd = shade_composite_maps(fr, pts[k], z[k], T[k], mask[k], d[k], S, cfg["model"]["cano_view_dirs"])
        acc[k], nw[k], dep[k] = a[:, 0], nn_, dd
    return acc, nw, dep


def _render(model, inputs, tiered=False, full=False, maps=True):
    """One eval forward with the tiering / shading mode pinned; returns a dict of cloned tensors."""
    idhr = model.idhr_network
    keep = (idhr.tiering, idhr.adaptive_shading, idhr.ray_tracer.full_shading)
    idhr.tiering, idhr.adaptive_shading, idhr.ray_tracer.full_shading = tiered, False, full
    try:
        with torch.no_grad():
            out = model.forward_maps(dict(inputs)) if maps else model(dict(inputs), eval=True)
        torch.cuda.synchronize()
    finally:
        idhr.tiering, idhr.adaptive_shading, idhr.ray_tracer.full_shading = keep
    return {k: v.clone() for k, v in out.items() if torch.is_tensor(v)}


def maps_vs_restatement(scene, fname, name, precision=None):
    """The untiered GPU forward with maps against the restatement on its own samples.  -> dict of the measured deviations."""
    from arah_release_amd import config
    g = golden(fname)
    S, nn_, nf_ = int(g["n_steps"]), int(g["n_near"]), int(g["n_far"])
    dev = torch.device("cuda:0")
    model, cfg = config.build_synthetic_model(name, S, nn_, nf_, device=dev)
    model.idhr_network.precision = precision
    H, W, fi = int(g["H"]), int(g["W"]), int(g["frame_idx"])
    inputs = scene.make_inputs(H, W, frame_idx=fi, device=dev)
    out = _render(model, inputs)
    n = inputs["ray_dirs"].shape[1]
    smp = model.idhr_network.ray_tracer.workspace(dev).debug_samples(n, S, which=("z", "pts", "T", "mask"))
    cpu_model, _ = config.build_synthetic_model(name, S, nn_, nf_, device="cpu")
    acc_r, nw_r, dep_r = restated_maps(cpu_model, cfg, scene.make_inputs(H, W, frame_idx=fi), smp, n, S)
    R = inputs["pose"][0, :3, :3].float().cpu()
    nc_r = nw_r @ R.t()
    acc, nc, dep = out["acc_values"][0].cpu(), out["normal_values"][0].cpu(), out["depth_values"][0].cpu()
    hit = acc > 0.5
    cos = (nc[hit] * nc_r[hit]).sum(-1) / (nc[hit].norm(dim=-1) * nc_r[hit].norm(dim=-1)).clamp_min(1e-12)
    empty = acc == 0
    return {"acc": float((acc - acc_r).abs().max()), "depth": float((dep - dep_r).abs().max()),
            "depth_rel": float(((dep - dep_r).abs() / dep_r.abs().clamp_min(1e-6)).max()),
            "cos_min": float(cos.min()) if hit.any() else 1.0, "n_hit": int(hit.sum()),
            "empty_norm": float(nc[empty].norm(dim=-1).max()) if empty.any() else 0.0, "n_empty": int(empty.sum())}


# ------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("name,tag", [("zju377_mono", "s64"), ("h36m", "s64"), ("zju377_mono", "s32")])
def test_restatement_weights_are_the_oracles(scene, name, tag):
    """On fixture F6's inputs (the F5 sampler's points and transforms): rgb and acc of the restatement equal
    oracle.shade_composite bit for bit, and its maps are consistent (|normal_world| <= acc, depth within the samples' span)."""
    g5 = golden("f5_tracer_%s.npz" % tag)
    g = golden("f6_shade_%s_%s.npz" % (name, tag))
    model, cfg = get_model(name)
    inputs = scene.make_inputs(int(g5["H"]), int(g5["W"]), frame_idx=int(g5["frame_idx"]), max_rays=int(g5["max_rays"]))
    fr = O.frame_from_model(model, inputs)
    S = int(g["n_steps"])
    vol = g["vol_mask"]
    T34 = g5["sampler_transforms34"].reshape(-1, S, 3, 4)
    T44 = np.concatenate([T34, np.tile(np.array([0, 0, 0, 1], np.float32), T34.shape[:2] + (1, 1))], axis=2)
    args = (torch.as_tensor(g5["sampler_pts"][vol]), torch.as_tensor(g5["sampler_dists"][vol]), torch.as_tensor(T44[vol]),
            torch.as_tensor(g5["sampler_converge_mask"][vol]), inputs["ray_dirs"][0][torch.as_tensor(vol)], S,
            cfg["model"]["cano_view_dirs"])
    rgb_o, acc_o = O.shade_composite(fr, *args)
    rgb, acc, nw, depth = shade_composite_maps(fr, *args)
    assert torch.equal(rgb, rgb_o) and torch.equal(acc, acc_o)
    assert bool((nw.norm(dim=-1) <= acc[:, 0] + 1e-5).all())
    z, m = args[1], args[3]
    zmin = torch.where(m, z, torch.full_like(z, 1e10)).min(-1)[0]
    zmax = torch.where(m, z, torch.full_like(z, -1e10)).max(-1)[0]
    a = acc[:, 0]
    assert bool((depth >= zmin * a - 1e-4).all() and (depth <= zmax * a + 1e-4).all())


def test_render_maps_entry_is_declared_and_exported():
    import __graft_entry__ as g
    g.build()
    from arah_release_amd import hip
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "arah_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(arah_[a-z0-9_]+)\s*\(", header))
    for name in ("arah_render_maps", "arah_render_maps_bytes"):
        assert name in declared and name in hip.EXPORTS
        assert hasattr(hip.load_library(), name)
    lib = hip.load_library()
    assert lib.arah_render_maps_bytes(512 * 512, 64) == 512 * 512 * 64 * 16   # one f32x4 per sample
    assert lib.arah_render_maps_bytes(-1, 64) == 0


def test_render_maps_is_an_eval_option(scene):
    from arah_release_amd import config
    model, _ = config.build_synthetic_model("zju377_mono", device="cpu")
    inputs = scene.make_inputs(8, 8, frame_idx=0)
    with pytest.raises(ValueError, match="render_maps"):
        model.forward_maps(dict(inputs), eval=False)
    model.train()
    with pytest.raises(ValueError, match="render_maps"):
        model.forward_maps(dict(inputs))
    with pytest.raises(ValueError, match="render_maps"):
        model.idhr_network(dict(inputs), render_maps=True)


def test_normal_display_matches_the_reference_mapping():
    from arah_release_amd import renderer
    n = torch.tensor([[[0.0, 0.0, 1.0], [1.0, -1.0, 0.2]], [[-3.0, 2.0, 0.0], [0.5, 0.5, 0.5]]])
    mask = torch.tensor([[True, True], [True, False]])
    img = renderer.normal_display(n, mask)
    assert torch.equal(img[0, 0], torch.tensor([0.5, 0.5, 1.0]))
    assert torch.equal(img[0, 1], torch.tensor([1.0, 0.0, 0.6]))
    assert torch.equal(img[1, 0], torch.tensor([0.0, 1.0, 0.5]))     # clipped
    assert torch.equal(img[1, 1], torch.zeros(3))                      # the reference's background: -1 -> black
    img = renderer.normal_display(n, mask, background=(1.0, 1.0, 1.0))
    assert torch.equal(img[1, 1], torch.ones(3)) and torch.equal(img[0, 0], torch.tensor([0.5, 0.5, 1.0]))


# ------------------------------------------------------------------------------------------ GPU
# The HIP maps against the restatement on the same samples, measured on the MI355X (profiles/render_maps.txt), largest over the
# three fixtures: split engine |d acc| 1.6e-5, |d depth| 5.0e-5; fp32 engine 2.3e-5, 7.2e-5; min cosine on
# acc > 0.5 at least 0.9995 (printed as 1.00) on both.  Bounds: four times the larger of the two engines; the cosine bound is the definition's.
TOL = {"split": {"acc": 1e-4, "depth": 3e-4, "cos": 0.999}, "fp32": {"acc": 1e-4, "depth": 3e-4, "cos": 0.999}}


@gpu
@pytest.mark.parametrize("engine", ["split", "fp32"])
@pytest.mark.parametrize("fname,name", F7_SMALL)
def test_maps_against_the_restatement(scene, fname, name, engine):
    from arah_release_amd import hip
    prec = hip.PRECISION_FP32 if engine == "fp32" else None
    m = maps_vs_restatement(scene, fname, name, prec)
    tol = TOL[engine]
    assert m["n_hit"] > 100 and m["n_empty"] > 100, m
    assert m["acc"] <= tol["acc"], m
    assert m["depth"] <= tol["depth"], m
    assert m["cos_min"] >= tol["cos"], m
    assert m["empty_norm"] <= 1e-5, m


def _assert_maps_equal(a, b, label):
    for k in MAP_KEYS:
        assert torch.equal(a[k], b[k]), "%s: %s differs on %d rays" % (label, k, int((a[k] != b[k]).reshape(a[k].shape[1], -1).any(-1).sum()))


def _paths_agree(model, inputs, label):
    exact = _render(model, inputs, tiered=False)
    tiered = _render(model, inputs, tiered=True)
    full = _render(model, inputs, tiered=False, full=True)
    _assert_maps_equal(exact, tiered, label + " tiered")
    _assert_maps_equal(exact, full, label + " full shading")
    for k in ("rgb_values", "network_body_mask", "points_cam"):
        assert torch.equal(exact[k], tiered[k]) and torch.equal(exact[k], full[k]), (label, k)
    return exact


@gpu
@pytest.mark.parametrize("fname,name", F7_ALL)
def test_maps_tiered_and_full_shading_equal_the_exact_path(scene, fname, name):
    from arah_release_amd import config
    g = golden(fname)
    dev = torch.device("cuda:0")
    model, _ = config.build_synthetic_model(name, int(g["n_steps"]), int(g["n_near"]), int(g["n_far"]), device=dev)
    inputs = scene.make_inputs(int(g["H"]), int(g["W"]), frame_idx=int(g["frame_idx"]), device=dev)
    out = _paths_agree(model, inputs, fname)
    assert bool((out["acc_values"] > 0.5).any())


@gpu
def test_maps_tiered_and_full_shading_equal_the_exact_path_on_the_benchmark_frames(scene):
    from arah_release_amd import config
    dev = torch.device("cuda:0")
    model, _ = config.build_synthetic_model("zju377_mono", 64, 16, 16, device=dev)
    for fi in range(20):
        _paths_agree(model, scene.make_inputs(512, 512, frame_idx=fi, device=dev), "frame %d" % fi)


@gpu
@pytest.mark.parametrize("engine", ["split", "fp32", "b3_off"])
def test_maps_leave_the_other_outputs_alone(scene, engine, monkeypatch):
    """rgb_values, network_body_mask, points_cam with the flag are those without it, bit for bit; the output keys without the
    flag are exactly the usual three.  Engines: split (bf16 x 3 shading), fp32, split with the fp32-MFMA shading."""
    from arah_release_amd import config, hip
    if engine == "b3_off":
        monkeypatch.setenv("ARAH_SHADE_ENGINE", "fp32")
    dev = torch.device("cuda:0")
    model, _ = config.build_synthetic_model("zju377_mono", 64, 16, 16, device=dev)
    if engine == "fp32":
        model.idhr_network.precision = hip.PRECISION_FP32
    inputs = scene.make_inputs(128, 128, frame_idx=3, device=dev)
    for tiered in (False, True):
        a = _render(model, inputs, tiered=tiered, maps=False)
        b = _render(model, inputs, tiered=tiered, maps=True)
        assert {"rgb_values", "network_body_mask", "points_cam"} <= set(a) and not set(a) & set(MAP_KEYS)
        assert set(b) == set(a) | set(MAP_KEYS)
        for k in ("rgb_values", "network_body_mask", "points_cam"):
            assert torch.equal(a[k], b[k]), (engine, tiered, k)
        n = inputs["ray_dirs"].shape[1]
        assert b["normal_values"].shape == (1, n, 3) and b["depth_values"].shape == (1, n)
        assert bool((b["normal_values"].norm(dim=-1) <= b["acc_values"] + 1e-5).all())


@gpu
def test_maps_survive_the_strict_audit_rerender(scene, monkeypatch):
    """ARAH_TIER_AUDIT=strict with a certificate damaged on purpose (a box of the bitmap cleared through the torso, as in
    tests/test_tier_audit.py): the violating frame is rendered again untiered, maps included -- they equal the untiered render's."""
    from arah_release_amd import config, hip
    g = golden("f7_forward_zju377_mono_128x128_s32.npz")
    dev = torch.device("cuda:0")
    model, _ = config.build_synthetic_model("zju377_mono", int(g["n_steps"]), int(g["n_near"]), int(g["n_far"]), device=dev)
    inputs = scene.make_inputs(int(g["H"]), int(g["W"]), frame_idx=int(g["frame_idx"]), device=dev)
    orig = hip.Workspace.occupancy
    half = (0.12, 0.12, 0.35)

    def damaged(self, frame):
        occ = orig(self, frame)
        info = self.occupancy_info()
        c = [o + d * info["voxel"] / 2 for o, d in zip(info["origin"], info["dims"])]
        self.occupancy_clear_box([x - h for x, h in zip(c, half)], [x + h for x, h in zip(c, half)])
        return occ

    monkeypatch.setattr(hip.Workspace, "occupancy", damaged)
    exact = _render(model, inputs, tiered=False)
    off = _render(model, inputs, tiered=True)
    assert not torch.equal(off["normal_values"], exact["normal_values"])   # the damage shows in the maps
    idhr = model.idhr_network
    idhr.tier_audit, idhr.tier_audit_rate_log2 = "strict", 0
    try:
        with pytest.warns(UserWarning, match="certificate"):
            strict = _render(model, inputs, tiered=True)
    finally:
        idhr.tier_audit = "off"
    assert idhr.tier_violations > 0
    _assert_maps_equal(exact, strict, "strict audit re-render")
    for k in ("rgb_values", "network_body_mask", "points_cam"):
        assert torch.equal(exact[k], strict[k]), k


@gpu
def test_maps_of_several_views_are_in_each_views_camera_frame(scene):
    """B = 2 with the same rays and camera centre and a different pose for view 1: view 1's normal is pose[1,:3,:3] applied to
    view 0's world normal; depth and acc are view 0's."""
    from arah_release_amd import config
    dev = torch.device("cuda:0")
    model, _ = config.build_synthetic_model("zju377_mono", 64, 16, 16, device=dev)
    one = scene.make_inputs(96, 96, frame_idx=2, device=dev)
    two = dict(one)
    for k in ("ray_dirs", "body_bounds_intersections", "cam_loc"):
        two[k] = torch.cat([one[k], one[k]], 0)
    c, s = np.cos(0.7), np.sin(0.7)
    rot = torch.tensor([[c, 0.0, s, 0.0], [0.0, 1.0, 0.0, 0.0], [-s, 0.0, c, 0.0], [0.0, 0.0, 0.0, 1.0]], dtype=torch.float32, device=dev)
    two["pose"] = torch.stack([one["pose"][0], rot @ one["pose"][0]], 0)
    a = _render(model, one)
    b = _render(model, two)
    N = one["ray_dirs"].shape[1]
    assert b["normal_values"].shape == (2, N, 3)
    assert torch.equal(b["normal_values"][0], a["normal_values"][0])
    assert torch.equal(b["depth_values"][1], a["depth_values"][0]) and torch.equal(b["acc_values"][1], a["acc_values"][0])
    R0, R1 = one["pose"][0, :3, :3], two["pose"][1, :3, :3]
    world = a["normal_values"][0] @ R0          # camera -> world (R0 is a rotation)
    torch.testing.assert_close(b["normal_values"][1], world @ R1.t(), rtol=0, atol=1e-6)


@gpu
def test_depth_and_normals_agree_with_independent_geometry(scene):
    """Plausibility on the benchmark frame (512 x 512 x 64):
    * converged surface rays with acc > 0.99: depth / acc lies within the near-surface sample spacing (2 * 0.05 / n_near) of
      the traced surface distance |points_cam| (unit ray directions, camera at the origin of its frame);
    * the volume normal map against the rasterised `output_normal` of the canonical-mesh branch (gen_cano_mesh=True) on the
      interior pixels of both masks (eroded by 3 pixels): median cosine, measured 0.998 over 16 189 pixels
      (profiles/render_maps.txt); bound 0.98, ten times the measured distance from 1."""
    from arah_release_amd import config, imageops
    dev = torch.device("cuda:0")
    model, _ = config.build_synthetic_model("zju377_mono", 64, 16, 16, device=dev)
    H = W = 512
    inputs = scene.make_inputs(H, W, frame_idx=0, device=dev)
    with torch.no_grad():
        out = model.forward_maps(dict(inputs), gen_cano_mesh=True)
    acc, depth = out["acc_values"][0], out["depth_values"][0]
    dist = out["points_cam"][0].norm(dim=-1)
    surf = (dist > 0) & (acc > 0.99)
    assert int(surf.sum()) > 10000
    err = (depth[surf] / acc[surf] - dist[surf]).abs()
    spacing = 2 * 0.05 / 16
    assert float(err.median()) < 0.5 * spacing and float(torch.quantile(err, 0.99)) < 2 * spacing, (
        float(err.median()), float(torch.quantile(err, 0.99)))
    pix = inputs["image_mask"][0].reshape(-1)             # the rays are these pixels, in row-major order
    mesh_img = out["output_normal"][0]                     # (H, W, 3) display colours, background 0
    mesh_mask = mesh_img.sum(-1) > 0
    vol_mask = torch.zeros(H * W, dtype=torch.bool, device=dev)
    vol_mask[pix] = acc > 0.99
    n_img = torch.zeros(H * W, 3, device=dev)
    n_img[pix] = out["normal_values"][0]
    vol_mask, n_img = vol_mask.reshape(H, W), n_img.reshape(H, W, 3)
    inner = imageops.erode(mesh_mask, 7) & imageops.erode(vol_mask, 7)
    assert int(inner.sum()) > 10000
    n_mesh = mesh_img[inner] * 2.0 - 1.0
    n_vol = n_img[inner]
    cos = (n_mesh * n_vol).sum(-1) / (n_mesh.norm(dim=-1) * n_vol.norm(dim=-1)).clamp_min(1e-12)
    med = float(cos.median())
    print("median cosine volume vs mesh normals: %.5f over %d pixels" % (med, int(inner.sum())))
    assert med > 0.98, med
