"""Posed-space queries of the articulated SDF: arah_query_posed, arah_sdf_grid_posed, MetaAvatarRender.query_posed / posed_mesh.

A posed point gets what the eval forward computes for a depth sample there (nearest vertex + inverse LBS, loop C, the SDF trunk);
the lattice meshes the posed level set.  CPU tests: the ABI surface, the box helpers and the band / value rule restated in torch.
GPU tests: the reference's own depth samples (F5), the oracle, exactness of the skips, band vs full lattice, consistency of the
posed meshes with each other and with the render, and the model entry.
"""
import os

import numpy as np
import pytest
import torch

from conftest import REPO, golden, get_model

gpu = pytest.mark.gpu
ENGINES = ["split", "fp32"]


class engine:
    """Frames built inside this context are prepared for the named GEMM engine (hip.default_precision reads the env)."""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.prev = os.environ.get("ARAH_PRECISION")
        os.environ["ARAH_PRECISION"] = self.name

    def __exit__(self, *exc):
        if self.prev is None:
            os.environ.pop("ARAH_PRECISION", None)
        else:
            os.environ["ARAH_PRECISION"] = self.prev


def rows_close_frac(a, b, atol, rtol=0.0):
    a = np.asarray(a, np.float64).reshape(len(a), -1)
    b = np.asarray(b, np.float64).reshape(len(b), -1)
    return float((np.abs(a - b) <= atol + rtol * np.abs(b)).all(axis=1).mean())


# ------------------------------------------------------------------------------------------ CPU
def test_posed_symbols_are_declared_and_exported():
    import re
    from arah_release_amd import hip
    header = open(os.path.join(REPO, "include", "arah_hip.h")).read()
    assert "#define ARAH_POSED_FILL 1.0f" in header
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("arah_query_posed_bytes", "arah_query_posed", "arah_sdf_grid_posed_bytes", "arah_sdf_grid_posed"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in hip.EXPORTS, name
    assert hip.POSED_FILL == 1.0


def test_query_buffer_is_bounded():
    import __graft_entry__ as g
    g.build()
    from arah_release_amd import hip
    lib = hip.load_library()
    small, big = lib.arah_query_posed_bytes(1000), lib.arah_query_posed_bytes(1 << 30)
    assert 0 < small < big
    assert lib.arah_sdf_grid_posed_bytes(256) == lib.arah_sdf_grid_posed_bytes(1024) == big   # a 256^3 lattice: passes of a fixed size
    assert big < 1 << 30
    assert lib.arah_sdf_grid_posed_bytes(1) == 0 and lib.arah_sdf_grid_posed_bytes(2000) == 0


def test_lattice_box_helpers():
    from arah_release_amd import hip
    box = hip.lattice_box([-0.5, -1.0, 0.2], [0.5, 0.8, 0.4], margin=0.1)
    side = 1.8 + 0.2
    np.testing.assert_allclose(box.numpy(), [0.0 - side / 2, -0.1 - side / 2, 0.3 - side / 2, side], rtol=0, atol=1e-6)
    # the corners of [-1,1]^3 are the lattice box's corners, the centre its centre; lattice point i sits at origin + i/(n-1) side
    corners = torch.tensor([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], [0.0, 0.0, 0.0]])
    w = hip.lattice_to_world(corners, box)
    np.testing.assert_allclose(w[0].numpy(), box[:3].numpy(), atol=1e-6)
    np.testing.assert_allclose(w[1].numpy(), (box[:3] + box[3]).numpy(), atol=1e-6)
    np.testing.assert_allclose(w[2].numpy(), (box[:3] + box[3] / 2).numpy(), atol=1e-6)
    n = 9
    i = torch.tensor([[3.0, 0.0, 8.0]])
    mc = -1.0 + i * (2.0 / (n - 1))                  # arah_marching_cubes' vertex of lattice index i
    np.testing.assert_allclose(hip.lattice_to_world(mc, box).numpy(), (box[:3] + i / (n - 1) * box[3]).numpy(), atol=1e-6)


def test_band_and_value_rule_keep_the_full_lattices_triangles():
    """On a hand-made lattice: a sphere, 'marked' = the points whose sdf is below a band, a few unconverged points far out.  The
    band (the dilation of the marked points) with the value rule gives the full lattice's signs everywhere, its values wherever it
    evaluated, and the CPU marching cubes the same triangles."""
    from arah_release_amd import hip, meshing
    n = 24
    ax = torch.linspace(-1, 1, n)
    X, Y, Z = torch.meshgrid(ax, ax, ax, indexing="ij")
    sdf = torch.sqrt(X ** 2 + Y ** 2 + Z ** 2) - 0.55
    state = torch.ones(n, n, n, dtype=torch.uint8)
    state[0, :3, :3] = 0                              # unconverged far from the body
    marked = sdf <= 0.1                               # the certificate: everything with sdf <= band lies in a marked voxel
    band = hip.posed_band(marked)
    assert band[marked].all() and band.sum() < n ** 3
    # the band evaluates exactly the points with a marked point among their 26 neighbours
    idx = torch.nonzero(band)[0]
    lo, hi = (idx - 1).clamp(min=0), (idx + 1).clamp(max=n - 1)
    assert marked[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1].any()
    full = hip.posed_value_rule(sdf, state)
    banded = hip.posed_value_rule(sdf, torch.where(band, state, torch.full_like(state, 2)))
    assert torch.equal(banded[band], full[band])
    assert torch.equal(banded < 0, full < 0)
    assert torch.equal(banded[~band], torch.full_like(banded[~band], hip.POSED_FILL))
    t_full = meshing.marching_cubes(full)
    t_band = meshing.marching_cubes(banded)
    assert t_full.shape[0] > 100 and torch.equal(t_full, t_band)


# ------------------------------------------------------------------------------------------ GPU helpers
def _frame(model, inputs, eng):
    from arah_release_amd import renderer
    dev = inputs["rots"].device
    with torch.no_grad(), engine(eng):
        dec = model.sdf_decoder({"coords": torch.zeros(1, 1, 3, device=dev), "rots": inputs["rots"][:1],
                                 "Jtrs": inputs["Jtrs"][:1], "latent": model.latent(inputs["geo_latent_code_idx"])})
        pose_cond = dict(inputs["pose_cond"])
        pose_cond["latent_code"] = model.latent(pose_cond["latent_code_idx"])
        return renderer.build_frame(dec["decoder"], model.skinning_model, model.color_decoder, model.deviation_decoder, pose_cond,
                                    inputs["smpl_verts"], inputs["skinning_weights"], inputs["bone_transforms"], inputs["trans"],
                                    inputs["coord_min"], inputs["coord_max"], inputs["center"])


def _query_points(model, inputs, n_each=1200, seed=0):
    """Surface points of a render (acc > 0.99), the same jittered by +-3 cm, uniform points in the body box and points up to 1 m
    outside it (beyond the nearest-vertex grid's box).  -> (P,3) device tensor, the four group sizes."""
    dev = inputs["rots"].device
    with torch.no_grad():
        out = model.forward_maps(inputs)
    acc, depth = out["acc_values"][0], out["depth_values"][0]
    d, o = inputs["ray_dirs"][0], inputs["cam_loc"][0].reshape(1, 3)
    surf = (o + depth[:, None] * d)[acc > 0.99]
    gen = torch.Generator(device="cpu").manual_seed(seed)
    surf = surf[torch.randperm(surf.shape[0], generator=gen)[:n_each].to(dev)]
    jit = surf + ((torch.rand(surf.shape, generator=gen) * 2 - 1) * 0.03).to(dev)
    v = inputs["smpl_verts"][0]
    lo, hi = v.min(0).values, v.max(0).values
    uni = lo + (hi - lo) * torch.rand(n_each, 3, generator=gen).to(dev)
    far = lo - 1.0 + (hi - lo + 2.0) * torch.rand(n_each, 3, generator=gen).to(dev)
    far = far[((far < lo) | (far > hi)).any(-1)]
    pts = torch.cat([surf, jit, uni, far]).contiguous()
    return pts, (surf.shape[0], jit.shape[0], uni.shape[0], far.shape[0])


def _lattice_mesh(hip, frame, ws, occ, n_side, band):
    sdf, box, counts = hip.sdf_grid_posed(frame, ws, n_side, occ=occ, band=band)
    tris, n = hip.marching_cubes(sdf, 0.0, 1 << 21)
    n = int(n.item())
    assert n <= 1 << 21
    return sdf, box, counts, tris, n


# ------------------------------------------------------------------------------------------ GPU
@gpu
@pytest.mark.parametrize("eng", ENGINES)
@pytest.mark.parametrize("tag", ["s64", "s32"])
def test_query_against_reference_depth_samples(scene, tag, eng):
    """The reference's converged depth samples (fixture f5: sampler_pts, sampler_transforms34 of inv_transform_points_opt) from
    their posed positions cam_loc + sampler_dists * ray_dir."""
    from arah_release_amd import config, hip
    g = golden("f5_tracer_%s.npz" % tag)
    dev = torch.device("cuda:0")
    S, nn, nfar = int(g["n_steps"]), int(g["n_near"]), int(g["n_far"])
    model, cfg = config.build_synthetic_model("zju377_mono", S, nn, nfar, device=dev)
    inputs = scene.make_inputs(int(g["H"]), int(g["W"]), frame_idx=int(g["frame_idx"]), max_rays=int(g["max_rays"]), device=dev)
    frame = _frame(model, inputs, eng)
    ws = model.idhr_network.ray_tracer.workspace(dev)
    m = torch.from_numpy(g["sampler_converge_mask"]).to(dev)
    z = torch.from_numpy(g["sampler_dists"]).to(dev).float()
    pts = (inputs["cam_loc"][0].reshape(1, 1, 3) + z[..., None] * inputs["ray_dirs"][0][:, None, :])[m]
    r = hip.query_posed(frame, ws, pts)
    conv = (r["state"] == 1).cpu().numpy()
    assert conv.mean() >= 0.995, conv.mean()
    mk = g["sampler_converge_mask"]
    ref_pts, ref_T = g["sampler_pts"][mk], g["sampler_transforms34"][mk].reshape(-1, 12)
    xh, Tm = r["points_hat"].cpu().numpy(), r["T"].cpu().numpy()
    assert rows_close_frac(xh[conv], ref_pts[conv], atol=3e-4) >= 0.999
    assert rows_close_frac(Tm[conv][:, :3, :].reshape(-1, 12), ref_T[conv], atol=3e-4, rtol=1e-3) >= 0.999


@pytest.fixture(scope="module")
def oracle_case(scene):
    """Query points of zju377_mono frame 0 and the oracle's answer at them (CPU torch)."""
    from arah_release_amd import config
    from oracle import arah_oracle as O
    dev = torch.device("cuda:0")
    model, cfg = get_model("zju377_mono", dev)
    model.eval()
    inputs = scene.make_inputs(128, 128, frame_idx=0, device=dev)
    pts, groups = _query_points(model, inputs)
    cpu_model, _ = config.build_synthetic_model("zju377_mono", device="cpu")
    fr = O.frame_from_model(cpu_model, scene.make_inputs(128, 128, frame_idx=0))
    p = pts.cpu().float()
    with torch.no_grad():
        xh, Tm, ok = O.canonicalize(fr, p)
        sdf, _, grad = O.sdf_forward_grad(fr, xh)
        nrm = torch.nn.functional.normalize(torch.einsum("pij,pj->pi", Tm[:, :3, :3], grad), dim=-1, eps=1e-12)
        w = O.query_weights(fr, O.unnormalize_points(fr, xh))
    return {"model": model, "inputs": inputs, "pts": pts, "groups": groups, "fr": fr,
            "ref": {"points_hat": xh.numpy(), "T": Tm.numpy(), "conv": ok.numpy(), "sdf": sdf.numpy(), "normal": nrm.numpy(),
                    "weights": w.numpy()}}


@gpu
@pytest.mark.parametrize("eng", ENGINES)
def test_query_against_oracle(oracle_case, eng):
    from arah_release_amd import hip
    c = oracle_case
    assert c["pts"].shape[0] >= 4096, c["groups"]
    dev = c["pts"].device
    frame = _frame(c["model"], c["inputs"], eng)
    ws = c["model"].idhr_network.ray_tracer.workspace(dev)
    r = {k: v.cpu().numpy() for k, v in hip.query_posed(frame, ws, c["pts"]).items()}
    ref = c["ref"]
    conv = r["state"] == 1
    agree = conv == ref["conv"]
    assert agree.mean() >= 0.995, agree.mean()
    both = conv & ref["conv"]
    assert both.sum() > 2000
    ok_x = rows_close_frac(r["points_hat"][both], ref["points_hat"][both], atol=2e-4)
    assert ok_x >= 0.999, ok_x
    # at the same canonical points: sdf, normal and weights of the kernels vs the oracle's
    close = (np.abs(r["points_hat"] - ref["points_hat"]) <= 2e-4).all(-1) & both
    scale = c["fr"].sdf_scale
    s_err = np.abs(r["sdf"][close] / scale - ref["sdf"][close])
    ok_s = s_err <= 1e-5 + 1e-4 * np.abs(ref["sdf"][close])
    cos = (r["normal"][close] * ref["normal"][close]).sum(-1)
    ok_w = (np.abs(r["weights"][close] - ref["weights"][close]) <= 1e-5 + 1e-4 * np.abs(ref["weights"][close])).all(-1)
    print("query vs oracle (%s): %d points, %d converged both; sdf worst %.3g (normalised), normal worst cos %.6f, weights worst %.3g"
          % (eng, len(conv), both.sum(), s_err.max(), cos.min(), np.abs(r["weights"][close] - ref["weights"][close]).max()))
    assert ok_s.mean() >= 0.999, ok_s.mean()
    assert (cos >= 0.9999).mean() >= 0.999, (cos >= 0.9999).mean()
    assert ok_w.mean() >= 0.999, ok_w.mean()


@gpu
@pytest.mark.parametrize("eng", ENGINES)
def test_skips_are_exact(oracle_case, eng):
    """Every evaluated point is bit-equal with and without the bitmap and under a permutation of the list; the points the bitmap
    certifies, evaluated, are unconverged or outside the 18 beta band of the certificate."""
    from arah_release_amd import hip
    c = oracle_case
    dev = c["pts"].device
    frame = _frame(c["model"], c["inputs"], eng)
    ws = c["model"].idhr_network.ray_tracer.workspace(dev)
    occ = ws.occupancy(frame)
    off = hip.query_posed(frame, ws, c["pts"])
    on = hip.query_posed(frame, ws, c["pts"], occ=occ)
    perm = torch.randperm(c["pts"].shape[0], generator=torch.Generator().manual_seed(1)).to(dev)
    pm = hip.query_posed(frame, ws, c["pts"][perm])
    inv = torch.argsort(perm)
    cert = on["state"] == 2
    ev = ~cert
    n_cert = int(cert.sum())
    assert 0 < n_cert < c["pts"].shape[0]
    assert torch.equal(on["state"][ev], off["state"][ev])
    assert bool((on["sdf"][cert] == hip.POSED_FILL).all())
    for k in hip.POSED_WANT:
        a, b = on[k][ev], off[k][ev]
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), k
        assert torch.equal(pm[k][inv].view(torch.int32), off[k].view(torch.int32)), k
    assert torch.equal(pm["state"][inv], off["state"])
    beta = float(torch.linalg.norm(c["model"].deviation_decoder.variance.detach()))
    st, sd = off["state"][cert], off["sdf"][cert]
    conv_cert = st == 1
    assert bool((sd[conv_cert] > 17.33 * beta).all()), float(sd[conv_cert].min()) / beta
    print("skips (%s): %d of %d points certified, %d of them converge when evaluated, min sdf / beta %.1f"
          % (eng, n_cert, len(cert), int(conv_cert.sum()), float(sd[conv_cert].min()) / beta if conv_cert.any() else float("inf")))


@gpu
@pytest.mark.parametrize("eng", ENGINES)
@pytest.mark.parametrize("name,frame_idx", [("zju377_mono", 1), ("zju377_mono", 5), ("h36m", 3)])
def test_band_lattice_gives_the_full_posed_lattices_mesh(scene, name, frame_idx, eng):
    from arah_release_amd import hip
    dev = torch.device("cuda:0")
    model, cfg = get_model(name, dev)
    inputs = scene.make_inputs(64, 64, frame_idx=frame_idx, device=dev)
    frame = _frame(model, inputs, eng)
    ws = model.idhr_network.ray_tracer.workspace(dev)
    occ = ws.occupancy(frame)
    full, box_f, cnt_f, t_full, n_full = _lattice_mesh(hip, frame, ws, occ, 256, False)
    band, box_b, cnt_b, t_band, n_band = _lattice_mesh(hip, frame, ws, occ, 256, True)
    assert torch.equal(box_f, box_b)
    cf, cb = cnt_f.tolist(), cnt_b.tolist()
    assert cf[0] == 256 ** 3 and cf[2] == 0 and cb[0] + cb[2] == 256 ** 3
    evaluated = band != hip.POSED_FILL
    assert bool((band[evaluated] == full[evaluated]).all())
    assert bool(((band < 0) == (full < 0)).all())
    assert n_full == n_band > 1000
    assert torch.equal(t_full, t_band)
    frac = cb[0] / 256 ** 3
    print("posed band lattice %s/%d (%s): box %s, %.1f %% evaluated, %d converged, %d triangles"
          % (name, frame_idx, eng, [round(v, 3) for v in box_b.tolist()], 100 * frac, cb[1], n_full))
    # Measured: ~62 % on zju377_mono frame 1.  The default cube's side is the body's height, so along the thin axes most of the cube
    # lies outside the bitmap's box, where nothing is certified (occ_lookup counts it as marked) and every point is evaluated.
    assert frac < 0.75


@gpu
@pytest.mark.parametrize("eng", ENGINES)
def test_posed_meshes_agree_with_the_field_and_the_render(oracle_case, eng):
    from arah_release_amd import hip, meshing
    c = oracle_case
    dev = c["pts"].device
    model, inputs = c["model"], c["inputs"]
    frame = _frame(model, inputs, eng)
    ws = model.idhr_network.ray_tracer.workspace(dev)
    occ = ws.occupancy(frame)
    n_side = 256
    _, box, _, tris, n = _lattice_mesh(hip, frame, ws, occ, n_side, True)
    step = float(box[3]) / (n_side - 1)
    tw = hip.lattice_to_world(tris[:n], box)
    verts = tw.reshape(-1, 3).contiguous()
    # 1. the field at the mesh's vertices: within the linear interpolation error of the lattice
    q = hip.query_posed(frame, ws, verts, want=("sdf",))
    conv = q["state"] == 1
    bad = conv & (q["sdf"].abs() > 2 * step)
    print("lattice mesh (%s): %d triangles, step %.4f m, %d vertices next to unconverged points" % (eng, n, step, int((~conv).sum())))
    assert int(bad.sum()) == 0, float(q["sdf"][conv].abs().max())
    # 2. the skinned canonical mesh lies on the lattice mesh (median distance below half a lattice step)
    faces = torch.arange(verts.shape[0], dtype=torch.int32, device=dev).reshape(-1, 3)
    _, posed, n_dev = meshing.skinned_mesh(frame, ws, inputs, 256)
    sk = posed[:int(n_dev.item())].reshape(-1, 3).contiguous()
    sel = torch.randperm(sk.shape[0], generator=torch.Generator().manual_seed(2))[:20000].to(dev)
    d2, *_ = hip.mesh_query(verts, faces, sk[sel])
    med = float(d2.sqrt().median())
    print("skinned mesh to lattice mesh (%s): median %.5f m" % (eng, med))
    assert med < 0.5 * step
    # 3. the render's surface points (acc > 0.99) lie on the lattice mesh
    with torch.no_grad():
        out = model.forward_maps(inputs)
    acc, depth = out["acc_values"][0], out["depth_values"][0]
    sp = (inputs["cam_loc"][0].reshape(1, 3) + depth[:, None] * inputs["ray_dirs"][0])[acc > 0.99].contiguous()
    d2, *_ = hip.mesh_query(verts, faces, sp)
    ok = (d2.sqrt() <= 2 * step).float().mean().item()
    print("render surface to lattice mesh (%s): %d rays, %.4f within 2 steps" % (eng, sp.shape[0], ok))
    assert ok >= 0.99


@gpu
def test_model_entry(scene, monkeypatch):
    from arah_release_amd import config, meshing
    dev = torch.device("cuda:0")
    model, cfg = config.build_synthetic_model("zju377_mono", device=dev)   # fresh: no forward has run on it
    model.eval()
    inputs = scene.make_inputs(32, 32, frame_idx=2, device=dev)
    v = inputs["smpl_verts"][0]
    lo, hi = v.min(0).values, v.max(0).values
    pts = (lo + (hi - lo) * torch.rand(2, 300, 3, generator=torch.Generator().manual_seed(3)).to(dev))
    r = model.query_posed(inputs, pts)
    assert r["sdf"].shape == (2, 300) and r["normal"].shape == (2, 300, 3) and r["weights"].shape == (2, 300, 24)
    assert r["points_hat"].shape == (2, 300, 3) and r["converged"].dtype == torch.bool and r["converged"].float().mean() > 0.9
    r1 = model.query_posed(inputs, pts[1])
    assert torch.equal(r1["sdf"], r["sdf"][1])
    rc = model.query_posed(inputs, pts, certify=True)
    ev = rc["state"] != 2
    assert torch.equal(rc["sdf"][ev], r["sdf"][ev])
    with torch.no_grad():
        before = model.forward_maps(inputs)
        mesh = model.posed_mesh(inputs, n_side=128)
        after = model.forward_maps(inputs)
    for k in before:
        if isinstance(before[k], torch.Tensor):
            assert torch.equal(before[k], after[k]), k
    assert mesh["n_tris"] == mesh["tris"].shape[0] > 500
    sk = model.posed_mesh(inputs, n_side=128, method="skinned")
    assert sk["n_tris"] == sk["tris"].shape[0] > 500
    # a too small first capacity is re-run at the exact size: nothing truncated
    cano_state = dict(meshing._mc_state(dev))
    monkeypatch.setattr(meshing, "MC_DEFAULT_CAP", 64)
    small = model.posed_mesh(inputs, n_side=128)
    assert small["n_tris"] == mesh["n_tris"] and torch.equal(small["tris"], mesh["tris"])
    small_sk = model.posed_mesh(inputs, n_side=128, method="skinned")
    assert small_sk["n_tris"] == sk["n_tris"] and torch.equal(small_sk["tris"], sk["tris"])
    # the canonical branch's adaptive capacity is not the posed meshes' business
    assert meshing._mc_state(dev)["cap"] == cano_state["cap"] and meshing._mc_state(dev)["overflowed"] == cano_state["overflowed"]
    box = mesh["box"]
    lo3, hi3 = box[:3].cpu(), (box[:3] + box[3]).cpu()
    given = model.posed_mesh(inputs, n_side=128, bounds=(lo3, hi3))
    assert given["n_tris"] > 500
    with pytest.raises(ValueError):
        model.posed_mesh(inputs, method="nope")
    model.train()
    try:
        with pytest.raises(ValueError):
            model.query_posed(inputs, pts)
        with pytest.raises(ValueError):
            model.posed_mesh(inputs)
    finally:
        model.eval()
