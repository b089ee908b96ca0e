"""The audit of the tiered forward's sigma = +0 certificate (arah_tier_audit, csrc/tier.hpp).

The tiers skip samples and rays on the strength of Lipschitz assumptions about the subject (tests/test_tiered.py holds them on the
synthetic subjects).  The audit re-runs a hashed sample of what a tiered frame skipped through the exact kernels:
* on an intact certificate it finds nothing, examines exactly what the render skipped, and leaves the render's state untouched;
* on a certificate damaged on purpose (arah_occupancy_clear_box: a box of the bitmap cleared through the torso) it finds exactly
  the samples and rays where the untiered render disagrees with what the tiers assumed;
* through the model entry, "strict" returns the untiered frame and "sample" switches the following frames to the untiered path.
"""
import numpy as np
import pytest
import torch

from conftest import golden

gpu = pytest.mark.gpu

F7_512 = "f7_forward_zju377_mono_512x512_s64.npz"
HALF = (0.12, 0.12, 0.35)   # metres: the box cleared around the centre of the body's box, deep along the view axis (+z)


def test_audit_struct_matches_the_header():
    from arah_release_amd import hip
    import ctypes as C
    assert C.sizeof(hip.ArahTierAudit) == 176 and hip.AUDIT_BYTES == 176
    assert C.sizeof(C.c_uint64) * 8 == hip.ArahTierAudit.first_index.offset


def _pick(x, seed, k):
    """The audit's selection, restated (include/arah_hip.h): fmix32(x * 0x9E3779B1 + seed) has its k low bits zero."""
    m = np.uint64(0xFFFFFFFF)
    h = (np.asarray(x, dtype=np.uint64) * np.uint64(0x9E3779B1) + np.uint64(seed)) & m
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & m
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & m
    h ^= h >> np.uint64(16)
    return (h & np.uint64((1 << k) - 1)) == 0


def _damage(monkeypatch):
    """Every occupancy built from now on loses the voxels of a box through the torso."""
    from arah_release_amd import hip
    orig = hip.Workspace.occupancy

    def damaged(self, frame):
        occ = orig(self, frame)
        info = self.occupancy_info()
        c = [o + d * info["voxel"] / 2 for o, d in zip(info["origin"], info["dims"])]
        self.occupancy_clear_box([x - h for x, h in zip(c, HALF)], [x + h for x, h in zip(c, HALF)])
        return occ

    monkeypatch.setattr(hip.Workspace, "occupancy", damaged)


class _Capture:
    """Records the arguments and results of hip.render (the audit needs the render's own frame, sampling and rays)."""

    def __init__(self, monkeypatch):
        from arah_release_amd import hip
        self.orig = hip.render
        self.last = None
        monkeypatch.setattr(hip, "render", self)

    def __call__(self, frame, ws, sampling, cam, dirs, nf, pose34, tiered=False):
        out = self.orig(frame, ws, sampling, cam, dirs, nf, pose34, tiered=tiered)
        self.last = {"frame": frame, "ws": ws, "samp": sampling, "cam": cam, "dirs": dirs, "nf": nf, "out": out}
        return out


def _bits(t):
    t = t.contiguous()
    return t.view(torch.uint8) if t.dtype != torch.uint8 else t


def _render(model, inputs, n, S, tiered, cap):
    """One frame through the model entry; -> dict of its outputs, per-sample / per-ray state and counters (clones)."""
    idhr = model.idhr_network
    idhr.tiering, idhr.adaptive_shading = tiered, False
    ws = idhr.ray_tracer.workspace(inputs["ray_dirs"].device)
    if ws.buf is not None:
        ws.reset_counters()
    with torch.no_grad():
        out = model(dict(inputs), eval=True)
    r = _state(ws, n, S)
    r["out"] = {k: v.clone() for k, v in out.items() if torch.is_tensor(v)}
    r["hip"] = [t.clone() for t in cap.last["out"]]
    r["call"] = cap.last
    return r


def _state(ws, n, S):
    smp = ws.debug_samples(n, S)
    tier, pos = ws.tier_debug(n, S)
    torch.cuda.synchronize()
    r = {k: v.clone() for k, v in smp.items()}
    r["tier"], r["pos"], r["ctr"] = tier.clone(), pos.clone(), ws.counters()
    return r


def _audit(call, rate_log2, seed):
    from arah_release_amd import hip
    with torch.no_grad():
        block = hip.tier_audit(call["frame"], call["ws"], call["samp"], call["cam"], call["dirs"], call["nf"], rate_log2, seed)
        res = hip.audit_result(block)
        stag, rtag = call["ws"].tier_audit_debug(call["dirs"].shape[0], call["samp"].n_steps)
        torch.cuda.synchronize()
    return res, stag.clone(), rtag.clone()


def _model(name, g):
    from arah_release_amd import config
    return config.build_synthetic_model(name, int(g["n_steps"]), int(g["n_near"]), int(g["n_far"]), device=torch.device("cuda:0"))[0]


@gpu
@pytest.mark.parametrize("fname,name,wide", [("f7_forward_zju377_mono_64x64_s64.npz", "zju377_mono", False),
                                             ("f7_forward_h36m_48x48_s32.npz", "h36m", False),
                                             (F7_512, "zju377_mono", False),
                                             ("f17_wide_skinning.npz", "zju377_mono", True)])
def test_audit_of_an_intact_certificate(scene, monkeypatch, fname, name, wide):
    """Rate 1 on an intact certificate: no violation, the examined counts are what the render skipped, and the render's outputs,
    per-sample arrays, tiers and counters are bit-equal before and after the audit."""
    from arah_release_amd import config
    g = golden(fname)
    dev = torch.device("cuda:0")
    if wide:   # fixture F17's subject: skinning-MLP gains x scale
        model, _ = config.build_synthetic_model("zju377_mono", device=dev)
        config.widen_skinning_(model, float(g["scale"]))
        S, H, W, fi = 64, 160, 160, 0
    else:
        model = _model(name, g)
        S, H, W, fi = int(g["n_steps"]), int(g["H"]), int(g["W"]), int(g["frame_idx"])
    inputs = scene.make_inputs(H, W, frame_idx=fi, device=dev)
    n = inputs["ray_dirs"].shape[1]
    cap = _Capture(monkeypatch)
    before = _render(model, inputs, n, S, True, cap)
    res, stag, rtag = _audit(cap.last, 0, 0)
    after = _state(cap.last["ws"], n, S)
    for k in ("z", "pts", "T", "mask", "shaded", "state", "tier", "pos"):
        assert torch.equal(_bits(before[k]), _bits(after[k])), k
    assert before["ctr"] == after["ctr"]
    for a, b in zip(before["hip"], cap.last["out"]):
        assert torch.equal(_bits(a), _bits(b))
    assert res["violations"] == 0, res
    assert res["min_ratio"] > 17.33, res
    c, st, mask = before["ctr"], before["state"], before["mask"]
    assert res["b_examined"] == int((st == 2).sum()) == c["n_tier_samples_skipped"]
    assert res["c_examined"] == c["n_tier_rays_untraced"]
    # certified and converged = converged phase-1 / phase-2 samples minus those the density pass evaluated
    assert res["a_examined"] == int(((mask == 1) & ((st == 1) | (st == 3))).sum()) - c["n_density"]
    assert res["a_examined"] > 0 and res["b_examined"] > 0
    assert int(((stag & 3) == 1).sum()) == res["a_examined"] and int(((stag & 3) == 2).sum()) == res["b_examined"]
    assert torch.equal((stag & 3) == 2, st == 2)
    assert int((rtag != 0).sum()) == res["c_examined"] and res["b_converged"] == int(((stag & 7) == 6).sum())


@pytest.fixture(scope="module")
def damaged_frame(scene):
    """bench.py's frame (512 x 512 x 64) with a box of the bitmap cleared through the torso: the tiered render, its rate-1 audit and
    the untiered render of the same inputs (the truth)."""
    mp = pytest.MonkeyPatch()
    try:
        g = golden(F7_512)
        dev = torch.device("cuda:0")
        model = _model("zju377_mono", g)
        S = int(g["n_steps"])
        inputs = scene.make_inputs(int(g["H"]), int(g["W"]), frame_idx=int(g["frame_idx"]), device=dev)
        n = inputs["ray_dirs"].shape[1]
        cap = _Capture(mp)
        _damage(mp)
        dmg = _render(model, inputs, n, S, True, cap)
        audit = _audit(cap.last, 0, 0)
        sampled = _audit(cap.last, 4, 7)
        truth = _render(model, inputs, n, S, False, cap)
        return {"dmg": dmg, "truth": truth, "audit": audit, "sampled": sampled, "n": n, "S": S}
    finally:
        mp.undo()


@gpu
def test_audit_finds_exactly_what_a_damaged_certificate_breaks(damaged_frame):
    """Rate 1 on the damaged frame: the violations are the untiered render's own disagreements with the tiers' assumptions."""
    d, t = damaged_frame["dmg"], damaged_frame["truth"]
    res, stag, rtag = damaged_frame["audit"]
    n, S = damaged_frame["n"], damaged_frame["S"]
    conv_t = t["hip"][5].reshape(n)
    # class C: the rays kept out of loops A+B that converge untiered
    examined = rtag != 0
    assert int(examined.sum()) == d["ctr"]["n_tier_rays_untraced"]
    assert torch.equal(rtag == 3, examined & (conv_t != 0))
    assert res["c_violations"] == int((examined & (conv_t != 0)).sum()) > 0
    # classes A + B, on the rays whose depth samples are the same both ways (a ray of class C that converges untiered is
    # sampled around its surface there, uniformly here: its sample q is not the same point)
    same = (_bits(d["z"]).reshape(n, S * 4) == _bits(t["z"]).reshape(n, S * 4)).all(-1)
    assert bool(same[~(rtag == 3)].all())
    same_q = same.repeat_interleave(S)
    st = d["state"]
    sig_t = t["shaded"][:, 3].contiguous().view(torch.int32) != 0
    sig_d0 = d["shaded"][:, 3].contiguous().view(torch.int32) == 0
    skipped = (st == 2) | (st == 3) | ((st == 1) & sig_d0)   # never evaluated, phase 2, or certified in phase 1
    truth = skipped & (t["mask"] == 1) & sig_t
    found = (stag & 8) != 0
    assert torch.equal(found[same_q], truth[same_q])
    n_ab = res["a_violations"] + res["b_violations"]
    assert n_ab == int(found.sum()) and int(truth[same_q].sum()) > 0
    assert res["min_ratio"] < 17.33
    assert res["n_first"] == 8 and len(res["first"]) == 8
    # the damage changes pixels: the tiered render of the damaged bitmap is not the untiered one
    assert not torch.equal(d["out"]["rgb_values"], t["out"]["rgb_values"])


@gpu
def test_sampled_audit_examines_the_hashed_subset(damaged_frame):
    """Rate 1/16, seed 7: the examined samples and rays are exactly the hash's choice among the rate-1 ones, and so are the
    violations found."""
    res0, stag0, rtag0 = damaged_frame["audit"]
    res, stag, rtag = damaged_frame["sampled"]
    n, S = damaged_frame["n"], damaged_frame["S"]
    pq = torch.from_numpy(_pick(np.arange(n * S), 7, 4)).to(stag.device)
    pr = torch.from_numpy(_pick(np.arange(n), 7, 4)).to(stag.device)
    assert 0.04 < float(pq.float().mean()) < 0.08
    assert torch.equal(stag & 3, torch.where(pq, stag0 & 3, torch.zeros_like(stag0)))
    assert torch.equal(rtag, torch.where(pr, rtag0, torch.zeros_like(rtag0)))
    assert torch.equal(stag & 8, torch.where(pq, stag0 & 8, torch.zeros_like(stag0)))
    assert res["rate_log2"] == 4 and res["seed"] == 7
    for k in ("a_violations", "b_violations", "c_violations"):
        assert res[k] <= res0[k]
    assert 0 < res["violations"] <= res0["violations"]


@gpu
def test_model_entry_audit_modes(scene, monkeypatch):
    """Through MetaAvatarRender.forward on the damaged certificate: "off" returns the tiers' (wrong) frame, "strict" the untiered
    one with a warning, "sample" warns after the audited frame and renders the next one untiered."""
    g = golden("f7_forward_zju377_mono_128x128_s32.npz")
    dev = torch.device("cuda:0")
    model = _model("zju377_mono", g)
    idhr = model.idhr_network
    inputs = scene.make_inputs(int(g["H"]), int(g["W"]), frame_idx=int(g["frame_idx"]), device=dev)
    keys = ("rgb_values", "network_body_mask", "points_cam")

    def frame(tiering, mode="off"):
        idhr.tiering, idhr.adaptive_shading, idhr.tier_audit = tiering, False, mode
        with torch.no_grad():
            out = model(dict(inputs), eval=True)
        torch.cuda.synchronize()
        return {k: out[k].clone() for k in keys}

    _damage(monkeypatch)
    exact = frame(False)
    off = frame(True, "off")
    assert not torch.equal(off["rgb_values"], exact["rgb_values"])
    assert idhr.tier_violations == 0 and idhr.tier_audit_last is None

    idhr.tier_audit_rate_log2 = 0
    with pytest.warns(UserWarning, match="certificate"):
        strict = frame(True, "strict")
    for k in keys:
        assert torch.equal(strict[k], exact[k]), k
    assert idhr.tier_violations > 0 and idhr.tiering is False and idhr.tier_audit_last["violations"] > 0

    idhr.tier_violations, idhr.tier_audit_every = 0, 1
    first = frame(True, "sample")                    # audited; its result is read when the next frame starts
    assert not torch.equal(first["rgb_values"], exact["rgb_values"])
    idhr.tier_audit = "sample"
    with pytest.warns(UserWarning, match="certificate"):
        with torch.no_grad():
            out = model(dict(inputs), eval=True)     # tiering is still True here: the audit's verdict turns it off
    for k in keys:
        assert torch.equal(out[k], exact[k]), k
    assert idhr.tier_violations > 0 and idhr.tiering is False
