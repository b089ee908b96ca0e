"""The five per-point kernels (arah_sdf_eval, arah_skin_lbs, arah_skin_jacobian, arah_color_eval, arah_shade_points) and
the compositing of loop D against the oracle in FLOAT64, over the whole domain the code claims.

Criterion.  For a point set and a quantity, with ``f64`` the float64 oracle (oracle.arah_oracle.frame_as), ``ref32`` the
fp32 oracle at the same fp32 inputs and ``got`` the kernel:

    E_ref = |ref32 - f64|     E_got = |got - f64|          (per element, float64 arithmetic)
    max(E_got) <= M_max * max(E_ref)      rms(E_got) <= M_rms * rms(E_ref)         (over the whole set)

The yardstick E_ref -- the fp32 reference's own rounding error -- is computed here, each run, on the CPU; it is not a
stored number and does not come from the kernels.

  * fp32-class arithmetic (everything on the fp32 engine; on the split engine arah_sdf_eval, arah_skin_lbs,
    arah_skin_jacobian, arah_color_eval and the sdf of arah_shade_points): M_max = 8, M_rms = 4.  The f16 hi+lo split drops
    the lo x lo product (2^-22 relative per product, four fp32 ulps), the hardware sine is within 1.24e-7 where libm is
    within ~6e-8 (profiles/r02_hw_sin_accuracy.txt), reductions run in another order: each about a factor 2 over the fp32
    reference, together below 8 on the worst element and below 4 on average.
  * bf16 x 3 arithmetic (split-engine frames: grad, rgb and density of arah_shade_points, rgb and acc of
    arah_shade_composite): M_max = 32, M_rms = 16.  16 significant bits per operand against 24 is 2^8 per product in the
    worst case; over a 256-wide reduction with random signs 2^8 / sqrt(256) = 16, doubled for the worst element.

Asserted on the sets core, box, claimed, surface and special (point_sets() below); `outer` lies beyond what the code claims
and is held to "never silently wrong" (test_outer_is_never_silently_wrong).  One line per (kernel, quantity, engine, subject,
set) is printed (``pointwise_f64 | ...``); profiles/pointwise_f64.txt is the table of one full run on the MI355X.

The kernels get the ORACLE's frame (hip_frame below): weights, FiLM constants, bones and box bit for bit, so that "the
same fp32 inputs" covers the networks too.  (Frames built from a model on the GPU carry the GPU rounding of the
hypernetwork and of the weight-norm fold; on the wide-range subject that alone put T at 7 / 9 times E_ref.)

What the first run found (MI355X; the bounds above were fixed before it):
  * fp32-class rows: ratio 0.3 .. 1.8 on every set, `claimed` and `outer` included (the wide-range subject to 3.6); bf16 x 3
    rows: gradient <= 7.6, colour <= 12.7, density <= 5.2.  No kernel defect in the arithmetic.
  * arah_skin_lbs, arah_skin_jacobian and arah_color_eval launch one fp32 kernel whatever the frame's engine: their rows
    are equal on both engines.  The split skinning MLP (its SCALED instance on the wide-range subject too) runs in loop C
    only, behind arah_broyden3_lbs; it is not reachable through these seams.
  * every seam refused n = 0 with ARAH_E_BADARG when called as hip.py calls it (an empty tensor's pointer is null and was
    checked before n): fixed in the entry points.
  * far from the body the density is exactly zero in float64 as in fp32 (`claimed`, `outer`): E_ref = 0 there because the
    quantity is, and the criterion asks the kernels for exactly zero (test_yardstick_is_not_vacuous says so).
  * two exceptions (EXCEPTIONS): the density on `special`, the wide-range subject's Jacobian on `outer`.
  * the tests bite: with the lo products removed from the split engine's GEMMs (hi x hi only; a scratch build) the split
    rows of arah_sdf_eval stand at 205 .. 814 (max) and 309 .. 720 (rms) times the reference's error.  (gemm_one_split
    alone is loop C's logit layer: no row here moves without it, test_broyden3_kernels_of_the_call does.)

The CPU tests at the top pin the float64 view against the REFERENCE's own fp32 outputs (fixtures F2/F3/F4/F6) and check
that the yardstick is not vacuous; the shape / isolation tests at the bottom are bit-exact.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import golden, get_model
from oracle import arah_oracle as O

gpu = pytest.mark.gpu

ENGINES = ["split", "fp32"]
M_FP32 = (8.0, 4.0)      # (M_max, M_rms), fp32-class arithmetic
M_BF16X3 = (32.0, 16.0)  # bf16 x 3 arithmetic
ASSERTED_SETS = ["core", "box", "claimed", "surface", "special"]
N_SET = 4096
CHUNK = 2048             # rows per oracle call (the float64 Jacobian keeps an autograd graph of 4 x 128 per row)


class engine:
    """Frames built inside this context are prepared for the named GEMM engine (as in test_hip_parity.py)."""

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


@pytest.fixture(scope="module", autouse=True)
def _at_most_16_threads():
    prev = torch.get_num_threads()
    torch.set_num_threads(min(16, prev))
    yield
    torch.set_num_threads(prev)


# ------------------------------------------------------------------------------------------ oracle frames (CPU)
_FRAMES = {}


def oracle_frames(scene, subject):
    """(fp32 Frame, float64 Frame, cano_view_dirs) of a subject; 'wide' is zju377_mono with the F17 skinning MLP."""
    if subject not in _FRAMES:
        from arah_release_amd import config
        if subject == "wide":
            model, cfg = config.build_synthetic_model("zju377_mono", device="cpu")   # a private copy: its skinning MLP is altered
            config.widen_skinning_(model, float(golden("f17_wide_skinning.npz")["scale"]))
        else:
            model, cfg = get_model(subject)
        fr = O.frame_from_model(model, scene.make_inputs(64, 64, frame_idx=0))
        _FRAMES[subject] = (fr, O.frame_as(fr, torch.float64), bool(cfg["model"]["cano_view_dirs"]))
    return _FRAMES[subject]


def chunked(fn, *xs):
    """fn over row chunks of the inputs; fn returns a tensor or a tuple of tensors."""
    n = xs[0].shape[0]
    outs = []
    for c in range(0, max(n, 1), CHUNK):
        r = fn(*[x[c:c + CHUNK] for x in xs])
        outs.append(r if isinstance(r, tuple) else (r,))
    cat = tuple(torch.cat(col, dim=0) for col in zip(*outs))
    return cat if len(cat) > 1 else cat[0]


# ------------------------------------------------------------------------------------------ point sets
_SETS = {}


def _shell(gen, outer, inner, n):
    """n uniform points of [-outer, outer]^3 that lie outside [-inner, inner]^3 (rejection from one seeded stream)."""
    keep = []
    have = 0
    while have < n:
        p = (torch.rand(4 * n, 3, generator=gen) * 2.0 - 1.0) * outer
        p = p[p.abs().max(dim=-1).values > inner]
        keep.append(p)
        have += p.shape[0]
    return torch.cat(keep)[:n].contiguous()


def _cube_marks(h):
    """8 corners, 6 face centres, 12 edge midpoints of the cube of half-width h: the 26 non-zero points of {-h, 0, h}^3."""
    g = torch.tensor([-h, 0.0, h])
    p = torch.cartesian_prod(g, g, g)
    return p[p.abs().sum(-1) > 0]


def point_sets(scene):
    """name -> (n, 3) fp32 normalised coordinates, drawn on the CPU from seeds; the same sets for every kernel."""
    if _SETS:
        return _SETS
    gen = torch.Generator().manual_seed(20260116)
    core = (torch.rand(N_SET, 3, generator=gen) * 2.0 - 1.0) * 0.8
    box = _shell(gen, 1.0, 0.8, N_SET)
    claimed = _shell(gen, 1.5, 1.0, N_SET)
    outer = _shell(gen, 3.0, 1.5, N_SET)
    # surface: core points pulled onto the zero level set by float64 Newton steps along the oracle's gradient
    _, fr64, _ = oracle_frames(scene, "zju377_mono")
    x = core.double()
    for _ in range(8):
        s, _, g = chunked(lambda q: O.sdf_forward_grad(fr64, q), x)
        step = (s / (g * g).sum(-1).clamp_min(1e-3))[:, None] * g
        x = x - step.clamp(-0.2, 0.2)
    x = x.float()
    s = chunked(lambda q: O.sdf_forward(fr64, q, count=False)[0], x.double())
    surface = x[(s.abs() <= 1e-3) & (x.abs().max(-1).values <= 1.0)].contiguous()
    assert surface.shape[0] >= 2048, surface.shape
    lat = torch.tensor([-1.5 + 3.0 * i / 8.0 for i in range(9)])    # the lattice k_skin_probe sizes the f16 scales on
    tiny = torch.tensor([[1e-40, -1e-42, 3e-39], [-1e-45, 1e-45, 0.0], [1.1754942e-38, -1.1754942e-38, 1e-41]])
    special = torch.cat([torch.zeros(1, 3), -torch.zeros(1, 3), tiny, _cube_marks(1.0), _cube_marks(1.5),
                         torch.cartesian_prod(lat, lat, lat), core[17:18].expand(64, 3)]).float().contiguous()
    _SETS.update(core=core, box=box, claimed=claimed, surface=surface, special=special, outer=outer)
    return _SETS


_INPUTS = {}


def point_inputs(scene, subject, pset):
    """Every per-point input of the five kernels for one subject and set, fp32, seeded: normalised points x, raw canonical
    x_hat (the skinning kernels' argument: unnormalised once, in fp32), random unit ray directions, random rotations with
    a small translation as blended transforms (as test_shade_points_on_the_shipped_engine draws them), and normal / feature
    from the float64 SDF oracle at the same points, cast to fp32 (arah_color_eval's inputs)."""
    if (subject, pset) in _INPUTS:
        return _INPUTS[(subject, pset)]
    fr, fr64, _ = oracle_frames(scene, subject)
    x = point_sets(scene)[pset]
    n = x.shape[0]
    gen = torch.Generator().manual_seed(11 + n)
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=gen), dim=-1)
    q, _ = torch.linalg.qr(torch.randn(n, 3, 3, generator=gen))
    Tm = torch.eye(4).repeat(n, 1, 1)
    Tm[:, :3, :3] = q
    Tm[:, :3, 3] = 0.1 * torch.randn(n, 3, generator=gen)
    _, feat, grad = chunked(lambda p: O.sdf_forward_grad(fr64, p), x.double())
    _INPUTS[(subject, pset)] = dict(x=x, x_hat=O.unnormalize_points(fr, x).contiguous(), d=d, T=Tm, normal=grad.float(),
                                    feat=feat.float())
    return _INPUTS[(subject, pset)]


# ------------------------------------------------------------------------------------------ the oracle's quantities
def density(fr, sdf_norm):
    """Laplace-CDF density of the metric SDF, as O.shade_composite forms it (IDR:343-351)."""
    sdf = sdf_norm * fr.sdf_scale
    inv_beta = 1.0 / min(max(abs(fr.beta), 1e-6), 1e6)
    return torch.relu(inv_beta * (0.5 + 0.5 * torch.sign(-sdf) * (1 - torch.exp(-sdf.abs() * inv_beta))))


def oracle_sdf(fr, inp, dt):
    sdf, feat, grad = chunked(lambda p: O.sdf_forward_grad(fr, p), inp["x"].to(dt))
    return dict(sdf=sdf, feat=feat, grad=grad)


def oracle_skin(fr, inp, dt):
    xh = inp["x_hat"].to(dt)
    w = chunked(lambda p: O.query_weights(fr, p, count=False), xh)
    xb, Tm = chunked(lambda p: O.lbs_forward(fr, p, count=False), xh)
    return dict(weights=w, x_bar=xb, T=Tm, jac=chunked(lambda p: O.lbs_jacobian(fr, p), xh))


def oracle_color(fr, inp, dt):
    rgb = chunked(lambda p, nr, v, ft: O.color_forward(fr, p, nr, v, ft), inp["x"].to(dt), inp["normal"].to(dt),
                  inp["d"].to(dt), inp["feat"].to(dt))
    return dict(rgb=rgb)


def oracle_shade(fr, inp, dt, cano):
    x, Tm, d = inp["x"].to(dt), inp["T"].to(dt), inp["d"].to(dt)
    sdf, feat, grad = chunked(lambda p: O.sdf_forward_grad(fr, p), x)
    normal = grad if cano else torch.einsum("pij,pj->pi", Tm[:, :3, :3], grad)
    vin = torch.einsum("pij,pj->pi", torch.linalg.inv(Tm)[:, :3, :3], -d) if cano else -d
    rgb = chunked(lambda p, nr, v, ft: O.color_forward(fr, p, nr, v, ft), x, normal, vin, feat)
    return dict(rgb=rgb, density=density(fr, sdf), sdf=sdf, grad=grad)


_ORACLE = {}


def oracle_pair(scene, kernel, subject, pset):
    """(ref32, f64): dicts quantity -> tensor of the fp32 oracle and of its float64 view at the same fp32 inputs."""
    key = (kernel, subject, pset)
    if key not in _ORACLE:
        fr, fr64, cano = oracle_frames(scene, subject)
        inp = point_inputs(scene, subject, pset)
        fn = dict(sdf=oracle_sdf, skin=oracle_skin, color=oracle_color,
                  shade=lambda f, i, dt: oracle_shade(f, i, dt, cano))[kernel]
        _ORACLE[key] = (fn(fr, inp, torch.float32), fn(fr64, inp, torch.float64))
    return _ORACLE[key]


def errors(a, f64):
    e = (a.detach().double().cpu() - f64).abs().reshape(-1)
    return float(e.max()), float((e * e).mean().sqrt())


# ------------------------------------------------------------------------------------------ CPU: the float64 view
def _pin(name, gold, o32, o64):
    """max |golden - f64| <= 2 max |oracle32 - f64|: the golden is the reference's own fp32 run of the same arithmetic,
    the factor 2 covers the different summation order of its BLAS calls."""
    e_gold, _ = errors(torch.from_numpy(np.asarray(gold)), o64)
    e_o32, _ = errors(o32, o64)
    print("f64 view | %-22s max|golden - f64| %.3e  max|oracle32 - f64| %.3e  ratio %.2f" % (name, e_gold, e_o32, e_gold / e_o32))
    assert e_o32 > 0 and e_gold <= 2.0 * e_o32, (name, e_gold, e_o32)


def test_float64_view_keeps_the_fp32_frame(scene):
    fr, fr64, _ = oracle_frames(scene, "zju377_mono")
    back = O.frame_as(fr64, torch.float32)
    for a, b, c in zip(fr.sdf_layers + fr.skin_layers + fr.color_layers, fr64.sdf_layers + fr64.skin_layers + fr64.color_layers,
                       back.sdf_layers + back.skin_layers + back.color_layers):
        for u, v, w in zip(a, b, c):
            assert (u is None and v is None) or (v.dtype == torch.float64 and u.dtype == torch.float32 and torch.equal(u, w))
    for k in ("pose_vec", "verts", "vert_weights", "bones", "trans", "center"):
        assert getattr(fr64, k).dtype == torch.float64 and torch.equal(getattr(back, k), getattr(fr, k)), k
    assert fr64.beta == fr.beta and fr64.coord_min == fr.coord_min and fr64.color_mode == fr.color_mode
    assert fr64.counters is not fr.counters and set(fr64.counters.values()) == {0}


def test_float64_view_is_pinned_to_the_reference_f2_f3(scene):
    fr, fr64, _ = oracle_frames(scene, "zju377_mono")
    g = golden("f3_sdf.npz")
    x = torch.from_numpy(g["x_norm"])
    a, b = O.sdf_forward_grad(fr, x), O.sdf_forward_grad(fr64, x.double())
    for k, name in enumerate(("sdf", "feat", "grad")):
        _pin("f3 " + name, g[name], a[k], b[k])
    g = golden("f2_pointwise.npz")
    xh = torch.from_numpy(g["x_hat"])
    _pin("f2 weights", g["weights"], O.query_weights(fr, xh), O.query_weights(fr64, xh.double()))
    (xb, Tm), (xb64, Tm64) = O.lbs_forward(fr, xh), O.lbs_forward(fr64, xh.double())
    _pin("f2 x_bar", g["x_bar"], xb, xb64)
    _pin("f2 T", g["T"], Tm, Tm64)
    _pin("f2 jac", g["jac"], O.lbs_jacobian(fr, xh), O.lbs_jacobian(fr64, xh.double()))


@pytest.mark.parametrize("name", ["zju377_mono", "zju313"])
def test_float64_view_is_pinned_to_the_reference_f4(scene, name):
    fr, fr64, _ = oracle_frames(scene, name)
    g = golden("f4_color_%s.npz" % name)
    args = [torch.from_numpy(g[k]) for k in ("points", "normals", "view", "feat")]
    _pin("f4 rgb " + name, g["rgb"], O.color_forward(fr, *args), O.color_forward(fr64, *[a.double() for a in args]))


def _f6_case(scene, name, tag):
    """The F5/F6 fixtures' points, depths, transforms, masks and view directions (fp32) for O.shade_composite."""
    g5 = golden("f5_tracer_%s.npz" % tag)
    g = golden("f6_shade_%s_%s.npz" % (name, tag))
    inputs = scene.make_inputs(int(g5["H"]), int(g5["W"]), frame_idx=int(g5["frame_idx"]), max_rays=int(g5["max_rays"]))
    S = int(g["n_steps"])
    T34 = g5["sampler_transforms34"].reshape(-1, S, 3, 4)
    T44 = np.concatenate([T34, np.tile(np.array([0, 0, 0, 1], np.float32), T34.shape[:2] + (1, 1))], axis=2)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    return dict(g5=g5, g=g, inputs=inputs, S=S, vol=g["vol_mask"], pts=t(g5["sampler_pts"]), z=t(g5["sampler_dists"]), T=t(T44),
                mask=t(g5["sampler_converge_mask"]), d=inputs["ray_dirs"][0])


def _f6_oracle(scene, name, tag):
    """(case, ref32, f64) of O.shade_composite on the rays that own a valid sample."""
    c = _f6_case(scene, name, tag)
    model, cfg = get_model(name)
    fr = O.frame_from_model(model, c["inputs"])
    fr64 = O.frame_as(fr, torch.float64)
    vol = torch.from_numpy(c["vol"])
    out = []
    for f, dt in ((fr, torch.float32), (fr64, torch.float64)):
        rgb, acc = O.shade_composite(f, c["pts"][vol].to(dt), c["z"][vol].to(dt), c["T"][vol].to(dt), c["mask"][vol], c["d"][vol].to(dt),
                                     c["S"], cfg["model"]["cano_view_dirs"])
        out.append(dict(rgb=rgb, acc=acc[:, 0]))
    c["cano"], c["frame"] = cfg["model"]["cano_view_dirs"], fr
    return c, out[0], out[1]


F6_CASES = [("zju377_mono", "s64"), ("h36m", "s64"), ("zju377_mono", "s32")]


@pytest.mark.parametrize("name,tag", F6_CASES)
def test_float64_view_is_pinned_to_the_reference_f6(scene, name, tag):
    c, o32, o64 = _f6_oracle(scene, name, tag)
    _pin("f6 rgb %s %s" % (name, tag), c["g"]["rgb"], o32["rgb"], o64["rgb"])
    _pin("f6 acc %s %s" % (name, tag), c["g"]["acc"][:, 0], o32["acc"], o64["acc"])


SUBJECTS = {"sdf": ["zju377_mono"], "skin": ["zju377_mono", "wide"], "color": ["zju377_mono", "zju313"],
            "shade": ["zju377_mono", "zju313"]}


@pytest.mark.parametrize("pset", ASSERTED_SETS + ["outer"])
def test_yardstick_is_not_vacuous(scene, pset):
    """max |oracle32 - f64| > 0 for every quantity on every point set: the bound the kernels are held to is not zero, and
    the float64 view is not the fp32 oracle in disguise."""
    for kernel in ("sdf", "skin", "color", "shade"):
        o32, o64 = oracle_pair(scene, kernel, "zju377_mono", pset)
        for q in o32:
            assert o64[q].dtype == torch.float64 and o32[q].dtype == torch.float32 and bool(torch.isfinite(o64[q]).all())
            e_max, e_rms = errors(o32[q], o64[q])
            print("yardstick | %-6s %-8s %-8s max %.3e rms %.3e (|f64| max %.3g)" % (kernel, q, pset, e_max, e_rms, float(o64[q].abs().max())))
            if q == "density" and float(o64[q].abs().max()) == 0:
                # Far from the body (every point of `claimed` and `outer` is more than 745 beta outside the surface) the
                # density exp(-sdf / beta) / (2 beta) underflows to exactly zero in float64 as in fp32: E_ref is zero
                # because the quantity is, and the criterion then asks the kernel for exactly zero -- no less.
                assert pset in ("claimed", "outer") and e_max == 0
                continue
            assert e_max > 0 and e_rms > 0, (kernel, q, pset)


# ------------------------------------------------------------------------------------------ GPU: frames and kernels
_GPU = {}


def gpu_ctx(scene, subject, eng):
    """HIP frame of a subject on an engine (cached), with a workspace of its own."""
    key = (subject, eng)
    if key not in _GPU:
        from arah_release_amd import hip
        dev = torch.device("cuda:0")
        fr, _, cano = oracle_frames(scene, subject)
        _GPU[key] = dict(hip=hip, dev=dev, frame=hip_frame(fr, dev, eng), ws=hip.Workspace(dev), cano=cano)
    return _GPU[key]


def hip_frame(fr, dev, eng):
    """The HIP frame of the ORACLE's frame: the kernels get the fp32 weights, FiLM constants, bones and box the oracles
    compute with, bit for bit -- "the same fp32 inputs" of the criterion covers the networks, not only the points.  (A
    frame built from a model on the GPU carries the hypernetwork's and the weight-norm fold's GPU rounding: emitted weights a
    few ulp away from the CPU oracle's, which the wide-range subject's logits of several thousand turn into an input
    error as large as the arithmetic's own.)"""
    from arah_release_amd import hip
    t = lambda v: v.to(dev).contiguous()
    with engine(eng):
        return hip.Frame([(t(W), t(b)) for W, b, _, _ in fr.sdf_layers], t(torch.cat([f for _, _, f, _ in fr.sdf_layers[:-1]])),
                         t(torch.cat([p for _, _, _, p in fr.sdf_layers[:-1]])), [(t(W), t(b)) for W, b in fr.skin_layers],
                         [(t(W), t(b)) for W, b in fr.color_layers], hip.COLOR_IDR if fr.color_mode == "idr" else hip.COLOR_NO_VIEW_DIR,
                         None if fr.pose_vec is None else t(fr.pose_vec), fr.beta, t(fr.verts), t(fr.vert_weights), t(fr.bones),
                         t(fr.trans), t(fr.center), fr.coord_min, fr.coord_max)


def run_sdf(c, inp, ws=None):
    sdf, feat, grad = c["hip"].sdf_eval(c["frame"], ws or c["ws"], inp["x"], want_feat=True, want_grad=True)
    sdf_f, feat_f, _ = c["hip"].sdf_eval(c["frame"], ws or c["ws"], inp["x"], want_feat=True)    # the forward-only instance
    return dict(sdf=sdf, feat=feat, grad=grad, sdf_fwd=sdf_f, feat_fwd=feat_f)


def run_skin(c, inp, ws=None):
    w, xb, Tm = c["hip"].skin_lbs(c["frame"], ws or c["ws"], inp["x_hat"])
    return dict(weights=w, x_bar=xb, T=Tm)


def run_jac(c, inp, ws=None):
    return dict(jac=c["hip"].skin_jacobian(c["frame"], ws or c["ws"], inp["x_hat"]))


def run_color(c, inp, ws=None):
    return dict(rgb=c["hip"].color_eval(c["frame"], ws or c["ws"], inp["x"], inp["normal"], inp["d"], inp["feat"]))


def run_shade(c, inp, ws=None):
    rgb, dens, sdf, grad = c["hip"].shade_points(c["frame"], ws or c["ws"], inp["x"], inp["T"], inp["d"], c["cano"])
    return dict(rgb=rgb.contiguous(), density=dens.contiguous(), sdf=sdf.contiguous(), grad=grad.contiguous())


RUNNERS = dict(sdf=run_sdf, skin=run_skin, jac=run_jac, color=run_color, shade=run_shade)
ORACLE_OF = dict(sdf="sdf", skin="skin", jac="skin", color="color", shade="shade")
ALIAS = dict(sdf_fwd="sdf", feat_fwd="feat")     # the forward-only instance is held to the same oracle quantities


def on_gpu(inp, dev, rows=None):
    return {k: (v if rows is None else v[rows]).contiguous().to(dev) for k, v in inp.items()}


def bound_of(kernel, quantity, eng):
    b3 = eng == "split" and os.environ.get("ARAH_SHADE_ENGINE") != "fp32"
    if b3 and (kernel, quantity) in (("shade", "grad"), ("shade", "rgb"), ("shade", "density"), ("composite", "rgb"), ("composite", "acc")):
        return M_BF16X3
    return M_FP32


# Exceptions: (kernel, quantity, set) -> (subjects, measured max ratio, measured rms ratio), capped at twice the
# measurement.  At most 3, none on `core`.
EXCEPTIONS = {
    # Only 2 of the set's 850 points lie within a few beta (1 mm) of the surface; everywhere else the density is saturated at
    # 0 or 1 / beta and both errors vanish, so ONE point decides the row (lattice point (0.375, -0.375, 0), density 22 of
    # 1000, slope 2.2e4 per metre) -- the per-point comparison the criterion excludes ("E_ref can be zero by luck").  There
    # the reference's SDF is 3.5e-9 off on the machine of the table (3.4e-8 on another CPU: its own luck moves by 10) and
    # the fp32 engine's 2.1e-8, a fiftieth of its set-wide worst (1.1e-6, ratio 0.9 on the sdf row).  The bf16 x 3 engine
    # draws 5.2 / 3.7 at the same point.  Measured on the fp32 engine, both colour subjects (same SDF).
    ("shade", "density", "special"): (("zju377_mono", "zju313"), 6.00, 4.27),
    # fp32 forward-mode differentiation itself: k_skin_jac carries three tangents through the MLP, the reference sweeps
    # backwards.  On the wide-range subject (logits to 6600, fp32 error 1.6e-3 in them, x 20 in the gates) the weights are
    # saturated, E_ref > 0 in 18 of 36864 elements, and one point at a steep gate carries the row: entry 0.3198, reference
    # 0.3195, kernel 0.3218.  torch's own forward mode (torch.autograd.functional.jvp on the fp32 oracle, CPU) gives
    # 0.3217 there and max 1.91e-3 / rms 1.47e-5 over the set -- ratio 3.10 / 4.01 with no kernel involved; the kernel:
    # 3.25 / 4.33 (max inside M_max).  One kernel serves both engines.
    ("jac", "jac", "outer"): (("wide",), 3.25, 4.33),
}
assert len(EXCEPTIONS) <= 3 and not any(k[2] == "core" for k in EXCEPTIONS)


def judge(kernel, eng, subject, pset, got, o32, o64):
    """Print one table line per quantity; return the list of quantities over their bound."""
    bad = []
    for q, val in got.items():
        oq = ALIAS.get(q, q)
        r_max, r_rms = errors(o32[oq], o64[oq])
        g_max, g_rms = errors(val, o64[oq])
        m_max, m_rms = bound_of(kernel, oq, eng)
        exc = EXCEPTIONS.get((kernel, oq, pset))
        if exc and subject in exc[0]:
            m_max, m_rms = max(m_max, 2 * exc[1]), max(m_rms, 2 * exc[2])
        finite = bool(torch.isfinite(val).all())
        ok = finite and g_max <= m_max * r_max and g_rms <= m_rms * r_rms
        ratio = lambda g, r: g / r if r > 0 else (0.0 if g == 0 else float("inf"))   # E_ref = 0: an exactly-zero quantity
        print("pointwise_f64 | %-9s %-8s %-5s %-11s %-8s n %5d | max E_ref %.3e E_got %.3e ratio %6.2f (M %g) | rms E_ref %.3e E_got %.3e "
              "ratio %6.2f (M %g) | %s" % (kernel, q, eng, subject, pset, val.shape[0], r_max, g_max, ratio(g_max, r_max), m_max, r_rms,
                                            g_rms, ratio(g_rms, r_rms), m_rms, "ok" if ok else "OVER"))
        if not ok:   # the evidence a finding starts from: how many elements carry the error, and the worst of them
            e_ref, e_got = (o32[oq].double() - o64[oq]).abs().reshape(-1), (val.double().cpu() - o64[oq]).abs().reshape(-1)
            print("pointwise_f64 |   over: %d of %d elements have E_ref > 0, %d have E_got > max E_ref; worst (index, f64, ref32, got): %s" % (
                int((e_ref > 0).sum()), e_ref.numel(), int((e_got > r_max).sum()),
                [(int(i), float(o64[oq].reshape(-1)[i]), float(o32[oq].reshape(-1)[i]), float(val.reshape(-1)[i])) for i in e_got.argsort(descending=True)[:3]]))
            bad.append((q, round(ratio(g_max, r_max), 2), round(ratio(g_rms, r_rms), 2), finite))
    return bad


def measure(scene, kernel, subject, eng, pset):
    c = gpu_ctx(scene, subject, eng)
    inp = point_inputs(scene, subject, pset)
    o32, o64 = oracle_pair(scene, ORACLE_OF[kernel], subject, pset)
    c["ws"].ensure(1, 1)
    c["ws"].reset_counters()
    got = RUNNERS[kernel](c, on_gpu(inp, c["dev"]))
    torch.cuda.synchronize()
    return judge(kernel, eng, subject, pset, got, o32, o64), c["ws"].counters()["n_split_nonfinite"], got


KERNEL_CASES = [(k, s) for k in ("sdf", "skin", "jac", "color", "shade") for s in SUBJECTS[ORACLE_OF[k]]]


@gpu
@pytest.mark.parametrize("pset", ASSERTED_SETS)
@pytest.mark.parametrize("eng", ENGINES)
@pytest.mark.parametrize("kernel,subject", KERNEL_CASES)
def test_kernel_against_float64_oracle(scene, kernel, subject, eng, pset):
    bad, _, _ = measure(scene, kernel, subject, eng, pset)
    assert not bad, "(quantity, max ratio, rms ratio, finite) over the bound: %s" % bad


@gpu
@pytest.mark.parametrize("eng", ENGINES)
@pytest.mark.parametrize("kernel,subject", KERNEL_CASES)
def test_outer_is_never_silently_wrong(scene, kernel, subject, eng):
    """`outer` ([-3, 3]^3 minus the claimed cube: what query_posed and stray Broyden iterates can reach) is beyond what the
    code claims.  The rule there is "never silently wrong": every output finite, and a call either meets its M or leaves
    n_split_nonfinite > 0 in the workspace counters.

    Found on the MI355X (profiles/pointwise_f64.txt): the FIRST alternative.  Every kernel meets its M on `outer` on both
    engines with ratios like those of `claimed` (0.5 .. 1.3 for the fp32-class rows), the counter stays at zero, so `outer`
    is asserted like the other sets -- exception mechanism included: the Jacobian of the wide-range subject takes one
    (EXCEPTIONS: fp32 forward-mode differentiation, rms 4.33 against 4) -- and no domain limit had to be written down."""
    bad, nonfinite, got = measure(scene, kernel, subject, eng, "outer")
    for q, v in got.items():
        assert bool(torch.isfinite(v).all()), (q, "non-finite output")
    assert nonfinite == 0
    assert not bad, "(quantity, max ratio, rms ratio, finite) over the bound, and no range report: %s" % bad


@gpu
@pytest.mark.parametrize("eng", ENGINES)
@pytest.mark.parametrize("name,tag", F6_CASES)
def test_shade_composite_against_float64_oracle(scene, name, tag, eng):
    """arah_shade_composite on the F5/F6 fixtures' points, depths, transforms and masks against O.shade_composite."""
    from arah_release_amd import hip
    c, o32, o64 = _f6_oracle(scene, name, tag)
    S, dev = c["S"], torch.device("cuda:0")
    frame = hip_frame(c["frame"], dev, eng)
    samp = hip.Sampling(dev, S, int(c["g"]["n_near"]), int(c["g"]["n_far"]), c["cano"], False)
    rgb, acc, vol = hip.shade_composite(frame, hip.Workspace(dev), samp, c["d"].to(dev), c["z"].to(dev), c["pts"].to(dev),
                                        c["T"].to(dev), c["mask"].to(torch.uint8).to(dev))
    vm = torch.from_numpy(c["vol"])
    assert torch.equal(vol.cpu().bool(), vm)
    bad = judge("composite", eng, name, "f6_" + tag, dict(rgb=rgb.cpu()[vm], acc=acc.cpu()[vm]), o32, o64)
    assert not bad, "(quantity, max ratio, rms ratio, finite) over the bound: %s" % bad


# ------------------------------------------------------------------------------------------ GPU: shapes and isolation
PREFIXES = [0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 4095]
ISO_CASES = [("sdf", "zju377_mono"), ("skin", "zju377_mono"), ("jac", "zju377_mono"), ("color", "zju313"), ("shade", "zju313"),
             ("shade", "zju377_mono")]


def assert_same(a, b, what):
    for q in a:
        assert a[q].shape == b[q].shape and torch.equal(a[q], b[q]), "%s: %s differs (%d rows)" % (what, q, int(
            (a[q] != b[q]).reshape(a[q].shape[0], -1).any(-1).sum()) if a[q].shape == b[q].shape else -1)


def rows_of(out, rows):
    return {q: v[rows] for q, v in out.items()}


@gpu
@pytest.mark.parametrize("eng", ENGINES)
@pytest.mark.parametrize("kernel,subject", ISO_CASES)
def test_a_point_does_not_depend_on_its_call(scene, kernel, subject, eng):
    """Bit-exact against the n = 4096 run of `box`: prefixes, the set tiled to n = 100003, a permutation, 64 copies of one
    point, and a large call followed by a small one on one workspace (and the reverse)."""
    c = gpu_ctx(scene, subject, eng)
    hip, dev, run = c["hip"], c["dev"], RUNNERS[kernel]
    inp = on_gpu(point_inputs(scene, subject, "box"), dev)
    full = run(c, inp)
    for n in PREFIXES:
        out = run(c, on_gpu(inp, dev, slice(0, n)))
        for q, v in out.items():
            assert v.shape[0] == n and v.shape[1:] == full[q].shape[1:], (q, n, v.shape)
        assert_same(out, rows_of(full, slice(0, n)), "prefix n = %d" % n)
    tiled = torch.arange(100003, device=dev) % N_SET
    assert_same(run(c, on_gpu(inp, dev, tiled)), rows_of(full, tiled), "n = 100003 (tiled)")
    perm = torch.randperm(N_SET, generator=torch.Generator().manual_seed(5)).to(dev)
    assert_same(run(c, on_gpu(inp, dev, perm)), rows_of(full, perm), "permutation")
    same = torch.full((64,), 1234, device=dev)
    assert_same(run(c, on_gpu(inp, dev, same)), rows_of(full, same), "64 copies of one point")
    small = slice(100, 165)
    ws_a, ws_b = hip.Workspace(dev), hip.Workspace(dev)
    big_a = run(c, on_gpu(inp, dev, tiled), ws_a)
    small_a = run(c, on_gpu(inp, dev, small), ws_a)
    small_b = run(c, on_gpu(inp, dev, small), ws_b)
    big_b = run(c, on_gpu(inp, dev, tiled), ws_b)
    assert_same(small_a, rows_of(full, small), "small call after a large one")
    assert_same(small_b, rows_of(full, small), "small call on a fresh workspace")
    assert_same(big_a, rows_of(full, tiled), "large call on a fresh workspace")
    assert_same(big_b, rows_of(full, tiled), "large call after a small one")


MARK = 0x7FC0BEEF    # a quiet-NaN bit pattern no kernel produces
PAD = 64


def raw_call(c, kernel, inp, n, outs, ws):
    """The raw C entry, as arah_release_amd/hip.py calls it, on caller-owned output buffers."""
    hip = c["hip"]
    lib, f, p = hip.load_library(), C.byref(c["frame"].handle), hip._ptr
    buf = ws.ensure(max(n, 1), 1)
    tail = (p(buf), C.c_size_t(buf.numel()), hip._stream(c["dev"]))
    with hip._on_device(c["dev"]):
        if kernel == "sdf":
            rc = lib.arah_sdf_eval(f, p(inp["x"]), C.c_int32(n), p(outs["sdf"]), p(outs["feat"]), p(outs["grad"]), *tail)
        elif kernel == "skin":
            rc = lib.arah_skin_lbs(f, p(inp["x_hat"]), C.c_int32(n), p(outs["weights"]), p(outs["x_bar"]), p(outs["T"]), *tail)
        elif kernel == "jac":
            rc = lib.arah_skin_jacobian(f, p(inp["x_hat"]), C.c_int32(n), p(outs["jac"]), *tail)
        elif kernel == "color":
            rc = lib.arah_color_eval(f, p(inp["x"]), p(inp["normal"]), p(inp["d"]), p(inp["feat"]), C.c_int32(n), p(outs["rgb"]), *tail)
        else:
            rc = lib.arah_shade_points(f, p(inp["x"]), p(inp["T"]), p(inp["d"]), C.c_int32(n), C.c_int32(int(c["cano"])),
                                       C.c_int32(hip.default_shade_engine()), p(outs["rgbs"]), p(outs["sdfn"]), *tail)
    hip._check(rc, kernel)


RAW_OUTPUTS = dict(sdf=dict(sdf=(), feat=(256,), grad=(3,)), skin=dict(weights=(24,), x_bar=(3,), T=(4, 4)), jac=dict(jac=(3, 3)),
                   color=dict(rgb=(3,)), shade=dict(rgbs=(4,), sdfn=(4,)))


@gpu
@pytest.mark.parametrize("eng", ENGINES)
@pytest.mark.parametrize("kernel,subject", ISO_CASES)
def test_rows_past_n_are_left_alone(scene, kernel, subject, eng):
    """Through ctypes on the raw entry: output buffers 64 rows longer than n, pre-filled with a marker bit pattern; the
    rows >= n hold the marker after the call and the rows < n are the rows of the n = 4096 run."""
    c = gpu_ctx(scene, subject, eng)
    dev = c["dev"]
    inp = on_gpu(point_inputs(scene, subject, "box"), dev)
    full = RUNNERS[kernel](c, inp)
    if kernel == "shade":
        full = dict(rgbs=torch.cat([full["rgb"], full["density"][:, None]], -1), sdfn=torch.cat([full["sdf"][:, None], full["grad"]], -1))
    for n in (1, 63, 65, 4095):
        outs = {q: torch.full((n + PAD,) + shp, MARK, dtype=torch.int32, device=dev).view(torch.float32) for q, shp in RAW_OUTPUTS[kernel].items()}
        raw_call(c, kernel, on_gpu(inp, dev, slice(0, n)), n, outs, c["ws"])
        torch.cuda.synchronize()
        for q, v in outs.items():
            assert bool((v[n:].view(torch.int32) == MARK).all()), "%s: rows >= n = %d were written" % (q, n)
            assert torch.equal(v[:n], full[q][:n]), "%s: rows < n = %d differ from the long run" % (q, n)
