"""The two Broyden root solvers at their seams -- loop C (hip.broyden3_lbs -> k_canon_wave / k_canon_solve) and loop B
(hip.joint_root_find -> k_joint_iter + k_joint_finish) -- against FLOAT64 residuals at the point the kernel returns.

Criterion.  The path Broyden takes is chaotic in the last bits; the residual at the returned point is not.  With ``x, T, err,
conv`` from the kernel, the float64 frame and the fp32 oracle frame (tests/test_pointwise_f64.oracle_frames; the kernels get
the oracle's frame bit for bit, hip_frame) are evaluated AT THE KERNEL'S OWN x (and z for loop B):

    r64   = |residual64(x)|         loop C: LBS64(x) - tgt        loop B: (sdf64_metric(x), LBS64(x) - (o + z d - trans))
    E     = |residual32(x) - residual64(x)|,  e_set  = max E over the set      (the fp32 reference's own rounding error,
    E_T   = |T32(x) - T64(x)| per entry,      eT_set = max over the set         computed each run on the CPU)
    M     = 8    (the fp32-class bound of test_pointwise_f64.py: loop C's split MLP is the same f16 hi+lo arithmetic, loop B's
                  SDF and skinning evaluations are the seams that file holds to 8)
    ROOT_THRESH = 1e-5  (kRootThresh, RT:18)

  C1  a converged point is a root:            conv  =>  r64 <= ROOT_THRESH + M e_set
  C2  the reported residual is the residual:  |err - r64| <= M e_set + 4 2^-24 r64              (loop C, which returns err)
  C3  the transform belongs to the point:     x != x0 bitwise: max |T - T64(x)| <= M eT_set;  x == x0 bitwise: T is T0 bit
      for bit (the reference discards the T of the start's evaluation, broyden.py:35)
  C4  conv is exactly err < 1e-5 in float32 (loop C); loop B's rays outside `valid` keep x0, z0, T0 bit for bit and are
      never converged
  C5  best-iterate tracking:                  not conv  =>  r64(x) <= r64(x0) + M e_set
  C6  the same roots as float64: where the float64 oracle converges from the same start the kernel converges too, within
      2 (r64(x) + r64(x64)) / sigma_min(J64(x64)) of its root (the linearised distance between two points of one residual
      ball, doubled for the curvature).  Rows failing either half are COUNTED: at most 0.5 % of a set (SURVEY 8c's agreement
      fraction, the cap of the existing solver tests -- a cap on what the test may overlook, not a measurement).
  every returned value finite; n_split_nonfinite stays 0 on split frames.

C1-C5 hold on every set; C6 on `fixture`, `s005`, `s03`, `s10`, the ordinary rows of `special` and both ray sets (`outer`,
sigma = 0.3 m, has ~4 % hopeless starts and the two ORACLES' flags differ on 2 of 1024 there).  One line per row is printed
(``root_solvers_f64 | seam | kernel | engine | subject | set | ...``); profiles/root_solvers_f64.txt is the table of one
full run on the MI355X.  The call-shape tests at the bottom are bit-exact (a point's result does not
depend on which tile, wave or slot it lands in).

The CPU tests pin the float64 view of both solvers to the REFERENCE's recorded answers (F1, F17), check that the
yardsticks are not zero and that the fp32 oracle itself meets C1, C2, C3, C5 with M = 1 and C6 with no row left out.  Two
things that self-check taught about the yardstick:
  * the fp32 oracle's BLAS takes another path for a single row than for a matrix, and broyden() evaluates its last straggler
    alone: against a yardstick from the batched evaluation only, the oracle's own T and err stood at 1.06 .. 1.25.  The
    self-check's yardstick therefore takes the larger of the two paths per row (evaluate(alone=True)); the kernels are held
    to the batched one, the smaller.
  * on the wide-range subject's sampled sets e_set is 3e-5 .. 7e-4, above ROOT_THRESH itself, and the fp32 oracle misses
    1 .. 4 rows of 1024 that float64 solves: "no row left out" is asserted on zju377_mono and the two fixtures, the cap there.

What the first run on the MI355X found (the bounds above were fixed before it):
  * every row inside its bound, EXCEPTIONS is empty.  Loop C, zju377_mono: C1 excess <= 1.05 e_set (`outer`; <= 0 elsewhere),
    C2 <= 4.5 and C3 <= 3.2 (k_canon_wave on s03; the tile kernel <= 1.6 / 1.3), C6 leaves out no row on any kernel.  Wide-range
    subject (SCALED instance): C1 <= 0.6, C2 <= 1.5, C3 <= 2.3, C6 leaves out 0 .. 4 rows of 1024 (<= 0.39 %, all "not
    converged", none astray; the fp32 oracle alone: 1 .. 4).  Loop B, both engines: C1 <= 0.05, C3 <= 1.1, C6 none left out.
  * every call shape bit-equal: prefixes, permutation, 65 836 rows, WAVE == WAVE_L2 on every set, loop B's masks.
  * arah_broyden3_lbs refused n = 0 with ARAH_E_BADARG as hip.py calls it (an empty tensor's pointer is null and was
    checked before n): fixed in the entry, as the per-point seams were.  arah_joint_root_find already checked n first.
  * loop C carries the target in row 3 of T and hands back (0, 0, 0, T0[3][3]) there: "T is T0 bit for bit" holds for any
    T0 whose bottom row is (0, 0, 0, s) -- every transform of this model, F1's 7 I included; include/arah_hip.h says so now.
  * a target far from the body does not make a point "never converge" (test_special_rows_are_what_they_claim): `special`
    carries such rows AND hopeless starts that neither oracle solves, which are the ones that run all 51 evaluations.
  * the tests bite (scratch builds of k_canon_wave, split engine, both subjects): retirement at 2 kRootThresh -> C6 on all 10
    rows held to it, 14 .. 16 % not converged on zju377_mono, 1.3 .. 2.3 % on the wide subject; the last iterate's T stored
    instead of the best one's -> C3 on all 12 rows (1e3 .. 4e5 eT_set, or an unmoved row without its T0); lo products
    removed from the split GEMMs -> 11 of 12 rows: C1 at 11 .. 395, C2 at 301 .. 2192, C3 at 448 .. 1146, C6 at 1.1 .. 6.0 %.
"""
import numpy as np
import pytest
import torch

from conftest import golden
from oracle import arah_oracle as O
from test_hip_parity import assert_rows_close
from test_pointwise_f64 import _at_most_16_threads, gpu_ctx, oracle_frames  # noqa: F401  (the autouse fixture; gpu_ctx: hip_frame under engine)

gpu = pytest.mark.gpu

M = 8.0
ROOT_THRESH = O.ROOT_THRESH
THRESH_F32 = torch.tensor(1e-5, dtype=torch.float32)   # kRootThresh as the kernels compare it
C6_CAP = 0.005
N_C = 1024
SIGMAS = {"s005": 0.005, "s03": 0.03, "s10": 0.1, "outer": 0.3}
C_SETS = ["fixture", "s005", "s03", "s10", "outer", "special"]
C6_SETS = ["fixture", "s005", "s03", "s10", "special"]
C_SUBJECTS = ["zju377_mono", "wide"]
B_SETS = ["f1", "traced"]
# (engine, kernel): the fp32 engine always runs the tile kernel -- one row
C_KERNELS = [("split", "wave"), ("split", "wave_l2"), ("split", "tile"), ("fp32", "tile")]
C_ROWS = [(s, e, k) for s in C_SUBJECTS for e, k in C_KERNELS]
ENGINES = ["split", "fp32"]

# (seam, kernel, engine, subject, set, criterion) -> (measured ratio, reason): the row's M for that criterion becomes twice
# the measurement; M stays 8 for every other row.
EXCEPTIONS = {}


def m_of(row, crit):
    exc = EXCEPTIONS.get(row + (crit,))
    return max(M, 2.0 * exc[0]) if exc else M


# ------------------------------------------------------------------------------------------ residuals, both precisions
def resid_c(fr, x, tgt):
    xb, Tm = O.lbs_forward(fr, x, count=False)
    return xb - tgt, Tm


def resid_b(fr, x, z, o, d):
    """O.joint_root_find's residual (RFU:430-445) at (x, z)."""
    tgt = d * z[:, None] + o - fr.trans
    xb, Tm = O.lbs_forward(fr, x, count=False)
    sdf = O.sdf_forward(fr, O.normalize_points(fr, x), count=False)[0] * fr.sdf_scale
    return torch.cat([sdf[:, None], xb - tgt], dim=-1), Tm


def evaluate(fr, fr64, resid, args, u, alone=False):
    """r64, E, T64, E_T at u = (x,) or (x, z): the float64 residual and the fp32 oracle's distance from it.  alone: the fp32
    oracle also evaluates every row in a call of its own and the larger distance counts (see the CPU self-check)."""
    r32, T32 = resid(fr, *u, *args)
    r64, T64 = resid(fr64, *[v.double() for v in u], *[a.double() for a in args])
    E, ET = torch.linalg.norm(r32.double() - r64, dim=-1), (T32.double() - T64).abs().reshape(-1, 16).amax(-1)
    if alone:
        one = [resid(fr, *[v[i:i + 1] for v in u], *[a[i:i + 1] for a in args]) for i in range(u[0].shape[0])]
        r1, T1 = torch.cat([r for r, _ in one]), torch.cat([t for _, t in one])
        E = torch.maximum(E, torch.linalg.norm(r1.double() - r64, dim=-1))
        ET = torch.maximum(ET, (T1.double() - T64).abs().reshape(-1, 16).amax(-1))
    return dict(r64=torch.linalg.norm(r64, dim=-1), E=E, T64=T64, ET=ET)


# ------------------------------------------------------------------------------------------ loop C: point sets (CPU)
_CSETS = {}


def loop_c_set(scene, subject, name):
    """tgt, x0, T0 (fp32, CPU, seeded), `ordinary` (the rows held to C6) and for `special` the row kinds."""
    key = (subject, name)
    if key in _CSETS:
        return _CSETS[key]
    fr, _, _ = oracle_frames(scene, subject)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    kind = None
    if name == "fixture":
        g = golden("f1_broyden3.npz" if subject == "zju377_mono" else "f17_wide_skinning.npz")
        tgt, x0, T0 = t(g["tgt"]), t(g["x0"]), t(g["T0"])
    elif name in SIGMAS:
        gen = torch.Generator().manual_seed(20260301 + int(SIGMAS[name] * 1000))
        idx = torch.randint(0, fr.verts.shape[0], (N_C,), generator=gen)
        pts = fr.verts[idx] + SIGMAS[name] * torch.randn(N_C, 3, generator=gen)
        x0, T0 = O.nn_inverse_lbs(fr, pts)
        tgt = pts - fr.trans
    else:
        # row i: i % 16 == 3 starts on a root (kind 1: retires at its first step), i % 16 == 11 has its target moved 3 m
        # away from the body's centroid, the start left where it was (kind 2: a 3 m first step; most of these still find a
        # root, see test_special_rows_are_what_they_claim), i % 16 == 7 is a hopeless start (kind 3: sigma = 0.3 m draws on
        # which neither oracle comes within ten thresholds of a root: the rows that run all 51 evaluations), the rest are s03's rows
        # (kind 0) -- interleaved, so all kinds share waves and slots are refilled mid-flight
        base = loop_c_set(scene, subject, "s03")
        tgt, x0, T0 = base["tgt"].clone(), base["x0"].clone(), base["T0"].clone()
        rows = torch.arange(N_C)
        kind = torch.zeros(N_C, dtype=torch.long)
        kind[rows % 16 == 3] = 1
        kind[rows % 16 == 11] = 2
        kind[rows % 16 == 7] = 3
        tgt[kind == 1] = O.lbs_forward(fr, x0[kind == 1], count=False)[0]
        p = tgt[kind == 2] + fr.trans
        tgt[kind == 2] = tgt[kind == 2] + 3.0 * torch.nn.functional.normalize(p - fr.verts.mean(0), dim=-1)
        gen = torch.Generator().manual_seed(20260307)
        cand = fr.verts[torch.randint(0, fr.verts.shape[0], (4 * N_C,), generator=gen)] + 0.3 * torch.randn(4 * N_C, 3, generator=gen)
        cx0, cT0 = O.nn_inverse_lbs(fr, cand)
        fr64 = oracle_frames(scene, subject)[1]
        _, _, e32, ok32 = O.broyden3_lbs(fr, cand - fr.trans, cx0, cT0)
        _, _, e64, ok64 = O.broyden3_lbs(fr64, (cand - fr.trans).double(), cx0.double(), cT0.double())
        hopeless = (~ok32 & ~ok64 & (e32 > 10 * ROOT_THRESH) & (e64 > 10 * ROOT_THRESH)).nonzero()[:64, 0]
        assert hopeless.numel() == 64
        tgt[kind == 3], x0[kind == 3], T0[kind == 3] = (cand - fr.trans)[hopeless], cx0[hopeless], cT0[hopeless]
    assert bool((T0[:, 3, :3].contiguous().view(torch.int32) == 0).all())   # an affine bottom row, +0: what loop C's seam keeps
    S = dict(tgt=tgt.contiguous(), x0=x0.contiguous(), T0=T0.contiguous(), kind=kind,
             ordinary=torch.ones(tgt.shape[0], dtype=torch.bool) if kind is None else kind == 0)
    _CSETS[key] = S
    return S


def loop_c_reference(scene, subject, name):
    """Once per set: r64 at the start, the float64 oracle's roots from the same starts and sigma_min of its Jacobian there."""
    S = loop_c_set(scene, subject, name)
    if "x64" not in S:
        fr, fr64, _ = oracle_frames(scene, subject)
        tgt64 = S["tgt"].double()
        S["r64_0"] = torch.linalg.norm(resid_c(fr64, S["x0"].double(), tgt64)[0], dim=-1)
        x64, _, err64, conv64 = O.broyden3_lbs(fr64, tgt64, S["x0"].double(), S["T0"].double())
        S.update(x64=x64, conv64=conv64, r64_x64=err64, smin=torch.linalg.svdvals(O.lbs_jacobian(fr64, x64))[:, -1])
    return S


def loop_c_oracle32(scene, subject, name):
    S = loop_c_set(scene, subject, name)
    if "o32" not in S:
        fr, _, _ = oracle_frames(scene, subject)
        x, Tm, err, conv = O.broyden3_lbs(fr, S["tgt"], S["x0"], S["T0"])
        S["o32"] = dict(x=x, T=Tm, err=err, conv=conv)
    return S["o32"]


# ------------------------------------------------------------------------------------------ loop B: ray sets (CPU)
_BSETS = {}


def loop_b_set(scene, name):
    """cam (1,3), o (N,3), d, valid, x0, z0, T0 of zju377_mono: F1's 256 rays, or the rays of a 64 x 64 frame with the
    fp32 oracle's sphere-tracing results as starts (every ray is passed; valid = ~diverged)."""
    if name in _BSETS:
        return _BSETS[name]
    fr, _, _ = oracle_frames(scene, "zju377_mono")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    if name == "f1":
        g = golden("f1_broyden4.npz")
        cam, d, valid, x0, z0, T0 = t(g["cam"][:1]), t(g["rays"]), t(g["valid"]), t(g["x0"]), t(g["z0"]), t(g["T0"])
        assert bool((t(g["cam"]) == cam).all())
    else:
        inputs = scene.make_inputs(64, 64, frame_idx=0)
        cam, d, nf = inputs["cam_loc"].reshape(1, 3), inputs["ray_dirs"][0].contiguous(), inputs["body_bounds_intersections"][0]
        x0, T0, z0, diverged = O.sphere_trace(fr, cam.expand(d.shape[0], 3), d, nf[:, 0].contiguous(), nf[:, 1].contiguous())
        valid = ~diverged
    S = dict(cam=cam.contiguous(), o=cam.expand(d.shape[0], 3).contiguous(), d=d.contiguous(), valid=valid, x0=x0.contiguous(),
             z0=z0.contiguous(), T0=T0.contiguous(), ordinary=valid.clone())
    _BSETS[name] = S
    return S


def jacobian_b(fr, x, d):
    """The 4 x 4 system of loop B (RFU:406-417) at x: rows (d sdf_metric / dx, 0) and (d LBS / dx, -d)."""
    J = torch.zeros(x.shape[0], 4, 4, dtype=x.dtype)
    J[:, 1:, :3] = O.lbs_jacobian(fr, x)
    with torch.enable_grad():
        xg = x.detach().clone().requires_grad_(True)
        sdf = O.sdf_forward(fr, O.normalize_points(fr, xg), count=False)[0] * fr.sdf_scale
        J[:, 0, :3] = torch.autograd.grad(sdf.sum(), xg)[0]
    J[:, 1:, 3] = -d
    return J


def loop_b_reference(scene, name):
    S = loop_b_set(scene, name)
    if "x64" not in S:
        fr, fr64, _ = oracle_frames(scene, "zju377_mono")
        o64, d64 = S["o"].double(), S["d"].double()
        S["r64_0"] = torch.linalg.norm(resid_b(fr64, S["x0"].double(), S["z0"].double(), o64, d64)[0], dim=-1)
        x64, z64, _, conv64 = O.joint_root_find(fr64, o64, d64, S["valid"], S["x0"].double(), S["z0"].double(), S["T0"].double())
        S.update(x64=torch.cat([x64, z64[:, None]], -1), conv64=conv64,
                 r64_x64=torch.linalg.norm(resid_b(fr64, x64, z64, o64, d64)[0], dim=-1),
                 smin=torch.linalg.svdvals(jacobian_b(fr64, x64, d64))[:, -1])
    return S


def loop_b_oracle32(scene, name):
    S = loop_b_set(scene, name)
    if "o32" not in S:
        fr, _, _ = oracle_frames(scene, "zju377_mono")
        x, z, Tm, conv = O.joint_root_find(fr, S["o"], S["d"], S["valid"], S["x0"], S["z0"], S["T0"])
        S["o32"] = dict(x=x, z=z, T=Tm, conv=conv)
    return S["o32"]


# ------------------------------------------------------------------------------------------ the judge
def bits_equal(a, b):
    return (a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).reshape(a.shape[0], -1).all(-1)


def judge(row, S, out, fr, fr64, m=None, c6=True, on=None, nonfinite=0, alone=False):
    """Print the row's table line; return the list of criteria it misses.  row = (seam, kernel, engine, subject, set);
    out: x, T, conv and err (loop C) or z (loop B) on the CPU; on: the rows the solver was asked to solve (loop B's mask);
    m: one M for every criterion (the CPU tests' M = 1), default M with the row's EXCEPTIONS."""
    seam = row[0]
    mm = (lambda crit: m) if m is not None else (lambda crit: m_of(row, crit))
    n = out["x"].shape[0]
    on = torch.ones(n, dtype=torch.bool) if on is None else on
    conv = out["conv"].bool()
    bad = []
    finite = all(bool(torch.isfinite(out[k]).all()) for k in ("x", "T", "err", "z") if k in out)
    if not finite:
        print("root_solvers_f64 | %s | non-finite output" % " | ".join(row))
        return ["finite"]
    if seam == "C":
        u, u0, ev = (out["x"],), (S["x0"],), evaluate(fr, fr64, resid_c, (S["tgt"],), (out["x"],), alone)
    else:
        u, u0, ev = (out["x"], out["z"]), (S["x0"], S["z0"]), evaluate(fr, fr64, resid_b, (S["o"], S["d"]), (out["x"], out["z"]), alone)
    r64 = ev["r64"]
    e_set, eT_set = float(ev["E"][on].max()) if bool(on.any()) else 0.0, float(ev["ET"][on].max()) if bool(on.any()) else 0.0
    ratio = lambda v, e: v / e if e > 0 else (0.0 if v <= 0 else float("inf"))
    # C1
    c1 = float((r64[conv] - ROOT_THRESH).max()) if bool(conv.any()) else float("-inf")
    if c1 > mm("C1") * e_set:
        bad.append("C1")
    # C2, C4 (loop C)
    c2 = float("nan")
    if seam == "C":
        err = out["err"]
        c2v = (err.double() - r64).abs()
        c2 = float(c2v.max())
        if bool((c2v > mm("C2") * e_set + 4.0 * 2.0 ** -24 * r64).any()):
            bad.append("C2")
        if not torch.equal(conv, err < THRESH_F32):
            bad.append("C4")
    # C3
    moved = on & ~torch.stack([bits_equal(a.reshape(n, -1), b.reshape(n, -1)) for a, b in zip(u, u0)]).all(0)
    dT = (out["T"].double() - ev["T64"]).abs().reshape(n, 16).amax(-1)
    c3 = float(dT[moved].max()) if bool(moved.any()) else 0.0
    kept = bits_equal(out["T"].reshape(n, 16), S["T0"].reshape(n, 16))
    if c3 > mm("C3") * eT_set:
        bad.append("C3")
    if not bool(kept[~moved].all()):
        bad.append("C3/T0")
    # C4 (loop B): rays outside the mask
    if seam == "B":
        off = ~on
        if bool(conv[off].any()) or not bool((bits_equal(out["x"], S["x0"]) & bits_equal(out["z"][:, None], S["z0"][:, None]))[off].all()):
            bad.append("C4")
    # C5
    lost = on & ~conv
    c5 = float((r64[lost] - S["r64_0"][lost]).max()) if bool(lost.any()) else float("-inf")
    if c5 > mm("C5") * e_set:
        bad.append("C5")
    # C6
    c6_txt = "-"
    if c6:
        rows = S["ordinary"] & on & S["conv64"]
        uu = torch.cat([v.reshape(n, -1) for v in u], -1).double()
        dist = torch.linalg.norm(uu - S["x64"], dim=-1)
        bound = 2.0 * (r64 + S["r64_x64"]) / S["smin"]
        missed, astray = rows & ~conv, rows & conv & (dist > bound)
        n_held = int((S["ordinary"] & on).sum())
        share = float((missed | astray).sum()) / max(n_held, 1)
        near = rows & conv
        c6_txt = "%d missed %d astray of %d (%.3f %%), worst dist/bound %.3f" % (
            int(missed.sum()), int(astray.sum()), n_held, 100.0 * share, float((dist / bound)[near].max()) if bool(near.any()) else 0.0)
        if share > C6_CAP:
            bad.append("C6")
    if nonfinite:
        bad.append("n_split_nonfinite")
    print("root_solvers_f64 | %s | n %5d on %5d conv %5d unmoved %4d | e_set %.3e eT_set %.3e | C1 (r64 - thr)/e %7.2f | C2 |err - r64|/e %6.2f | "
          "C3 dT/eT %6.2f | C5 (r64 - r64_0)/e %9.2f | C6 %s | nonfinite %d | %s" % (
              " | ".join("%-11s" % v if i == 3 else "%-7s" % v if i in (1, 4) else v for i, v in enumerate(row)), n, int(on.sum()),
              int(conv.sum()), int((on & ~moved).sum()), e_set, eT_set, ratio(c1, e_set) if c1 > float("-inf") else float("nan"),
              ratio(c2, e_set), ratio(c3, eT_set), ratio(c5, e_set) if c5 > float("-inf") else float("nan"), c6_txt, nonfinite,
              "ok" if not bad else "OVER " + ",".join(bad)))
    out["_e_set"] = e_set
    return bad


# ------------------------------------------------------------------------------------------ CPU: the float64 view
def test_float64_loop_c_is_pinned_to_the_reference(scene):
    """O.broyden3_lbs in float64 on F1 and F17 against the reference's recorded fp32 answers, at the tolerances of
    test_broyden3 and test_wide_range_skinning_network -- and O.broyden3_lbs in fp32 is what test_oracle_golden's F1 test
    computes with the fixture's own J^-1_0."""
    for subject, name, flags, atol, frac in (("zju377_mono", "f1_broyden3.npz", 0.995, 2e-5, 0.99), ("wide", "f17_wide_skinning.npz", 0.99, 5e-5, 0.98)):
        g = golden(name)
        S = loop_c_reference(scene, subject, "fixture")
        assert S["x64"].dtype == torch.float64
        ok, valid = S["conv64"].numpy(), g["valid"]
        assert (ok == valid).mean() >= flags
        both = ok & valid
        assert both.sum() > 200
        assert_rows_close(S["x64"].numpy()[both], g["result"][both], atol=atol, frac=frac)
        _, T64, _, _ = O.broyden3_lbs(oracle_frames(scene, subject)[1], S["tgt"].double(), S["x0"].double(), S["T0"].double())
        assert_rows_close(T64.numpy()[both], g["transforms"][both], atol=1e-4, rtol=1e-3, frac=0.99)
        never = np.isclose(g["transforms"][:, 0, 0], 7.0)
        assert (np.isclose(T64.numpy()[:, 0, 0], 7.0) == never).mean() >= 0.99
    g = golden("f1_broyden3.npz")
    fr = oracle_frames(scene, "zju377_mono")[0]
    t = lambda a: torch.from_numpy(a)

    def resid(x, k):
        xb, Tm = O.lbs_forward(fr, x)
        return xb - t(g["tgt"])[k], Tm

    a = O.broyden(resid, t(g["x0"]), t(g["T0"]), t(g["Jinv0"]))
    b = O.broyden3_lbs(fr, t(g["tgt"]), t(g["x0"]), t(g["T0"]))
    assert (a[3] == b[3]).float().mean() >= 0.995
    assert_rows_close(a[0].numpy()[(a[3] & b[3]).numpy()], b[0].numpy()[(a[3] & b[3]).numpy()], atol=2e-5, frac=0.99)


def test_float64_loop_b_is_pinned_to_the_reference(scene):
    """O.joint_root_find in float64 on F1 against the reference's recorded fp32 answers, at test_joint_root_find's tolerances."""
    g = golden("f1_broyden4.npz")
    S = loop_b_reference(scene, "f1")
    fr64 = oracle_frames(scene, "zju377_mono")[1]
    x, z, Tm, conv = O.joint_root_find(fr64, S["o"].double(), S["d"].double(), S["valid"], S["x0"].double(), S["z0"].double(), S["T0"].double())
    assert x.dtype == z.dtype == Tm.dtype == torch.float64
    x, z, Tm, conv = x.numpy(), z.numpy(), Tm.numpy(), conv.numpy()
    ref_conv = g["converged"]
    assert (conv == ref_conv).mean() >= 0.995
    both = conv & ref_conv
    assert both.sum() > 200
    assert_rows_close(x[both], g["x_opt"][both], atol=2e-5, frac=0.99)
    assert_rows_close(z[both][:, None], g["z_opt"][both][:, None], atol=2e-5, frac=0.99)
    assert_rows_close(Tm[both].reshape(-1, 16), g["T_opt"][both].reshape(-1, 16), atol=1e-4, rtol=1e-3, frac=0.99)
    off = ~g["valid"]
    np.testing.assert_array_equal(x[off], g["x0"][off].astype(np.float64))
    np.testing.assert_array_equal(z[off], g["z0"][off].astype(np.float64))
    np.testing.assert_array_equal(Tm[off], g["T0"][off].astype(np.float64))
    assert not conv[off].any()


def test_float64_sphere_trace_follows_its_inputs(scene):
    """O.sphere_trace allocates in the dtype of its inputs: the float64 view traces the same rays to the same depths."""
    fr, fr64, _ = oracle_frames(scene, "zju377_mono")
    inputs = scene.make_inputs(16, 16, frame_idx=0)
    d, nf = inputs["ray_dirs"][0], inputs["body_bounds_intersections"][0]
    o = inputs["cam_loc"].reshape(1, 3).expand(d.shape[0], 3)
    a = O.sphere_trace(fr, o, d, nf[:, 0].contiguous(), nf[:, 1].contiguous())
    b = O.sphere_trace(fr64, o.double(), d.double(), nf[:, 0].double(), nf[:, 1].double())
    assert a[0].dtype == a[1].dtype == a[2].dtype == torch.float32 and b[0].dtype == b[1].dtype == b[2].dtype == torch.float64
    same = ~a[3] & ~b[3]
    assert (a[3] == b[3]).float().mean() >= 0.995 and int(same.sum()) > 10
    assert_rows_close(a[2][same].numpy()[:, None], b[2][same].numpy()[:, None], atol=2e-4, frac=0.99)


def test_special_rows_are_what_they_claim(scene):
    """`special`: per 16 rows one that starts on a root, one whose target lies 3 m further out (at least 2 m from the body),
    one hopeless start that neither oracle solves, 13 ordinary ones.  (Targets far from the body do NOT "never converge" on
    this model: the first Broyden step is the nearest vertex's inverse transform of the whole offset and lands next to a
    root of the extrapolated skinning field -- 40 to 50 of the 64 converge in fp32 and float64 alike.  The rows that run all
    51 evaluations are the hopeless starts.)"""
    for subject in C_SUBJECTS:
        S = loop_c_reference(scene, subject, "special")
        fr = oracle_frames(scene, subject)[0]
        o32 = loop_c_oracle32(scene, subject, "special")
        kind = S["kind"]
        assert [int((kind == k).sum()) for k in (0, 1, 2, 3)] == [832, 64, 64, 64]
        for c in range(0, N_C, 16):
            assert sorted(set(kind[c:c + 16].tolist())) == [0, 1, 2, 3]
        assert bool((S["r64_0"][kind == 1] < ROOT_THRESH).all()) and bool(o32["conv"][kind == 1].all())
        assert float(torch.cdist(S["tgt"][kind == 2] + fr.trans, fr.verts).min()) >= 2.0
        assert not bool(o32["conv"][kind == 3].any()) and not bool(S["conv64"][kind == 3].any())
        print("special | %-11s far targets: %d of 64 converge in fp32, %d in float64" % (subject, int(o32["conv"][kind == 2].sum()), int(S["conv64"][kind == 2].sum())))


@pytest.mark.parametrize("name", C_SETS)
@pytest.mark.parametrize("subject", C_SUBJECTS)
def test_fp32_oracle_meets_the_criteria_loop_c(scene, subject, name):
    """The yardstick is not vacuous (e_set, eT_set > 0) and the fp32 oracle itself meets C1, C2, C3, C5 with M = 1 on every
    set and C6 with no row left out."""
    fr, fr64, _ = oracle_frames(scene, subject)
    S = loop_c_reference(scene, subject, name)
    out = dict(loop_c_oracle32(scene, subject, name))
    bad = judge(("C", "oracle", "fp32cpu", subject, name), S, out, fr, fr64, m=1.0, c6=name in C6_SETS, alone=True)
    assert out["_e_set"] > 0
    assert not bad, bad
    # "no row left out" where the reference's rounding error stays below the threshold it solves to: zju377_mono and both
    # fixtures.  On the wide-range subject's sampled sets e_set is 4e-5 .. 7e-4 against ROOT_THRESH = 1e-5 (logits of several
    # thousand), whether the fp32 oracle gets below 1e-5 is luck there, and it misses 1 .. 4 rows of 1024 (0.1 .. 0.4 %) that
    # float64 solves: held to the cap like the kernels (judge above).
    if name in C6_SETS and (subject == "zju377_mono" or name == "fixture"):
        rows = S["ordinary"] & S["conv64"]
        dist = torch.linalg.norm(out["x"].double() - S["x64"], dim=-1)
        r64 = torch.linalg.norm(resid_c(fr64, out["x"].double(), S["tgt"].double())[0], dim=-1)
        assert bool(out["conv"][rows].all()) and bool((dist <= 2.0 * (r64 + S["r64_x64"]) / S["smin"])[rows].all())


@pytest.mark.parametrize("name", B_SETS)
def test_fp32_oracle_meets_the_criteria_loop_b(scene, name):
    fr, fr64, _ = oracle_frames(scene, "zju377_mono")
    S = loop_b_reference(scene, name)
    out = dict(loop_b_oracle32(scene, name))
    bad = judge(("B", "oracle", "fp32cpu", "zju377_mono", name), S, out, fr, fr64, m=1.0, on=S["valid"], alone=True)
    assert out["_e_set"] > 0 and int(S["valid"].sum()) >= 200
    assert not bad, bad
    rows = S["valid"] & S["conv64"]
    uu = torch.cat([out["x"], out["z"][:, None]], -1).double()
    r64 = torch.linalg.norm(resid_b(fr64, out["x"].double(), out["z"].double(), S["o"].double(), S["d"].double())[0], dim=-1)
    assert bool(out["conv"][rows].all())
    assert bool((torch.linalg.norm(uu - S["x64"], dim=-1) <= 2.0 * (r64 + S["r64_x64"]) / S["smin"])[rows].all())


# ------------------------------------------------------------------------------------------ GPU: the seams
def kernel_id(c, kern):
    return dict(wave=c["hip"].CANON_KERNEL_WAVE, wave_l2=c["hip"].CANON_KERNEL_WAVE_L2, tile=c["hip"].CANON_KERNEL_TILE)[kern]


def call_c(c, kern, S, rows=None):
    """hip.broyden3_lbs on the rows of a set -> dict of CPU tensors."""
    pick = lambda v: (v if rows is None else v[rows]).contiguous().to(c["dev"])
    x, Tm, err, conv = c["hip"].broyden3_lbs(c["frame"], c["ws"], pick(S["tgt"]), pick(S["x0"]), pick(S["T0"]), canon_kernel=kernel_id(c, kern))
    torch.cuda.synchronize()
    return dict(x=x.cpu(), T=Tm.cpu(), err=err.cpu(), conv=conv.cpu())


def call_b(c, S, valid=None, rows=None):
    pick = lambda v: (v if rows is None else v[rows]).contiguous().to(c["dev"])
    valid = S["valid"] if valid is None else valid
    x, z, Tm, conv = c["hip"].joint_root_find(c["frame"], c["ws"], S["cam"].to(c["dev"]), pick(S["d"]), pick(valid), pick(S["x0"]), pick(S["z0"]),
                                            pick(S["T0"]))
    torch.cuda.synchronize()
    return dict(x=x.cpu(), z=z.cpu(), T=Tm.cpu(), conv=conv.cpu())


_RUNS = {}


def run_c(scene, subject, eng, kern, name):
    """The full call of a set (cached: the table row, WAVE == WAVE_L2 and the call-shape tests share it) and its counter."""
    key = (subject, eng, kern, name)
    if key not in _RUNS:
        c = gpu_ctx(scene, subject, eng)
        c["ws"].ensure(1, 1)
        c["ws"].reset_counters()
        out = call_c(c, kern, loop_c_set(scene, subject, name))
        _RUNS[key] = (out, c["ws"].counters()["n_split_nonfinite"])
    return _RUNS[key]


def run_b(scene, eng, name):
    key = ("B", eng, name)
    if key not in _RUNS:
        c = gpu_ctx(scene, "zju377_mono", eng)
        c["ws"].ensure(1, 1)
        c["ws"].reset_counters()
        out = call_b(c, loop_b_set(scene, name))
        _RUNS[key] = (out, c["ws"].counters()["n_split_nonfinite"])
    return _RUNS[key]


@gpu
@pytest.mark.parametrize("name", C_SETS)
@pytest.mark.parametrize("subject,eng,kern", C_ROWS)
def test_loop_c_against_float64_residuals(scene, subject, eng, kern, name):
    fr, fr64, _ = oracle_frames(scene, subject)
    S = loop_c_reference(scene, subject, name)
    out, nonfinite = run_c(scene, subject, eng, kern, name)
    bad = judge(("C", kern, eng, subject, name), S, dict(out), fr, fr64, c6=name in C6_SETS, nonfinite=nonfinite if eng == "split" else 0)
    assert not bad, "criteria missed: %s" % bad


@gpu
@pytest.mark.parametrize("name", C_SETS)
@pytest.mark.parametrize("subject", C_SUBJECTS)
def test_wave_and_wave_l2_are_bit_equal(scene, subject, name):
    """The same arithmetic on operands delivered differently (hi fragments from LDS or from L2): equal on every set."""
    a, _ = run_c(scene, subject, "split", "wave", name)
    b, _ = run_c(scene, subject, "split", "wave_l2", name)
    for q in ("x", "T", "err", "conv"):
        assert torch.equal(a[q], b[q]), q


@gpu
@pytest.mark.parametrize("name", B_SETS)
@pytest.mark.parametrize("eng", ENGINES)
def test_loop_b_against_float64_residuals(scene, eng, name):
    fr, fr64, _ = oracle_frames(scene, "zju377_mono")
    S = loop_b_reference(scene, name)
    out, nonfinite = run_b(scene, eng, name)
    bad = judge(("B", "joint", eng, "zju377_mono", name), S, dict(out), fr, fr64, on=S["valid"], nonfinite=nonfinite if eng == "split" else 0)
    assert not bad, "criteria missed: %s" % bad


def mask_patterns(S):
    n = S["valid"].shape[0]
    last = torch.zeros(n, dtype=torch.bool)
    last[-1] = True
    return dict(all_off=torch.zeros(n, dtype=torch.bool), alternating=torch.arange(n) % 2 == 0, last_on=last)


@gpu
@pytest.mark.parametrize("eng", ENGINES)
def test_loop_b_mask_patterns(scene, eng):
    """`traced` under other masks (all off, every second ray, only the last): C1, C3, C4, C5 as above -- the alternating
    mask also sends diverged rays' starts into the solver -- and a ray solved under both masks gets the same answer bit
    for bit."""
    fr, fr64, _ = oracle_frames(scene, "zju377_mono")
    S = loop_b_reference(scene, "traced")
    c = gpu_ctx(scene, "zju377_mono", eng)
    full, _ = run_b(scene, eng, "traced")
    for pname, mask in mask_patterns(S).items():
        out = call_b(c, S, valid=mask)
        bad = judge(("B", "joint", eng, "zju377_mono", "traced/" + pname), S, dict(out), fr, fr64, c6=False, on=mask)
        assert not bad, "%s: criteria missed: %s" % (pname, bad)
        both = mask & S["valid"]
        for q in ("x", "z", "T", "conv"):
            assert torch.equal(out[q][both], full[q][both]), (pname, q)


# ------------------------------------------------------------------------------------------ GPU: call shapes, bit-exact
C_PREFIXES = [0, 1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023]
B_PREFIXES = [0, 1, 15, 16, 17, 63, 64, 65, 257]
N_LARGE = 65536 + 300      # more than one workgroup per CU holds at once: workgroups return to the queue


def assert_same(a, b, what):
    for q in a:
        if q.startswith("_"):
            continue
        assert a[q].shape == b[q].shape, (what, q, a[q].shape, b[q].shape)
        assert torch.equal(a[q], b[q]), "%s: %s differs in %d rows" % (what, q, int((a[q] != b[q]).reshape(a[q].shape[0], -1).any(-1).sum()))


def rows_of(out, rows):
    return {q: v[rows] for q, v in out.items() if not q.startswith("_")}


@gpu
@pytest.mark.parametrize("subject,eng,kern", C_ROWS)
def test_loop_c_point_does_not_depend_on_its_call(scene, subject, eng, kern):
    """Bit-exact against the 1024-row call of `special` (points that retire at once, points that never do and ordinary ones
    share waves): prefixes around a wave's 32 slots, the 64-seed chunk and a workgroup's 256 points, a permutation, and the
    set tiled to 65 836 rows."""
    S = loop_c_set(scene, subject, "special")
    c = gpu_ctx(scene, subject, eng)
    full, _ = run_c(scene, subject, eng, kern, "special")
    for n in C_PREFIXES:
        out = call_c(c, kern, S, slice(0, n))
        assert out["x"].shape == (n, 3) and out["T"].shape == (n, 4, 4) and out["err"].shape == (n,) and out["conv"].shape == (n,)
        assert_same(out, rows_of(full, slice(0, n)), "prefix n = %d" % n)
    perm = torch.randperm(N_C, generator=torch.Generator().manual_seed(7))
    assert_same(call_c(c, kern, S, perm), rows_of(full, perm), "permutation")
    tiled = torch.arange(N_LARGE) % N_C
    assert_same(call_c(c, kern, S, tiled), rows_of(full, tiled), "n = %d (tiled)" % N_LARGE)


@gpu
@pytest.mark.parametrize("eng", ENGINES)
def test_loop_b_ray_does_not_depend_on_its_call(scene, eng):
    """Bit-exact against the full call of `traced`: prefixes and a permutation."""
    S = loop_b_set(scene, "traced")
    c = gpu_ctx(scene, "zju377_mono", eng)
    full, _ = run_b(scene, eng, "traced")
    n_all = S["valid"].shape[0]
    assert n_all > max(B_PREFIXES)
    for n in B_PREFIXES:
        out = call_b(c, S, rows=slice(0, n))
        assert out["x"].shape == (n, 3) and out["z"].shape == (n,) and out["T"].shape == (n, 4, 4) and out["conv"].shape == (n,)
        assert_same(out, rows_of(full, slice(0, n)), "prefix n = %d" % n)
    perm = torch.randperm(n_all, generator=torch.Generator().manual_seed(7))
    assert_same(call_b(c, S, rows=perm), rows_of(full, perm), "permutation")
