"""Run from the repository root: `timeout -k 10 600 python tools/probes/tier_audit_cost.py` (one GPU).
Cost of the certificate's audit on bench.py's workload (512 x 512 x 64, zju377_mono synthetic): torch events around
(1) a tiered frame through the model entry, (2) arah_tier_audit alone behind it at rates 1 and 1/16, (3) the policy modes."""
import json, os, sys, time
sys.path.insert(0, os.getcwd())
import torch
from arah_release_amd import config, hip, synthetic

dev = torch.device("cuda:0")
model, _ = config.build_synthetic_model("zju377_mono", 64, 16, 16, device=dev)
idhr = model.idhr_network
idhr.adaptive_shading = False
scene = synthetic.SyntheticScene(0)
frames = [scene.make_inputs(512, 512, frame_idx=i, device=dev) for i in range(8)]
last = {}
orig = hip.render
def cap(frame, ws, samp, cam, d, nf, pose34, tiered=False):
    out = orig(frame, ws, samp, cam, d, nf, pose34, tiered=tiered)
    last.update(frame=frame, ws=ws, samp=samp, cam=cam, d=d, nf=nf)
    return out
hip.render = cap

def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); r = fn(); b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b), r

res = {"frame_ms": [], "audit_ms": {0: [], 4: []}, "results": {0: [], 4: []}}
with torch.no_grad():
    for _ in range(3):
        model(dict(frames[0]), eval=True)
    torch.cuda.synchronize()
    for rep in range(3):
        for i, inp in enumerate(frames):
            t, _ = timed(lambda: model(dict(inp), eval=True))
            res["frame_ms"].append(t)
            for k in (0, 4):
                ta, blk = timed(lambda: hip.tier_audit(last["frame"], last["ws"], last["samp"], last["cam"], last["d"], last["nf"], k, rep * 8 + i))
                res["audit_ms"][k].append(ta)
                if rep == 0:
                    res["results"][k].append(hip.audit_result(blk))
    # the policy: wall time per frame over 32 frames, stream drained at the end only
    for mode, every, k in (("off", 16, 4), ("sample", 16, 4), ("sample", 16, 0), ("strict", 1, 4), ("strict", 1, 0)):
        idhr.tier_audit, idhr.tier_audit_every, idhr.tier_audit_rate_log2, idhr.tiering = mode, every, k, True
        for inp in frames[:2]:
            model(dict(inp), eval=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for j in range(32):
            model(dict(frames[j % 8]), eval=True)
        torch.cuda.synchronize()
        res.setdefault("policy_ms", {})["%s every=%d rate=1/%d" % (mode, every, 1 << k)] = (time.perf_counter() - t0) / 32 * 1e3
        assert idhr.tier_violations == 0 and idhr.tiering
med = lambda v: sorted(v)[len(v) // 2]
summary = {"frame_ms_median": med(res["frame_ms"]), "audit_ms_median": {str(k): med(v) for k, v in res["audit_ms"].items()},
           "audit_ms_min_max": {str(k): [min(v), max(v)] for k, v in res["audit_ms"].items()}, "policy_ms": res["policy_ms"],
           "results_rate1_frame0": res["results"][0][0], "results_rate16_frame0": res["results"][4][0],
           "violations": sum(r["violations"] for v in res["results"].values() for r in v),
           "min_ratio_min": min(r["min_ratio"] for v in res["results"].values() for r in v)}
print(json.dumps(summary, indent=1))
