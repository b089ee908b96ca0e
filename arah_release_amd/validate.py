"""Score rendered frames against the captured images -- the reference's ``validate.py`` (validate.py:1-106) on this build.

    python -m arah_release_amd.validate CONFIG.yaml                      # training views, the config's val frames
    python -m arah_release_amd.validate CONFIG.yaml --novel-view         # every 30th frame of the val views
    python -m arah_release_amd.validate CONFIG.yaml --novel-pose [--novel-pose-view 1]
    python -m arah_release_amd.validate CONFIG.yaml --geometry DIR       # + geometry scores against DIR/<frame>.{npz,ply}
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m arah_release_amd.validate CONFIG.yaml ...

Same arguments and the same overrides of the configuration as validate.py:42-50.  The model is sized from the TRAINING
dataset (latent codes, optimised cameras and SMPL parameters: validate.py:57,65) and loaded from
``<out_dir>/checkpoints/last.ckpt``; the frames come from the ``val`` dataset (``test`` with --novel-pose) as validation
items (data.validation_item), go through ``LightningModel.validation_step(metrics="device")`` with
renderer.frames_in_flight of them in flight -- PSNR and SSIM are computed on the GPU (hip.image_metrics) and read once per
chunk -- and are aggregated by ``validation_epoch_end``.  With N processes frame i goes to rank i mod N.  Rank 0 prints one
JSON line (means, frame count, seconds per frame) and writes the per-frame values to ``<out_dir>/validation.json``.
LPIPS needs VGG weights that are not part of this build: ``--lpips MODULE:FUNCTION`` names a callable
(pred HxWx3, gt HxWx3, box mask) -> float to import; without it no LPIPS is reported.
``--geometry DIR``: every frame whose ground truth exists as ``DIR/<name of the frame's model file>.npz`` or ``.ply`` is also
scored against it in world metres (MetaAvatarRender.geometry_metrics: Chamfer distance, accuracy / completeness, normal
consistency, Hausdorff distances; DESIGN.md "Geometry metrics on the device").  A file with faces is a mesh (keys ``vertices``,
``faces``), one without is a scan (geometry.load_geometry: ``points`` [, ``normals``], or a vertex-only PLY; DESIGN.md "Scoring
against point clouds") -- a directory may mix the two; a frame scored against a scan without normals has ``normal_consistency``
null, and the mean of a score runs over the frames that have it (null when none has).  The
scalars stay on the device until the epoch ends; the JSON line gains their means over the scored frames and ``n_geometry``,
the number of such frames.  ``--geometry-thresholds 0.005,0.01,0.02`` adds ``precision@T``, ``recall@T`` and ``fscore@T`` for
every distance T in metres (keys formatted with ``repr(float)``), per frame and as means.  ``--geometry-iou N`` adds ``iou``, the
volumetric intersection over union of the posed mesh and the ground-truth mesh from N uniform points (geometry.mesh_iou; DESIGN.md
"Containment, occupancy grids and IoU on the device"), to the frames whose ground truth is a mesh -- a frame scored against a scan
gets no ``iou`` -- and its mean over those frames to the JSON line.  ``--geometry-sdf N`` (with ``--geometry-sdf-band METRES``,
default 0.05) adds ``sdf_l1`` and ``sdf_sign`` in the same way: the posed SDF against the ground-truth mesh's signed distance at N
points in a band around it (MetaAvatarRender.geometry_metrics, sdf=; DESIGN.md "Signed distance to a mesh on the device").
``--geometry-inside winding`` (default ``parity``) answers the inside tests of ``--geometry-iou`` and ``--geometry-sdf`` with
generalized winding numbers instead of crossing parities (geometry's ``rule="winding"``; DESIGN.md "Winding numbers on the device"):
for ground truth that is not watertight.  The JSON line then gains ``"geometry_inside": "winding"``.
Without the options the output is unchanged."""
import argparse
import importlib
import json
import os
import time

import torch


def build_parser():
    p = argparse.ArgumentParser(description="Validation function on with-distribution poses (ZJU training and testing).")
    p.add_argument("config", type=str, help="Path to config file.")
    p.add_argument("--novel-pose", action="store_true", help="Test on novel-poses.")
    p.add_argument("--novel-pose-view", type=str, default=None,
                   help="Novel view to use for rendering novel poses. Specify this argument if you only want to render a "
                        "specific view of novel poses.")
    p.add_argument("--novel-view", action="store_true", help="Test on novel-views of all training poses.")
    p.add_argument("--multi-gpu", action="store_true", help="Accepted for compatibility (validate.py:31): frames are sharded "
                                                            "over the ranks of torch.distributed.run whenever WORLD_SIZE > 1.")
    p.add_argument("--num-workers", type=int, default=4, help="Accepted for compatibility: items are composed on the GPU.")
    p.add_argument("--run-name", type=str, default="", help="Accepted for compatibility (the reference's Wandb run name).")
    p.add_argument("--lpips", type=str, default=None, help="MODULE:FUNCTION of an LPIPS callable (pred, gt, box mask) -> float.")
    p.add_argument("--data-range", type=float, default=2.0,
                   help="SSIM data range: 2.0 is what scikit-image 0.18.1 takes for float images, 1.0 the images' own range.")
    p.add_argument("--geometry", type=str, default=None, metavar="DIR",
                   help="Directory of ground-truth meshes <frame>.npz / <frame>.ply (named like the dataset's model files): "
                        "adds geometry scores of the posed mesh against them.")
    p.add_argument("--geometry-n-side", type=int, default=256, help="Lattice resolution of the posed mesh that is scored.")
    p.add_argument("--geometry-samples", type=int, default=100000, help="Surface samples per mesh of the geometry scores.")
    p.add_argument("--geometry-seed", type=int, default=0, help="Seed of the geometry scores' surface samples.")
    p.add_argument("--geometry-thresholds", type=str, default=None, metavar="T1,T2,...",
                   help="Distances in metres (up to 16): adds precision@T, recall@T and fscore@T to the geometry scores.")
    p.add_argument("--geometry-iou", type=int, default=None, metavar="N",
                   help="Uniform points of the volumetric IoU against ground-truth meshes: adds iou to the geometry scores.")
    p.add_argument("--geometry-sdf", type=int, default=None, metavar="N",
                   help="Points in a band around ground-truth meshes at which the posed SDF is compared with the mesh's signed "
                        "distance: adds sdf_l1 and sdf_sign to the geometry scores.")
    p.add_argument("--geometry-sdf-band", type=float, default=0.05, metavar="METRES", help="Half width of that band.")
    p.add_argument("--geometry-inside", type=str, default="parity", choices=("parity", "winding"),
                   help="The inside test of --geometry-iou and --geometry-sdf: crossing parities (watertight ground truth) or "
                        "generalized winding numbers (ground truth with holes, open sheets, flipped patches).")
    p.add_argument("--default-config", type=str, default="configs/default.yaml")
    p.add_argument("--body-models", type=str, default="body_models/misc", help="Directory of the SMPL model files.")
    return p


def apply_overrides(cfg, args):
    """validate.py:42-50."""
    if args.novel_view and not args.novel_pose:          # novel-view synthesis on training poses: every 30th frame
        cfg["data"]["val_subsampling_rate"] = 30
    if args.novel_pose_view is not None:                 # view synthesis (training or testing views) on novel poses
        assert args.novel_pose
        cfg["data"]["test_subsampling_rate"] = 1
        cfg["data"]["test_views"] = [args.novel_pose_view]
    return cfg


def load_callable(spec):
    module, _, name = spec.partition(":")
    if not module or not name:
        raise ValueError("--lpips takes MODULE:FUNCTION, not %r" % spec)
    return getattr(importlib.import_module(module), name)


def geometry_file(directory, model_file):
    """The ground-truth mesh of the frame whose SMPL parameters are `model_file`: DIR/<same name>.npz or .ply, else None."""
    stem = os.path.splitext(os.path.basename(model_file))[0]
    for ext in (".npz", ".ply"):
        path = os.path.join(directory, stem + ext)
        if os.path.exists(path):
            return path
    return None


def validate(lm, dataset, device, rank=0, world=1, lpips_fn=None, data_range=2.0, geometry=None):
    """Frames rank, rank + world, ... of the dataset through validation_step with device metrics; -> (what
    validation_epoch_end returns, frames this rank rendered, seconds it took).  Images are dropped chunk by chunk: only the
    metric scalars of a frame stay.  geometry: None, or {"dir", "n_side", "n_samples", "seed"} -- frames with a ground-truth
    mesh or scan in dir are scored by model.geometry_metrics in the same in-flight step, the scalars are read when the epoch ends
    and the result gains their means, "n_geometry" and the per-frame values; an optional "thresholds" (tuple of distances) adds
    precision@T / recall@T / fscore@T.  normal_consistency of a frame scored against a scan without normals is null; a mean runs over
    the frames that have the score.  An optional "iou" (a number of points) adds iou for the frames whose ground truth is a mesh; an
    optional "inside" ("parity" or "winding") is the inside test of iou and sdf."""
    from . import geometry as geo, renderer
    lm = lm.to(device).eval()
    mine = list(range(rank, len(dataset), world))
    geo_keys = geo.METRIC_KEYS
    thresholds = geometry.get("thresholds") if geometry is not None else None
    if thresholds:
        geo_keys = geo_keys + tuple("%s@%r" % (name, t) for name in ("precision", "recall", "fscore") for t in thresholds)
    n_iou = geometry.get("iou") if geometry is not None else None
    if n_iou:
        geo_keys = geo_keys + ("iou",)
    n_sdf = geometry.get("sdf") if geometry is not None else None
    if n_sdf:
        geo_keys = geo_keys + ("sdf_l1", "sdf_sign")
    inside = geometry.get("inside", "parity") if geometry is not None else "parity"
    mesh_only = tuple(q for q, key in enumerate(geo_keys) if key in ("iou", "sdf_l1", "sdf_sign"))   # scores a scan cannot have

    def step(item):
        gt = item.get("geometry.gt")
        if gt is None:
            return lm.validation_step(item, lpips_fn=lpips_fn, metrics="device", data_range=data_range)
        item = {k: v for k, v in item.items() if k != "geometry.gt"}
        out = lm.validation_step(item, lpips_fn=lpips_fn, metrics="device", data_range=data_range)
        scores = lm.model.geometry_metrics(lm.compose_inputs(item, eval=True), gt, n_side=geometry["n_side"],
                                           n_samples=geometry["n_samples"], seed=geometry["seed"], thresholds=thresholds or None,
                                           iou=n_iou if n_iou and not geo._is_cloud(gt) else None,
                                           **({"inside": inside} if inside != "parity" else {}),
                                           **({"sdf": n_sdf, "sdf_band": geometry.get("sdf_band", 0.05)}
                                              if n_sdf and not geo._is_cloud(gt) else {}))
        out["geometry"] = torch.stack([scores[k] for k in geo.METRIC_KEYS])
        if thresholds:
            out["geometry"] = torch.cat([out["geometry"], scores["precision"], scores["recall"], scores["fscore"]])
        if n_iou:   # a scan has no volume: its slot stays NaN and the frame gets no iou
            out["geometry"] = torch.cat([out["geometry"], scores["iou"].reshape(1) if "iou" in scores
                                         else torch.full((1,), float("nan"), dtype=torch.float64, device=out["geometry"].device)])
        if n_sdf:   # ... and no signed distance
            out["geometry"] = torch.cat([out["geometry"], torch.stack([scores["sdf_l1"], scores["sdf_sign"]]) if "sdf_l1" in scores
                                         else torch.full((2,), float("nan"), dtype=torch.float64, device=out["geometry"].device)])
        if n_iou or n_sdf:
            out["geometry_mesh"] = not geo._is_cloud(gt)
        out["geometry_scan"] = isinstance(gt, geo.PointCloud) and gt.normals is None   # a scan without normals
        return out

    kept = []
    torch.cuda.synchronize(device)
    t0 = time.time()
    for c in range(0, len(mine), 20):   # twenty frames resident at a time, renderer.frames_in_flight of them in flight
        items = [dataset.validation_item(i, device) for i in mine[c:c + 20]]
        if geometry is not None:
            for i, item in zip(mine[c:c + 20], items):
                path = geometry_file(geometry["dir"], dataset.data[i]["model_file"])
                if path is not None:
                    item["geometry.gt"] = geo.load_geometry(path, device)
        outs = renderer.map_in_flight(step, items, owner=lm.model)
        kept += [{k: v for k, v in o.items() if k in ("psnr", "ssim", "lpips", "metrics_status", "geometry", "geometry_scan", "geometry_mesh")}
                 for o in outs]
    torch.cuda.synchronize(device)
    seconds = time.time() - t0
    res = lm.validation_epoch_end([{k: v for k, v in o.items() if k not in ("geometry", "geometry_scan", "geometry_mesh")} for o in kept], first_index=rank,
                                  index_stride=world)
    if geometry is not None:
        nc = geo.METRIC_KEYS.index("normal_consistency")

        def values(o):   # a scan without normals has no normal consistency: null in the strict JSON.  Any other NaN stays NaN.
            v = o["geometry"].cpu().tolist()
            if o["geometry_scan"] and v[nc] != v[nc]:
                v[nc] = None
            if mesh_only and not o["geometry_mesh"]:
                for q in mesh_only:
                    v[q] = None
            return v
        rows = [(rank + k * world, values(o)) for k, o in enumerate(kept) if "geometry" in o]
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            gathered = [None] * dist.get_world_size()
            dist.all_gather_object(gathered, rows)
            rows = [r for part in gathered for r in part]
        if res is not None:
            scored = dict(rows)
            for frame in res["frames"]:
                if frame["frame"] in scored:
                    frame.update(zip(geo_keys, scored[frame["frame"]]))
                    for q in mesh_only:   # scored against a scan
                        if frame[geo_keys[q]] is None:
                            del frame[geo_keys[q]]
            res["n_geometry"] = len(scored)
            for q, key in enumerate(geo_keys):
                col = [v[q] for v in scored.values() if v[q] is not None]   # the frames that have the score
                res[key] = sum(col) / len(col) if col else None   # null: no frame was scored, or none has this score
    return res, len(mine), seconds


def main(argv=None, body=None, faces=None, log=print):
    from . import config, data
    args = build_parser().parse_args(argv)
    cfg = apply_overrides(config.load_config(args.config, args.default_config), args)
    out_dir = cfg["training"]["out_dir"]
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    checkpoint_path = os.path.join(out_dir, "checkpoints/last.ckpt")
    if not os.path.exists(checkpoint_path):
        raise FileNotFoundError("No checkpoint is found!")          # validate.py:88-90
    if not torch.cuda.is_available():
        raise SystemExit("validate needs a GPU (the renderer has no CPU fallback)")
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    train_dataset = data.get_capture_dataset("train", cfg, body=body, faces=faces, body_models=args.body_models)
    val_dataset = data.get_capture_dataset("test" if args.novel_pose else "val", cfg, body=train_dataset.body,
                                           faces=train_dataset.faces, body_models=args.body_models)
    # mode "val": sized from the training dataset like the reference's construction, without reading the MetaAvatar
    # initialisation files the checkpoint is about to replace
    lm = config.get_model(cfg, dataset=train_dataset, val_size=len(val_dataset), mode="val", checkpoint_path=checkpoint_path,
                          body_model=train_dataset.body)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)
    lpips_fn = load_callable(args.lpips) if args.lpips else None
    geometry = None
    if args.geometry is not None:
        if not os.path.isdir(args.geometry):
            raise FileNotFoundError("--geometry: %s is not a directory" % args.geometry)
        geometry = {"dir": args.geometry, "n_side": args.geometry_n_side, "n_samples": args.geometry_samples,
                    "seed": args.geometry_seed}
        if args.geometry_thresholds is not None:
            from . import geometry as geo
            geometry["thresholds"] = geo.check_thresholds([float(t) for t in args.geometry_thresholds.split(",")])
        if args.geometry_iou is not None:
            if args.geometry_iou < 1:
                raise ValueError("--geometry-iou takes a positive number of points")
            geometry["iou"] = args.geometry_iou
        if args.geometry_sdf is not None:
            if args.geometry_sdf < 1 or not 0 < args.geometry_sdf_band < float("inf"):
                raise ValueError("--geometry-sdf takes a positive number of points and --geometry-sdf-band a finite length > 0")
            geometry["sdf"], geometry["sdf_band"] = args.geometry_sdf, args.geometry_sdf_band
        if args.geometry_inside != "parity":
            geometry["inside"] = args.geometry_inside
    elif args.geometry_thresholds is not None:
        raise ValueError("--geometry-thresholds needs --geometry DIR")
    elif args.geometry_iou is not None:
        raise ValueError("--geometry-iou needs --geometry DIR")
    elif args.geometry_sdf is not None:
        raise ValueError("--geometry-sdf needs --geometry DIR")
    elif args.geometry_inside != "parity":
        raise ValueError("--geometry-inside needs --geometry DIR")
    res, n_mine, seconds = validate(lm, val_dataset, device, rank, world, lpips_fn, args.data_range, geometry)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if res is None:
        return None
    frames = res.pop("frames")
    res.update(seconds_per_frame=seconds / max(1, n_mine), world=world, data_range=args.data_range,
               mode="test" if args.novel_pose else "val")
    if geometry is not None and geometry.get("inside", "parity") != "parity":
        res["geometry_inside"] = geometry["inside"]
    with open(os.path.join(out_dir, "validation.json"), "w") as f:
        json.dump(dict(res, frames=frames), f, indent=1)
    log(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
