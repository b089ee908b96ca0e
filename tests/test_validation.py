"""Validation against ground truth: the validation item of the capture datasets (reference im2mesh/data/zju_mocap.py:399-433,
603-607), LightningModel.validation_step with device metrics / validation_epoch_end (lightning_model.py:160-298) and the
entry point arah_release_amd/validate.py (reference validate.py).  The float64 restatement of the two metrics and its bounds
are tests/test_image_metrics.py's."""
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import golden
from test_image_metrics import PSNR_HOST_TOL, PSNR_TOL, SSIM_TOL, psnr_restatement, ssim_restatement

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def body(scene):
    from arah_release_amd import smpl
    return smpl.BodyModel.synthetic(scene)


def _fixture_frame():
    g = golden("f9_callers.npz")
    return ({k[3:]: g[k] for k in g.files if k.startswith("md.")}, {k[4:]: g[k] for k in g.files if k.startswith("cam.")})


def _rim_mask(H, W, seed):
    """1 on a 'body', 100 on a rim around it, 0 elsewhere -- the three values ZJUMOCAPDataset.get_mask produces."""
    yy, xx = np.mgrid[0:H, 0:W]
    r = np.hypot(yy - 0.5 * H, xx - 0.5 * W) + np.random.RandomState(seed).rand(H, W) * 3
    return np.where(r < 0.22 * H, 1, np.where(r < 0.3 * H, 100, 0)).astype(np.int64)


# ------------------------------------------------------------------------------------------------------------ CPU
def test_validation_item_against_the_reference_branch(body):
    """data.validation_item against zju_mocap.py:409-433 restated in numpy: the pixels of the projected box whose ray hits the
    body box, row-major, black where mask_erode == 0, the rim (100) keeping its colour; no 'inputs.novel_seq'; every other key
    as frame_item gives it."""
    from arah_release_amd import data
    md, cam = _fixture_frame()
    H = W = 64
    image = np.random.RandomState(1).rand(H, W, 3).astype(np.float32)
    mask_erode = _rim_mask(H, W, 2)
    ids = dict(cam_idx=2, frame_idx=5, data_idx=1, gender="neutral")
    base = data.frame_item(md, cam, body, (H, W), 64, device="cpu", **ids)
    item = data.validation_item(md, cam, body, image, mask_erode, (H, W), 64, box_margin=0.05, device="cpu", **ids)
    # the reference's branch: y_inds, x_inds = np.where(bound_mask); pixels there, background blacked, then [mask_at_box].
    # image_mask marks exactly the kept pixels, and np.where walks it in the same row-major order
    image_mask = base["inputs.image_mask"][0].numpy()
    y_inds, x_inds = np.where(image_mask)
    sampled = image[y_inds, x_inds, :].copy()
    sampled[(mask_erode == 0)[y_inds, x_inds]] = 0
    got = item["inputs"][0].numpy()
    assert got.shape == (int(image_mask.sum()), 3) and got.shape[0] == base["inputs.ray_dirs"].shape[1] > 100
    np.testing.assert_array_equal(got, sampled)
    kept = (mask_erode == 100)[y_inds, x_inds]
    assert kept.any() and (mask_erode == 0)[y_inds, x_inds].any()
    np.testing.assert_array_equal(got[kept], image[y_inds, x_inds][kept])                 # rim pixels keep their colour
    assert "inputs.novel_seq" not in item and "inputs.novel_seq" in base
    assert set(item) == set(base) - {"inputs.novel_seq"}
    for k in item:
        if k == "inputs":
            continue
        if isinstance(item[k], torch.Tensor):
            assert torch.equal(item[k], base[k]), k
        else:
            assert item[k] == base[k], k
    with pytest.raises(ValueError):
        data.validation_item(md, cam, body, image[:32], mask_erode, (H, W), 64, device="cpu", **ids)


def _write_capture(root, scene, n_frames=2, size=256, focal=300.0, images=None, full_masks=False, seed=0):
    """<root>/CoreView_000 in the reference's ZJU layout (cam_params.json, models/*.npz, <camera>/*.jpg + *.png)."""
    from PIL import Image
    sub = root / "CoreView_000"
    (sub / "models").mkdir(parents=True, exist_ok=True)
    (sub / "1").mkdir(exist_ok=True)
    H = W = size
    K = [[focal, 0, size / 2], [0, focal, size / 2], [0, 0, 1]]
    (sub / "cam_params.json").write_text(json.dumps({"all_cam_names": ["1"], "1": {"K": K, "D": [0.0] * 5, "R": np.eye(3).tolist(),
                                                                                  "T": [[0], [0], [0.2]]}}))
    rng = np.random.RandomState(seed)
    for f in range(n_frames):
        fr = scene.frame(f)
        np.savez(sub / "models" / ("%06d.npz" % f), minimal_shape=scene.verts_cano, betas=np.zeros((1, 10), np.float32),
                 Jtr_posed=fr["joints_posed"], bone_transforms=fr["bone_transforms"], trans=np.array([0.0, 0.0, 3.0], np.float32),
                 root_orient=np.zeros(3, np.float32), pose_body=np.zeros(63, np.float32), pose_hand=np.zeros(6, np.float32))
        if full_masks:
            sil = np.full((H, W), 255, np.uint8)
        else:
            v = fr["smpl_verts"] + np.array([0, 0, 0.2], np.float32)
            px = np.round(v[:, :2] / v[:, 2:3] * focal + size / 2).astype(int)
            sil = np.zeros((H, W), np.uint8)
            ok = (px[:, 0] >= 3) & (px[:, 0] < W - 3) & (px[:, 1] >= 3) & (px[:, 1] < H - 3)
            for dx in range(-3, 4):
                for dy in range(-3, 4):
                    sil[px[ok, 1] + dy, px[ok, 0] + dx] = 255
        img = images[f] if images is not None else rng.randint(0, 255, (H, W, 3)).astype(np.uint8)
        Image.fromarray(img).save(sub / "1" / ("%06d.jpg" % f), quality=95)
        Image.fromarray(sil).save(sub / "1" / ("%06d.png" % f))


def _capture_cfg(tmp_path, n_fg=256, n_bg=128):
    from arah_release_amd import config
    cfg = config.builtin_config("zju313")
    cfg["training"].update(out_dir=str(tmp_path / "out"), batch_size=1)
    d = {"dataset": "zju_mocap", "path": str(tmp_path / "data"), "high_res": False, "num_fg_samples": n_fg, "num_bg_samples": n_bg,
         "off_surface_thr": 0.2, "inside_thr": 0.001, "box_margin": 0.05, "sampling": "default", "sample_reg_surface": True,
         "erode_mask": True}
    for mode in ("train", "val", "test"):
        d.update({mode + "_split": ["CoreView_000"], mode + "_views": [], mode + "_subsampling_rate": 1, mode + "_start_frame": 0,
                  mode + "_end_frame": 0})
    cfg["data"] = d
    return cfg


def _fake_samples(v, f, w, cmin, cmax, cen, reg, inside, *a, **k):
    gen = torch.Generator(device=v.device).manual_seed(0)
    out = {"points_uniform": torch.rand(1024, 3, device=v.device, generator=gen) * 2 - 1,
           "points_skinning": v[:1024].clone(), "sampled_weights": w[:1024].clone()}
    if inside:
        out["points_inside"] = (torch.rand(1024, 3, device=v.device, generator=gen) - 0.5) * 0.2
    return out


def test_capture_dataset_factory_and_items_of_mode_val(tmp_path, scene, body, monkeypatch):
    """get_capture_dataset per mode (im2mesh/config.py:141-250), TrainingDataset.validation_item from files, and the behaviour
    that must not move: item() of a dataset in mode 'val' is still a TRAINING item (sampled rays, no image mask)."""
    from PIL import Image
    from arah_release_amd import data, imageops
    _write_capture(tmp_path / "data", scene, n_frames=3)
    monkeypatch.setattr(data, "training_samples", _fake_samples)
    cfg = _capture_cfg(tmp_path)
    cfg["data"].update(val_subsampling_rate=2, high_res=True)
    faces = np.zeros((1, 3), np.int32)
    train_ds = data.get_capture_dataset("train", cfg, body=body, faces=faces)
    val_ds = data.get_capture_dataset("val", cfg, body=body, faces=faces)
    assert (train_ds.mode, train_ds.img_size, len(train_ds)) == ("train", (1024, 1024), 3)          # high_res: training only
    assert (val_ds.mode, val_ds.img_size, len(val_ds)) == ("val", (512, 512), 2)
    assert [d["frame_idx"] for d in val_ds.data] == [0, 2]
    assert train_ds.num_fg_samples == 256 and train_ds.sample_reg_surface is True and train_ds.box_margin == 0.05
    cfg_h = _capture_cfg(tmp_path)
    cfg_h["data"]["dataset"] = "zju_mocap_odp"
    with pytest.raises(ValueError):
        data.get_capture_dataset("val", cfg_h, body=body, faces=faces)
    with pytest.raises(ValueError):
        data.get_capture_dataset("eval", cfg, body=body, faces=faces)
    # item() in mode 'val': today's training item
    it = val_ds.item(1, "cpu", generator=torch.Generator().manual_seed(0))
    assert it["inputs"].shape == (1, 256 + 128, 3) and "inputs.image_mask" not in it and "image.points_uniform" in it
    assert "inputs.novel_seq" not in it
    # validation_item(): the whole box, colours of the prepared image
    vi = val_ds.validation_item(1, "cpu")
    d = val_ds.data[1]
    raw = torch.as_tensor(np.array(Image.open(d["img_file"]).convert("RGB"))).float()
    msk = torch.as_tensor(np.array(Image.open(d["mask_file"]).convert("L")))
    cam = val_ds.cameras["1"]
    image, _, rim, orig = val_ds._prepare(raw, msk, val_ds._rim(msk), torch.as_tensor(np.asarray(cam["K"], np.float32)),
                                          np.zeros(5))
    assert orig == (256, 256) and tuple(image.shape) == (512, 512, 3)
    image_mask = vi["inputs.image_mask"][0].numpy()
    y_inds, x_inds = np.where(image_mask)
    want = image.numpy()[y_inds, x_inds].copy()
    want[(rim.numpy() == 0)[y_inds, x_inds]] = 0
    np.testing.assert_array_equal(vi["inputs"][0].numpy(), want)
    assert (rim.numpy() == 100).any() and int(vi["inputs.frame_idx"][0]) == 2 and int(vi["inputs.data_idx"][0]) == 1
    assert vi["inputs"].shape[1] == vi["inputs.ray_dirs"].shape[1] == int(image_mask.sum()) and "inputs.novel_seq" not in vi
    assert imageops is not None


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _frame_output(i, status=0):
    psnr = float("inf") if i == 3 else 20.0 + i
    out = {"psnr": torch.tensor(psnr, dtype=torch.float64) if i % 2 else psnr, "ssim": torch.tensor(0.5 + 0.1 * i, dtype=torch.float64),
           "lpips": 0.01 * i, "rgb_pred": torch.zeros(3, 4, 4)}
    if i != 4:
        out["metrics_status"] = torch.tensor(status, dtype=torch.int32)
    return out


def _epoch_end_worker(rank, world, port, out):
    from arah_release_amd import config
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    lm = object.__new__(config.LightningModel)                     # the aggregation uses no state of the module
    mine = list(range(rank, 5, world))                             # frame i -> rank i mod N: 3 + 2 frames
    res = lm.validation_epoch_end([_frame_output(i) for i in mine], first_index=rank, index_stride=world)
    try:
        lm.validation_epoch_end([_frame_output(i, status=2 if i == 3 else 0) for i in mine], first_index=rank, index_stride=world)
        err = None
    except ValueError as e:
        err = str(e)
    out[rank] = (res, err)
    dist.barrier()
    dist.destroy_process_group()


def test_validation_epoch_end_two_ranks_gloo():
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_epoch_end_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    (res, err0), (res1, err1) = out[0], out[1]
    assert res1 is None                                             # the means live on rank 0
    assert res["n"] == 5 and [r["frame"] for r in res["frames"]] == [0, 1, 2, 3, 4]          # every frame once, in frame order
    assert res["n_psnr_inf"] == 1 and res["psnr"] == pytest.approx((20 + 21 + 22 + 24) / 4.0, abs=1e-12)   # inf reported, not averaged
    assert res["ssim"] == pytest.approx(0.7, abs=1e-12) and res["lpips"] == pytest.approx(0.02, abs=1e-12)
    assert res["frames"][3]["psnr"] == float("inf") and res["frames"][2]["ssim"] == pytest.approx(0.7)
    for err in (err0, err1):                                        # a status != 0 names the frame, on every rank
        assert err is not None and "frame 3" in err and "SSIM" in err
    # a single process without a process group
    from arah_release_amd import config
    lm = object.__new__(config.LightningModel)
    one = lm.validation_epoch_end([_frame_output(i) for i in range(3)])
    assert one["n"] == 3 and one["n_psnr_inf"] == 0 and one["psnr"] == pytest.approx(21.0) and one["ssim"] == pytest.approx(0.6)


def test_validate_overrides_and_missing_checkpoint(tmp_path):
    """validate.py:42-50 and :88-90."""
    import yaml
    from arah_release_amd import validate
    base = lambda: {"data": {"val_subsampling_rate": 1, "test_subsampling_rate": 7, "test_views": ["1", "2"]}}
    parse = validate.build_parser().parse_args
    assert validate.apply_overrides(base(), parse(["c.yaml"])) == base()
    assert validate.apply_overrides(base(), parse(["c.yaml", "--novel-view"]))["data"]["val_subsampling_rate"] == 30
    assert validate.apply_overrides(base(), parse(["c.yaml", "--novel-view", "--novel-pose"])) == base()
    got = validate.apply_overrides(base(), parse(["c.yaml", "--novel-pose", "--novel-pose-view", "5"]))["data"]
    assert got == {"val_subsampling_rate": 1, "test_subsampling_rate": 1, "test_views": ["5"]}
    with pytest.raises(AssertionError):
        validate.apply_overrides(base(), parse(["c.yaml", "--novel-pose-view", "5"]))
    args = parse(["c.yaml", "--multi-gpu", "--num-workers", "2", "--run-name", "x"])          # accepted for compatibility
    assert args.multi_gpu and args.num_workers == 2 and args.run_name == "x" and args.lpips is None and args.data_range == 2.0
    assert validate.load_callable("math:sqrt")(4.0) == 2.0
    with pytest.raises(ValueError):
        validate.load_callable("math")
    cfg = _capture_cfg(tmp_path)
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(cfg))
    with pytest.raises(FileNotFoundError, match="No checkpoint is found!"):
        validate.main([str(tmp_path / "cfg.yaml"), "--default-config", str(tmp_path / "cfg.yaml")])


# ------------------------------------------------------------------------------------------------------------ GPU
def _gpu_model(dev, n_data_points=4):
    from arah_release_amd import config
    cfg = config.builtin_config("zju313")
    lm = config.get_model(cfg, mode="test", n_data_points=n_data_points)
    lm.model.load_state_dict(config.synthetic_state_dict(cfg), strict=False)
    lm = lm.to(dev).eval()
    lm.model.frames = []
    return lm


def _images(res):
    return (res["rgb_pred"].permute(1, 2, 0).cpu().numpy(), res["rgb_gt"].permute(1, 2, 0).cpu().numpy())


@gpu
def test_validation_step_with_device_metrics(body):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from arah_release_amd import data, renderer
    dev = torch.device("cuda:0")
    md, cam = _fixture_frame()
    H = W = 256
    lm = _gpu_model(dev)

    def item_of(seed):
        image = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(seed))
        return data.validation_item(md, cam, body, image, _rim_mask(H, W, seed), H, 64, device=dev, frame_idx=5, data_idx=1)

    item = item_of(0)
    res = lm.validation_step(item, metrics="device")
    assert set(res) == {"psnr", "ssim", "metrics_status", "rgb_pred", "normal_pred", "rgb_gt"}
    for k in ("psnr", "ssim"):
        assert res[k].is_cuda and res[k].dim() == 0 and res[k].dtype == torch.float64, k
    assert res["metrics_status"].is_cuda and int(res["metrics_status"]) == 0
    pred, gt = _images(res)
    box = item["inputs.image_mask"][0].cpu().numpy()
    want_ssim, want_psnr = ssim_restatement(pred, gt, box), psnr_restatement(pred, gt, box)
    print("device ssim %.15f (restatement %.15f)  psnr %.10f dB (restatement %.10f)" % (float(res["ssim"]), want_ssim,
                                                                                       float(res["psnr"]), want_psnr))
    assert abs(float(res["ssim"]) - want_ssim) <= SSIM_TOL and abs(float(res["psnr"]) - want_psnr) <= PSNR_TOL
    assert 0.0 < float(res["ssim"]) < 1.0 and np.isfinite(float(res["psnr"]))
    # today's route with the restatement as ssim_fn: same frame, same numbers (its PSNR is float32 on the host)
    host = lm.validation_step(item, ssim_fn=ssim_restatement)
    assert set(host) == {"psnr", "ssim", "rgb_pred", "normal_pred", "rgb_gt"}
    assert abs(float(res["ssim"]) - host["ssim"]) <= SSIM_TOL and abs(float(res["psnr"]) - float(host["psnr"])) <= PSNR_HOST_TOL
    assert torch.equal(host["rgb_pred"], res["rgb_pred"]) and torch.equal(host["rgb_gt"], res["rgb_gt"])
    assert torch.equal(host["normal_pred"], res["normal_pred"])
    with pytest.raises(ValueError):
        lm.validation_step(item, ssim_fn=ssim_restatement, metrics="device")
    with pytest.raises(ValueError):
        lm.validation_step(item, metrics="host")
    # data_range reaches the kernel
    r1 = lm.validation_step(item, metrics="device", data_range=1.0)
    assert abs(float(r1["ssim"]) - ssim_restatement(pred, gt, box, 1.0)) <= SSIM_TOL and float(r1["ssim"]) != float(res["ssim"])
    # ground truth = prediction
    same = dict(item)
    same["inputs"] = res["rgb_pred"].permute(1, 2, 0)[item["inputs.image_mask"][0]].unsqueeze(0).clone()
    rs = lm.validation_step(same, metrics="device")
    assert abs(float(rs["ssim"]) - 1.0) <= 1e-15 and float(rs["psnr"]) == float("inf") and int(rs["metrics_status"]) == 0
    # eight frames in flight = the same frames one at a time, bit for bit
    items = [item_of(10 + k) for k in range(8)]
    step = lambda it: lm.validation_step(it, metrics="device")
    single = [step(it) for it in items]
    torch.cuda.synchronize()
    flight = renderer.map_in_flight(step, items, owner=lm.model)
    torch.cuda.synchronize()
    for a, b in zip(single, flight):
        for k in ("psnr", "ssim"):
            assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k
        assert torch.equal(a["rgb_pred"], b["rgb_pred"]) and int(b["metrics_status"]) == 0
    assert len({float(a["ssim"]) for a in single}) == 8
    agg = lm.validation_epoch_end(flight)
    assert agg["n"] == 8 and agg["ssim"] == pytest.approx(np.mean([float(a["ssim"]) for a in single]), abs=1e-15)


@gpu
def test_validate_entry_end_to_end(tmp_path, scene, body, monkeypatch):
    """python -m arah_release_amd.validate on a capture in the reference's layout whose images ARE the model's renders
    (through JPEG): the JSON line's means are the restatement's means over the frames; against black images both metrics are
    strictly worse.  JPEG is lossy, so no absolute PSNR is asserted."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import yaml
    from arah_release_amd import config, data, train, validate
    dev = torch.device("cuda:0")
    monkeypatch.setattr(data, "training_samples", _fake_samples)
    n_frames, size = 3, 512
    faces = np.zeros((1, 3), np.int32)
    black = [np.zeros((size, size, 3), np.uint8)] * n_frames
    _write_capture(tmp_path / "data", scene, n_frames=n_frames, size=size, focal=600.0, images=black, full_masks=True)
    cfg = _capture_cfg(tmp_path)
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(cfg))
    argv = [str(tmp_path / "cfg.yaml"), "--default-config", str(tmp_path / "cfg.yaml")]
    train_ds = data.get_capture_dataset("train", cfg, body=body, faces=faces)
    val_ds = data.get_capture_dataset("val", cfg, body=body, faces=faces)
    lm = config.get_model(cfg, dataset=train_ds, mode="val", body_model=body)
    own = lm.model.state_dict()     # (the latent codes are sized by the capture's frames, not by the synthetic subject's)
    lm.model.load_state_dict({k: v for k, v in config.synthetic_state_dict(cfg).items()
                              if k not in own or own[k].shape == v.shape}, strict=False)
    train.save_checkpoint(str(tmp_path / "out" / "checkpoints" / "last.ckpt"), lm, lm.configure_optimizers(), epoch=1, global_step=n_frames)
    lm = lm.to(dev).eval()

    def restated_means():
        ssim, psnr = [], []
        for i in range(len(val_ds)):
            item = val_ds.validation_item(i, dev)
            res = lm.validation_step(item)
            pred, gt = _images(res)
            box = item["inputs.image_mask"][0].cpu().numpy()
            ssim.append(ssim_restatement(pred, gt, box))
            psnr.append(psnr_restatement(pred, gt, box))
        return float(np.mean(ssim)), float(np.mean(psnr)), pred

    lines = []
    res_black = validate.main(argv, body=body, faces=faces, log=lines.append)
    want_ssim, want_psnr, _ = restated_means()
    assert json.loads(lines[-1])["n"] == n_frames
    assert abs(res_black["ssim"] - want_ssim) <= SSIM_TOL and abs(res_black["psnr"] - want_psnr) <= PSNR_TOL
    # the renders become the capture's images
    renders = []
    for i in range(len(val_ds)):
        img = lm.validation_step(val_ds.validation_item(i, dev))["rgb_pred"].permute(1, 2, 0)
        renders.append((img.clamp(0, 1) * 255.0).round().to(torch.uint8).cpu().numpy())
    assert renders[0].max() > 50
    _write_capture(tmp_path / "data", scene, n_frames=n_frames, size=size, focal=600.0, images=renders, full_masks=True)
    res = validate.main(argv, body=body, faces=faces, log=lines.append)
    line = json.loads(lines[-1])
    want_ssim, want_psnr, _ = restated_means()
    print("validate: black %s\n          renders %s\n          restated ssim %.15f psnr %.10f" % (lines[-2], lines[-1], want_ssim, want_psnr))
    assert line["n"] == n_frames and line["n_psnr_inf"] == 0 and line["seconds_per_frame"] > 0
    assert abs(line["ssim"] - want_ssim) <= SSIM_TOL and abs(line["psnr"] - want_psnr) <= PSNR_TOL
    assert line["ssim"] <= 1.0
    assert line["ssim"] > res_black["ssim"] and line["psnr"] > res_black["psnr"]
    saved = json.load(open(tmp_path / "out" / "validation.json"))
    assert [f["frame"] for f in saved["frames"]] == list(range(n_frames)) and saved["ssim"] == res["ssim"]
    assert all(f["status"] == 0 for f in saved["frames"]) and "lpips" not in line
    assert np.mean([f["ssim"] for f in saved["frames"]]) == pytest.approx(line["ssim"], abs=1e-15)
