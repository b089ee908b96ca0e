"""render_sequence with render_maps=True (several frames in flight, each on its own stream and scratch, the per-sample normal
slab included).  In a file of its own that runs late, like tests/test_zz_render_sequence.py: a stalled multi-stream launch
ends the whole pytest process."""
import pytest
import torch

gpu = pytest.mark.gpu


@gpu
@pytest.mark.timeout(150)
def test_render_sequence_with_maps_matches_frame_by_frame(scene):
    """Four frames in flight: every frame's maps (and rgb) equal a forward of that frame alone, bit for bit -- the frames in
    flight keep their maps apart."""
    from arah_release_amd import config, renderer
    dev = torch.device("cuda:0")
    model, _ = config.build_synthetic_model("zju377_mono", device=dev)
    frames = [scene.make_inputs(s, s, frame_idx=f, device=dev) for f, s in ((0, 256), (3, 192), (7, 256), (11, 128), (5, 256), (9, 192))]
    with torch.no_grad():
        ref = [model.forward_maps(dict(f)) for f in frames]
    got = renderer.render_sequence(model, [dict(f) for f in frames], n_streams=4, eval=True, render_maps=True)
    assert len(got) == len(ref)
    for a, b in zip(ref, got):
        for k in ("normal_values", "depth_values", "acc_values", "rgb_values", "network_body_mask", "points_cam"):
            assert torch.equal(a[k], b[k]), k
    assert not torch.equal(got[0]["normal_values"], got[2]["normal_values"])   # different frames, different maps
