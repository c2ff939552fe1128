"""The frame driver (csrc/frame.hip run_frame) on a real MI355X, through the public API only: every branch the driver takes depends
on the cascade and the source mode, not on the image size, so the frames are 64x96 (the smallest multiple-of-32 frame), S = 3,
volume planes (8, 8).  The frame with the side lane must equal the one-stream frame bit for bit, twice in a row; a gated last
FeatureNet stage (side_gate 2 / 3 / 4) must not change it either; and a graph replay must equal the eager frame.  What a missing
join looks like when these pass by luck is tests/test_frame_driver.py's business (the emulator's trace)."""
import pytest
import torch

import __graft_entry__ as G
from enerf_amd.config import CascadeConfig, EnerfConfig
from enerf_amd.synth import make_batch

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU (run with -m gpu on the MI355X box)")]
H, W, S = 64, 96, 3
CFG_DEFAULT = EnerfConfig().with_cas(volume_planes=(8, 8), render_if=(False, True))
CFG_BOTH = EnerfConfig().with_cas(volume_planes=(8, 8), render_if=(True, True))
# configs/enerf/dtu_pretrain_nocascade.yaml:27-38
CFG_ONE = EnerfConfig(cas=CascadeConfig(num=1, depth_inv=(True,), volume_scale=(0.25,), volume_planes=(8,), im_feat_scale=(0.25,),
                                        im_ibr_scale=(1.0,), render_scale=(1.0,), render_im_feat_level=(2,),
                                        nerf_model_feat_ch=(8,), render_if=(True,), num_samples=(2,)))
#        cascade, human, feature backend, through a source cache
CASES = {"default": (CFG_DEFAULT, False, "hip", False),
         "both": (CFG_BOTH, False, "hip", False),
         "one": (CFG_ONE, False, "hip", False),
         "human_mask": (CFG_DEFAULT, True, "hip", False),
         "nchw": (CFG_DEFAULT, False, "torch", False),
         "cached": (CFG_DEFAULT, False, "hip", True)}


def _frame(case):
    """-> (net, run(options) -> outputs, fn, batch): ``fn(batch)`` is the frame with the network's current options."""
    cfg, human, backend, cached = CASES[case]
    dev = torch.device("cuda:0")
    net = G._seeded_network(cfg, dev, human=human, feature_backend=backend)        # enerf_amd/libenerf_hip.so
    batch = {k: torch.from_numpy(v).to(dev) for k, v in make_batch(H, W, S, cfg, seed=3, textured=True, mask_box=human).items()}
    if cached:
        cache = net.cache_sources(batch["src_inps"][0].contiguous(), batch["src_exts"][0].contiguous(), batch["src_ixts"][0].contiguous())
        idx = torch.arange(S, dtype=torch.int32, device=dev)
        batch = {k: v for k, v in batch.items() if not k.startswith("src_")}
        fn = lambda b: net.forward_cached(cache, idx, b)
    else:
        fn = net

    def run(options=None):
        net.options = options
        with torch.no_grad():
            out = {k: v.clone() for k, v in fn(batch).items()}
        torch.cuda.synchronize()
        return out
    return net, run, fn, batch


def _same(out, ref):
    assert sorted(out) == sorted(ref)
    for k in ref:
        assert out[k].shape == ref[k].shape, k
        assert torch.equal(out[k], ref[k]), k


@pytest.mark.parametrize("case", list(CASES))
def test_lane_frame_equals_one_stream_frame(case):
    from enerf_amd.lib import Options
    net, run, fn, batch = _frame(case)
    ref = run(None)
    rgb = ref[max(k for k in ref if k.startswith("rgb"))]
    assert bool(torch.isfinite(rgb).all()) and float(rgb.abs().max()) > 0
    _same(run(None), ref)                                  # the same twice in a row
    _same(run(Options(single_stream=1)), ref)
    _same(run(None), ref)
    if CASES[case][0] is CFG_DEFAULT:
        for gate in (2, 3, 4):
            _same(run(Options(side_gate=gate)), ref)
        _same(run(None), ref)
    if case in ("both", "cached"):
        from enerf_amd.graph import GraphedFrame
        net.options = None
        frame = GraphedFrame(net, batch, fn=None if fn is net else fn)
        for _ in range(2):
            out = frame(batch)
            torch.cuda.synchronize()
            _same(out, ref)
