"""Source-view cache on a real MI355X, through the C ABI: ``forward_cached`` against ``Network.forward`` on the same views
gathered by hand — bit for bit, on every output of every rendered level — at the three real shapes the parity suite runs, with
V = 8 synthetic source views (enerf_amd.synth); the interactive loop select_views -> forward_cached -> pack_rgb8 captured in a HIP
graph; and no implicit host synchronisation anywhere in it.  (An out-of-range index is exercised on the CPU emulator only.)"""
import numpy as np
import pytest
import torch

from enerf_amd.config import EnerfConfig
from enerf_amd.synth import look_at_w2c, make_batch, make_lego_batch, make_zju_batch
from golden_cases import load_weights

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU (run with -m gpu on the MI355X box)")]
V = 8


def _dev():
    return torch.device("cuda:0")


def _net(cfg, human=False, **kw):
    from enerf_amd.network import Network, NetworkHuman
    net = (NetworkHuman if human else Network)(cfg, **kw)              # enerf_amd/libenerf_hip.so
    net.load_state_dict(load_weights(), strict=False)
    return net.to(_dev()).eval()


def _split(batches):
    """Batches of one synthetic rig (numpy, B = 1) -> (V views on the device, target part of the first batch)."""
    cat = lambda k: torch.from_numpy(np.concatenate([b[k][0] for b in batches])).to(_dev()).contiguous()
    views = (cat("src_inps"), cat("src_exts"), cat("src_ixts"))
    assert views[0].shape[0] == V
    tar = {k: torch.from_numpy(v).to(_dev()) for k, v in batches[0].items() if not k.startswith("src_")}
    return views, tar


def _by_hand(views, tar, idx):
    rows = torch.as_tensor(idx, dtype=torch.long, device=_dev())
    rows = rows[None] if rows.dim() == 1 else rows
    return dict(tar, src_inps=views[0][rows].contiguous(), src_exts=views[1][rows].contiguous(), src_ixts=views[2][rows].contiguous())


def _same(out, ref):
    assert sorted(out) == sorted(ref)
    for k in ref:
        assert out[k].shape == ref[k].shape, k
        assert torch.equal(out[k], ref[k]), k


def _check(net, views, tar, index_rows):
    from enerf_amd.lib import Options
    cache = net.cache_sources(*views)
    for idx in index_rows:
        ref = {k: v.clone() for k, v in net(_by_hand(views, tar, idx)).items()}
        out = net.forward_cached(cache, torch.tensor(idx, dtype=torch.int32, device=_dev()), tar)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out[max(k for k in out if k.startswith("rgb"))]).all())
        _same(out, ref)
        # the side lane only changes WHEN the level-2 / texel share is gathered
        one = net._forward(tar, Options(single_stream=1), cache, torch.tensor(idx, dtype=torch.int32, device=_dev()))
        torch.cuda.synchronize()
        _same(one, ref)
    return cache


def test_dtu_eval_512x640_3_of_8_views():
    cfg = EnerfConfig.dtu_eval()
    views, tar = _split([make_batch(512, 640, V, cfg, seed=0, textured=True)])
    cache = _check(_net(cfg), views, tar, ([0, 1, 2], [6, 3, 5], [7, 7, 1]))
    assert cache.l2_stride == 12 and cache.nbytes() == 4 * V * (128 * 160 * 32 + 256 * 320 * 16 + 512 * 640 * 12 + 25)


def test_lego_800x800_4_of_8_views_both_levels():
    cfg = EnerfConfig()
    views, tar = _split([make_lego_batch(800, 800, 4, cfg, seed=5), make_lego_batch(800, 800, 4, cfg, seed=6)])
    cache = _check(_net(cfg), views, tar, ([0, 1, 2, 3], [5, 2, 7, 0]))
    assert cache.struct.tex[0] and not cache.struct.tex[1]


def test_zju_1024_4_of_8_views_masked():
    cfg = EnerfConfig().with_cas(volume_planes=(32, 8), render_if=(False, True))
    views, tar = _split([make_zju_batch(1024, 1024, 4, cfg, seed=6), make_zju_batch(1024, 1024, 4, cfg, seed=7)])
    net = _net(cfg, human=True)
    _check(net, views, tar, ([0, 1, 2, 3], [4, 1, 6, 3]))
    m = int(tar["mask_at_box"].bool().sum())
    out = net.forward_cached(net.cache_sources(*views), torch.tensor([4, 1, 6, 3], dtype=torch.int32, device=_dev()), tar)
    assert out["depth_level1"].shape == (1, m)                          # compacted, like the reference


@pytest.mark.parametrize("views", [5, 6, 21])
def test_view_counts_that_leave_a_remainder_chunk(views):
    """V not divisible by 4 (21: the interactive rig, a last chunk of ONE image): the cache equals ONE enerf_feature_net call over
    all V images on the hardware too, and frames drawn from the remainder chunk equal today's frame."""
    cfg = EnerfConfig.dtu_eval()
    b = make_batch(128, 160, views, cfg, seed=4, textured=True)
    inps, exts, ixts = (torch.from_numpy(b[k][0]).to(_dev()).contiguous() for k in ("src_inps", "src_exts", "src_ixts"))
    tar = {k: torch.from_numpy(v).to(_dev()) for k, v in b.items() if not k.startswith("src_")}
    net = _net(cfg)
    cache = net.cache_sources(inps, exts, ixts)
    f0, f1, f2, _ = net.lib.feature_net(net._packed_weights("feature_net"), inps, l2_stride=cache.l2_stride)
    torch.cuda.synchronize()
    for got, ref in zip(cache.feats, (f0, f1, f2)):
        assert torch.equal(got, ref)
    for idx in ([views - 1, 0, views - 2], [views - 1, views - 1, 4]):
        ref = {k: v.clone() for k, v in net(_by_hand((inps, exts, ixts), tar, idx)).items()}
        out = net.forward_cached(cache, torch.tensor(idx, dtype=torch.int32, device=_dev()), tar)
        torch.cuda.synchronize()
        _same(out, ref)


def _interactive_scene(cfg, h, w, human=False):
    b = make_batch(h, w, V, cfg, seed=2, textured=True, mask_box=human)
    views, tar = _split([b])
    cam_points = torch.linalg.inv(views[1].double().cpu())[:, :3, 3].float().to(_dev()).contiguous()     # camera centres
    cams = []
    for c in ([0.0, 0.0, 0.0], [-120.0, -30.0, 10.0], [150.0, 90.0, -20.0]):
        ext = look_at_w2c(np.array(c))
        cams.append((torch.from_numpy(ext.astype(np.float32))[None].to(_dev()),
                     torch.from_numpy(np.linalg.inv(ext).astype(np.float32)).to(_dev()).contiguous()))
    tar = {k: v for k, v in tar.items() if not k.startswith("rays_")}   # full-image rays are generated on the device
    return views, tar, cam_points, cams


def test_interactive_loop_under_a_hip_graph_matches_eager():
    """select_views + forward_cached + pack_rgb8 captured once; replayed with three target cameras == eager, bit for bit."""
    from enerf_amd.graph import GraphedFrame
    cfg = EnerfConfig.dtu_eval()
    h, w = 256, 320
    net = _net(cfg)
    lib = net.lib
    views, tar, cam_points, cams = _interactive_scene(cfg, h, w)
    cache = net.cache_sources(*views)

    def loop(b):
        idx = lib.select_views(cam_points, b["c2w"], 3)
        out = dict(net.forward_cached(cache, idx, b))
        out["near_views"] = idx
        out["rgb8"] = lib.pack_rgb8(out["rgb_level1"][0], h, w)
        return out

    batches = [dict(tar, tar_ext=ext, c2w=c2w) for ext, c2w in cams]
    eager = [{k: v.clone() for k, v in loop(b).items()} for b in batches]
    torch.cuda.synchronize()
    assert len({tuple(e["near_views"].tolist()) for e in eager}) >= 2   # the cameras really select different views
    for e, b in zip(eager, batches):                                   # and the eager loop is today's frame on those views
        ref = net(_by_hand(views, b, e["near_views"].tolist()))
        for k in ref:
            assert torch.equal(e[k], ref[k]), k
    frame = GraphedFrame(net, batches[0], fn=loop)
    for b, e in list(zip(batches, eager)) + [(batches[0], eager[0])]:
        out = frame(b)
        torch.cuda.synchronize()
        for k in e:
            assert torch.equal(out[k], e[k]), k
    # in place between replays: the caller writes the static target tensors itself
    frame.static_in["tar_ext"].copy_(batches[2]["tar_ext"])
    frame.static_in["c2w"].copy_(batches[2]["c2w"])
    frame.graph.replay()
    torch.cuda.synchronize()
    for k in eager[2]:
        assert torch.equal(frame.static_out[k], eager[2][k]), k


def test_interactive_loop_has_no_implicit_host_sync():
    """Under ``torch.cuda.set_sync_debug_mode("error")`` any implicit synchronisation raises: the view index never reaches the host
    (plain network, and the human variant with static_shapes)."""
    cfg = EnerfConfig.dtu_eval()
    h, w = 128, 160
    for human in (False, True):
        net = _net(cfg, human=human, static_shapes=human)
        lib = net.lib
        views, tar, cam_points, cams = _interactive_scene(cfg, h, w, human)
        net.prepare()
        cache = net.cache_sources(*views)
        b = dict(tar, tar_ext=cams[1][0], c2w=cams[1][1])
        warm = net.forward_cached(cache, lib.select_views(cam_points, b["c2w"], 3), b)     # sizes the workspace
        ref = {k: v.clone() for k, v in warm.items()}
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            fresh = net.cache_sources(*views)                           # the build does not synchronise either
            idx = lib.select_views(cam_points, b["c2w"], 3)
            out = net.forward_cached(fresh, idx, b)
            rgb8 = lib.pack_rgb8(out["rgb_level1"][0], h, w)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        assert torch.equal(out["rgb_level1"], ref["rgb_level1"]) and rgb8.shape == (h, w, 3)
