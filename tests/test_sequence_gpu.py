"""Dynamic scenes on a real MI355X, through libenerf_hip.so: the GPU twins of tests/test_ingest.py (``enerf_ingest_views_u8`` bit
for bit at all 256 values, both load paths, every dilation; ``enerf_bounds_near_far`` within its derived bound; the uint8 cache and
its in-place rebuild) and of tests/test_sequence.py — the :class:`SequencePlayer` rebuilding one slot on its build stream while the
other is rendered from, every output equal to ``Network.forward`` on the float restatement computed BEFOREHAND, serially — and no
implicit host synchronisation in submit / flip / render / bounds_near_far.  Every float restatement is computed on the CPU."""
import pytest
import torch

import __graft_entry__ as G
from enerf_amd.config import EnerfConfig
from enerf_amd.lib import EnerfError
from sequence_cases import (CAMERAS, NEAR_FAR_CASES, all_values_image, assert_same, by_hand, check_near_far, edge_masks, play, restate,
                            time_frames)

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU (run with -m gpu on the MI355X box)")]
CFG = EnerfConfig().with_cas(volume_planes=(8, 8), render_if=(False, True))
V, DILATE = 5, 5
SEEDS = (3, 4, 5, 6)


def _dev():
    return torch.device("cuda:0")


def _lib():
    from enerf_amd.lib import get_lib
    return get_lib()


def _ingest(img, mask=None, dilate=0):
    out = _lib().ingest_views_u8(img.to(_dev()), None if mask is None else mask.to(_dev()), dilate)
    return out.cpu()


def test_all_256_values_bit_exact():
    img = all_values_image()
    assert torch.equal(_ingest(img), (img.float() / 255 * 2 - 1).permute(0, 3, 1, 2))


@pytest.mark.parametrize("dilate", [0, 3, 5, 9])
@pytest.mark.parametrize("hw", [(13, 22), (16, 24)], ids=["byte_path_13x22", "aligned_16x24"])
def test_mask_dilation_and_unaligned_rows(hw, dilate):
    H, W = hw
    g = torch.Generator().manual_seed(H * W + dilate)
    img = torch.randint(0, 256, (2, H, W, 3), generator=g, dtype=torch.uint8)
    for second in (0, 255):
        mask = edge_masks(H, W, second)
        ref = restate(img, mask, dilate)
        out = _ingest(img, mask, dilate)
        assert torch.equal(out, ref), second
        assert bool((out[1] == -1).all()) == (second == 0)
        assert torch.equal(_ingest(img, mask != 0, dilate), ref)
        buf = torch.zeros(mask.numel() + 1, dtype=torch.uint8, device=_dev())      # a mask that is not dword-aligned in memory
        buf[1:] = mask.flatten().to(_dev())
        assert torch.equal(_lib().ingest_views_u8(img.to(_dev()), buf[1:].view(2, H, W), dilate).cpu(), ref)


def test_tile_seams_and_a_frame_sized_image():
    """20 x 260: two tiles each way, the dilation crosses both seams.  72 x 516 x V = 5: several blocks per view, fast path."""
    g = torch.Generator().manual_seed(5)
    img = torch.randint(0, 256, (1, 20, 260, 3), generator=g, dtype=torch.uint8)
    mask = torch.zeros((1, 20, 260), dtype=torch.uint8)
    for y, x in ((15, 255), (16, 256), (3, 254), (17, 100), (14, 258)):
        mask[0, y, x] = 9
    for dilate in (0, 3, 9):
        assert torch.equal(_ingest(img, mask, dilate), restate(img, mask, dilate)), dilate
    img = torch.randint(0, 256, (5, 72, 516, 3), generator=g, dtype=torch.uint8)
    mask = (torch.rand((5, 72, 516), generator=g) < 0.02).to(torch.uint8) * 200
    for dilate in (0, 5, 9):
        assert torch.equal(_ingest(img, mask, dilate), restate(img, mask, dilate)), dilate
    assert torch.equal(_ingest(img), restate(img))


def test_refusals_launch_nothing():
    lib = _lib()
    img = torch.zeros((1, 4, 4, 3), dtype=torch.uint8, device=_dev())
    out = torch.full((1, 3, 4, 4), 7.0, device=_dev())
    for dilate in (4, 11):
        with pytest.raises(EnerfError, match=r"dilate=%d" % dilate):
            lib.ingest_views_u8(img, None, dilate, out=out)
    call = lib.dll.enerf_ingest_views_u8
    assert call(img.data_ptr(), None, 0, 0, 4, 4, out.data_ptr(), None) == -1 and b"V=0" in lib.dll.enerf_last_error()
    assert call(None, None, 0, 1, 4, 4, out.data_ptr(), None) == -1 and b"null img" in lib.dll.enerf_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


def test_cache_from_uint8_and_rebuild_in_place():
    H, W = 32, 64
    dev = _dev()
    net = G._seeded_network(CFG, dev)
    frames, exts, ixts, tar = time_frames(CFG, H, W, V, seeds=(3, 4))
    exts, ixts, tar = exts.to(dev), ixts.to(dev), {k: v.to(dev) for k, v in tar.items()}
    (u8a, ma), (u8b, mb) = frames
    fa, fb = restate(u8a, ma, DILATE).to(dev), restate(u8b, mb, DILATE).to(dev)

    def same_buffers(x, y):
        for p, q in zip(x.buffers, y.buffers):
            assert (p is None) == (q is None) and (p is None or torch.equal(p, q))

    idx = torch.tensor(CAMERAS[0], dtype=torch.int32, device=dev)
    cache = net.cache_sources(u8a.to(dev), exts, ixts, ma.to(dev), dilate=DILATE)
    same_buffers(cache, net.cache_sources(fa, exts, ixts))
    assert_same(net.forward_cached(cache, idx, tar), net(by_hand(fa, exts, ixts, tar, CAMERAS[0])))
    ptrs = [None if b is None else b.data_ptr() for b in cache.buffers]
    cache.rebuild(u8b.to(dev), masks=mb.to(dev), dilate=DILATE)
    assert ptrs == [None if b is None else b.data_ptr() for b in cache.buffers]
    same_buffers(cache, net.cache_sources(fb, exts, ixts))
    assert_same(net.forward_cached(cache, idx, tar), net(by_hand(fb, exts, ixts, tar, CAMERAS[0])))
    with pytest.raises(ValueError, match="V=5"):
        cache.rebuild(u8a[:4].to(dev))


@pytest.mark.parametrize("case", sorted(NEAR_FAR_CASES))
def test_bounds_near_far_against_float64(case):
    vertices, exts, near_min = NEAR_FAR_CASES[case]
    check_near_far(_lib(), vertices, exts, near_min, device=_dev())


# -- the player ------------------------------------------------------------------------------------------------------------------
# 64 x 96.  A whole frame of this cascade needs H and W divisible by 32 (level 0's 1/8-scale volume goes through a network that
# halves it twice: 40 x 72 is refused by enerf_cost_reg, "D,h,w (8,5,9) must be divisible by 4"), so the full-resolution map is
# always whole 8 x 32 FeatureNet tiles; at 64 x 96 the half-resolution map is 32 x 48 = 4 x 1.5 tiles and the quarter-resolution
# one 16 x 24 = 2 x 0.75 tiles, so the cache build cuts tile edges in smooth1, conv1 and conv2 — the smallest such frame with more
# than one tile row at full resolution.
H, W = 64, 96


def _scene(human=False, seeds=SEEDS):
    """Network, time frames, cameras on the device, and the reference of every (time frame, camera) computed serially up front."""
    dev = _dev()
    net = G._seeded_network(CFG, dev, human=human)
    net.static_shapes = human
    frames, exts, ixts, tar = time_frames(CFG, H, W, V, seeds, mask_box=human)
    exts, ixts, tar = exts.to(dev), ixts.to(dev), {k: v.to(dev) for k, v in tar.items()}
    refs = {}
    for t, (u8, mask) in enumerate(frames):
        views = restate(u8, mask, DILATE).to(dev)
        for c, idx in enumerate(CAMERAS):
            refs[(t, c)] = {k: v.clone() for k, v in net(by_hand(views, exts, ixts, tar, idx)).items()}
    torch.cuda.synchronize()
    return net, frames, exts, ixts, tar, refs


@pytest.mark.parametrize("where", ["host_frames", "pinned_frames", "device_frames"])
def test_player_overlaps_rebuild_and_render_bit_exactly(where):
    from enerf_amd.sequence import SequencePlayer
    net, frames, exts, ixts, tar, refs = _scene()
    if where == "pinned_frames":
        frames = [(u8.pin_memory(), m.pin_memory()) for u8, m in frames]
    player = SequencePlayer(net, exts, ixts, H, W, slots=2, dilate=DILATE)
    for rounds in range(2):                                             # the second round reuses warm slots and staging buffers
        outs = play(player, frames, tar, _dev(), to_device=where == "device_frames")
        torch.cuda.synchronize()
        assert sorted(outs) == sorted(refs)
        for key, ref in refs.items():
            assert_same(outs[key], ref)
    assert not torch.equal(refs[(0, 0)]["rgb_level1"], refs[(1, 0)]["rgb_level1"])
    player.submit(*frames[0])
    with pytest.raises(RuntimeError, match="no free slot"):
        player.submit(*frames[1])
    torch.cuda.synchronize()
    caches = sum(s.cache.nbytes() for s in player.slots)
    assert player.nbytes() == caches + V * H * W * 16 + player._workspace.numel() * 4 and player.pinned_nbytes() == 2 * V * H * W * 4


def test_human_network_with_mask_at_box_renders_through_the_player():
    from enerf_amd.sequence import SequencePlayer
    net, frames, exts, ixts, tar, refs = _scene(human=True, seeds=SEEDS[:2])
    player = SequencePlayer(net, exts, ixts, H, W, slots=2, dilate=DILATE)
    outs = play(player, frames, tar, _dev())
    torch.cuda.synchronize()
    m = int(tar["mask_at_box"].bool().sum())
    assert 1 < m < H * W
    for key, ref in refs.items():
        out = outs[key]
        assert int(out["num_rays_level1"][0]) == m
        assert_same(out, ref, ("rgb_level1", "depth_mvs_level1", "std_level1"))
        for k in ("depth_level1", "weights_level1"):                   # rows past the count are never written
            assert torch.equal(out[k][:, :m], ref[k][:, :m]), k


def test_player_and_bounds_have_no_implicit_host_sync():
    """Under ``torch.cuda.set_sync_debug_mode("error")`` any implicit synchronisation raises."""
    from enerf_amd.sequence import SequencePlayer
    net, frames, exts, ixts, tar, refs = _scene(seeds=SEEDS[:3])
    lib = net.lib
    vertices, _, _ = NEAR_FAR_CASES["two_cameras"]
    vertices = vertices.to(_dev())
    player = SequencePlayer(net, exts, ixts, H, W, slots=2, dilate=DILATE)
    frames = [(u8.pin_memory(), m.pin_memory()) for u8, m in frames]
    tar = dict(tar)
    near_far = tar.pop("near_far")
    idx = [torch.tensor(c, dtype=torch.int32, device=_dev()) for c in CAMERAS]
    player.submit(*frames[0])                                           # warm: sizes the frame workspace, creates the events
    player.flip()
    player.render(idx[0], dict(tar, near_far=near_far))
    torch.cuda.synchronize()
    outs = {}
    torch.cuda.set_sync_debug_mode("error")
    try:
        nf = lib.bounds_near_far(vertices, tar["tar_ext"], 0.05)
        for t in (1, 2):
            player.submit(*frames[t])
            outs[(t - 1, 0)] = player.render(idx[0], dict(tar, near_far=near_far))
            outs[(t - 1, 1)] = player.render(idx[1], dict(tar, near_far=near_far))
            player.flip()
        outs[(2, 0)] = player.render(idx[0], dict(tar, near_far=near_far))
        by_bounds = player.render(idx[0], dict(tar, near_far=nf))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    for key, out in outs.items():
        assert_same(out, refs[key])
    assert nf.shape == (1, 2) and bool(torch.isfinite(by_bounds["rgb_level1"]).all())
