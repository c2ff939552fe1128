"""``enerf_ingest_raw_u8`` on a real MI355X, through libenerf_hip.so: the GPU twins of tests/test_ingest_raw.py.  Every reference —
the float64 restatement of tests/ingest_raw_cases.py and its bound (2 (9 + n) + 1) 2^-24 — is computed on the CPU.  Non-finite
cameras stay with the emulator file; the only out-of-image case here is the finite strong distortion.

Worst |err| / bound measured on an MI355X: 0.13 (area only), 0.17 (undistort + area); every case prints its own."""
import numpy as np
import pytest
import torch

import __graft_entry__ as G
import ingest_raw_cases as R
from enerf_amd.config import EnerfConfig
from enerf_amd.raw_ingest import RawIngest
from sequence_cases import CAMERAS, all_values_image, assert_same, edge_masks, play

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU (run with -m gpu on the MI355X box)")]
CFG = EnerfConfig().with_cas(volume_planes=(8, 8), render_if=(False, True))


def _dev():
    return torch.device("cuda:0")


def _lib():
    from enerf_amd.lib import get_lib
    return get_lib()


# -- 1. identity -------------------------------------------------------------------------------------
def test_identity_all_256_values():
    img = all_values_image().to(_dev())
    assert torch.equal(_lib().ingest_raw_u8(img), _lib().ingest_views_u8(img))


@pytest.mark.parametrize("dilate", [0, 5])
@pytest.mark.parametrize("hw", [(13, 22), (16, 24), (20, 260)], ids=["byte_path_13x22", "aligned_16x24", "dilation_seams_20x260"])
def test_identity_equals_ingest_views_u8(hw, dilate):
    lib, dev = _lib(), _dev()
    H, W = hw
    img = R.raw_frame(2, H, W, seed=H * W + dilate).to(dev)
    mask = edge_masks(H, W, 255)
    if W > 256:
        for y, x in ((15, 255), (16, 256), (3, 254), (14, 258)):
            mask[0, y, x] = 9
    want = lib.ingest_views_u8(img, mask.to(dev), dilate)
    mo = torch.full((2, H, W), 7, dtype=torch.uint8, device=dev)
    assert torch.equal(lib.ingest_raw_u8(img, None, None, mask.to(dev), dilate, mask_out=mo), want)
    for v in range(2):
        assert np.array_equal(mo[v].cpu().numpy(), R._dilate(mask[v].numpy() != 0, dilate).astype(np.uint8))
    assert torch.equal(lib.ingest_raw_u8(img), lib.ingest_views_u8(img))


# -- 2. area only --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.AREA_CASES, ids=[c[0] for c in R.AREA_CASES])
def test_area_only(case):
    name, Hraw, Wraw, r = case
    out, _, _ = R.check(_lib(), _dev(), name, R.raw_frame(2, Hraw, Wraw, seed=Hraw + Wraw), r=r)
    assert tuple(out.shape[2:]) == R.geometry(Hraw, Wraw, r) == _lib().ingest_raw_geometry(Hraw, Wraw, r)


# -- 3. undistort -----------------------------------------------------------------------------------
def test_zero_coefficients_take_the_bilinear_path_and_agree_with_the_identity():
    img = R.raw_frame(1, 16, 24, seed=3)
    K, D = R.cams(1, 16, 24, coef=(0.0,) * 5, off=(1.5, -0.75))
    out, ref, _ = R.check(_lib(), _dev(), "zero_coefficients", img, K, D)
    assert float((out - _lib().ingest_views_u8(img.to(_dev())).cpu()).abs().max()) <= R.bound(ref["n"])


@pytest.mark.parametrize("case", [("d_48x64_r075", 48, 64, 0.75), ("d_41x55_r05", 41, 55, 0.5), ("d_40x56_r025", 40, 56, 0.25),
                                  ("d_37x53_r1", 37, 53, 1.0)], ids=lambda c: c[0])
def test_undistort_off_centre_principal_point(case):
    name, Hraw, Wraw, r = case
    K, D = R.cams(1, Hraw, Wraw, off=(2.25, -1.5))
    R.check(_lib(), _dev(), name, R.raw_frame(1, Hraw, Wraw, seed=Hraw), K, D, r=r)


def test_three_views_with_their_own_cameras():
    V, Hraw, Wraw = 3, 37, 53
    K, D = R.per_view_cameras(V, Hraw, Wraw)
    R.check(_lib(), _dev(), "three_views", R.raw_frame(V, Hraw, Wraw, seed=8), K, D, r=0.75)


def test_strong_finite_distortion_pushes_a_band_outside():
    Hraw, Wraw = 40, 56
    K, D = R.cams(1, Hraw, Wraw, coef=R.STRONG)
    img = R.raw_frame(1, Hraw, Wraw, seed=11).clamp_(min=1)
    out, ref, _ = R.check(_lib(), _dev(), "strong", img, K, D, r=0.5)
    band = torch.from_numpy((ref["out"] == -1.0).all(axis=1))
    assert 0.1 < float(band.float().mean()) < 0.9
    assert bool((out.permute(0, 2, 3, 1)[band] == -1.0).all()) and bool((out.permute(0, 2, 3, 1)[~band] != -1.0).any())


# -- 4. crop ------------------------------------------------------------------------------------------
def test_outdoor_crop_is_a_slice_and_moves_the_intrinsics():
    lib, dev = _lib(), _dev()
    Hraw, Wraw, r = 64, 88, 0.75
    y0, x0 = RawIngest.outdoor_crop(*lib.ingest_raw_geometry(Hraw, Wraw, r), 32, 64)
    assert (y0, x0) == (10, 1)
    K, D = R.cams(2, Hraw, Wraw, off=(1.25, 2.5))
    img = R.raw_frame(2, Hraw, Wraw, seed=21)
    full, _ = R.run(lib, dev, img, K, D, r=r)
    out, _, _ = R.check(lib, dev, "crop", img, K, D, r=r, crop=(y0, x0, 32, 64))
    assert torch.equal(out, full[:, :, y0:y0 + 32, x0:x0 + 64])
    rig = RawIngest(K.to(dev), D.to(dev), Hraw, Wraw, input_ratio=r, crop=(y0, x0, 32, 64))
    assert torch.equal(rig(img.to(dev)).cpu(), out) and rig.ixts.is_cuda


# -- 5. tiles ---------------------------------------------------------------------------------------------
def test_more_than_one_tile_with_partial_last_tiles():
    Hraw, Wraw = 28, 100
    K, D = R.cams(1, Hraw, Wraw, off=(-3.0, 1.0))
    mask = R.blob_mask(1, Hraw, Wraw, seed=2)
    out, _, _ = R.check(_lib(), _dev(), "tiles", R.raw_frame(1, Hraw, Wraw, seed=5), K, D, mask, 3, r=0.75)
    assert tuple(out.shape) == (1, 3, 21, 75)


# -- 6. mask, ZJU order ---------------------------------------------------------------------------
@pytest.mark.parametrize("dilate", [0, 5])
def test_mask_dilate_undistort_nearest_resize(dilate):
    lib, dev = _lib(), _dev()
    V, Hraw, Wraw = 2, 41, 55
    K, D = R.cams(V, Hraw, Wraw, off=(1.0, 0.5))
    img, mask = R.raw_frame(V, Hraw, Wraw, seed=31), R.blob_mask(V, Hraw, Wraw, seed=7)
    out, ref, _ = R.check(lib, dev, f"mask_dilate{dilate}", img, K, D, mask, dilate, r=0.5)
    assert not ref["tie"].any()
    args = (img.to(dev), K.to(dev), D.to(dev))
    assert torch.equal(lib.ingest_raw_u8(*args, (mask != 0).to(dev), dilate, 0.5).cpu(), out)
    buf = torch.zeros(mask.numel() + 1, dtype=torch.uint8, device=dev)
    buf[1:] = mask.flatten().to(dev)
    assert torch.equal(lib.ingest_raw_u8(*args, buf[1:].view(V, Hraw, Wraw), dilate, 0.5).cpu(), out)
    R.check(lib, dev, f"mask_area_dilate{dilate}", img, None, None, mask, dilate, r=0.5)


# -- 8. refusals ----------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    lib, dev = _lib(), _dev()
    img = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=dev)
    mask = torch.ones((1, 8, 8), dtype=torch.uint8, device=dev)
    out = torch.full((1, 3, 4, 4), 7.0, device=dev)
    call, err = lib.dll.enerf_ingest_raw_u8, lib.dll.enerf_last_error
    ip, mp, op = img.data_ptr(), mask.data_ptr(), out.data_ptr()
    assert call(None, None, None, None, 1, 8, 8, 0.5, 0, 0, 4, 4, 0, None, op, None, None) == -1 and b"null img" in err()
    assert call(ip, None, None, None, 0, 8, 8, 0.5, 0, 0, 4, 4, 0, None, op, None, None) == -1 and b"V=0" in err()
    assert call(ip, None, None, None, 1, 8, 8, 0.2, 0, 0, 4, 4, 0, None, op, None, None) == -1 and b"input_ratio" in err()
    assert call(ip, None, None, None, 1, 8, 8, 0.5, 1, 0, 4, 4, 0, None, op, None, None) == -1 and b"leaves the resized image" in err()
    assert call(ip, mp, None, None, 1, 8, 8, 0.5, 0, 0, 4, 4, 4, None, op, None, None) == -1 and b"dilate=4" in err()
    assert call(ip, mp, None, None, 1, 8, 8, 0.5, 0, 0, 4, 4, 5, None, op, None, None) == -1 and b"mask_scratch" in err()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# -- 9. wiring -------------------------------------------------------------------------------------
def test_source_cache_from_raw_frames_and_rebuild_in_place():
    R.source_cache_case(_lib(), _dev(), G._seeded_network(CFG, _dev()), CFG)


def test_composite_cache_from_raw_image_and_raw_background():
    R.composite_cache_case(_lib(), _dev())


def test_sequence_player_over_raw_time_frames_without_a_host_sync():
    """Four raw time frames through two slots equal ``forward`` on the float images computed beforehand; under
    ``torch.cuda.set_sync_debug_mode("error")`` any implicit synchronisation in submit / flip / render raises."""
    from enerf_amd.sequence import SequencePlayer
    lib, dev = _lib(), _dev()
    H, W, V = 64, 96, 5
    net = G._seeded_network(CFG, dev)
    rig, exts, frames, tar, refs = R.player_scene(lib, dev, net, CFG, H, W, V, seeds=(3, 4, 5, 6))
    torch.cuda.synchronize()
    player = SequencePlayer(net, exts, rig.ixts, rig.H, rig.W, slots=2, dilate=5, raw=rig)
    frames = [(u8.pin_memory(), m.pin_memory()) for u8, m in frames]
    outs = play(player, frames, tar, dev)                               # warm: sizes the frame workspace, creates the events
    torch.cuda.synchronize()
    for key, ref in refs.items():
        assert_same(outs[key], ref)
    idx = [torch.tensor(c, dtype=torch.int32, device=dev) for c in CAMERAS]
    torch.cuda.synchronize()
    outs = {}
    torch.cuda.set_sync_debug_mode("error")
    try:
        player.submit(*frames[0])
        player.flip()
        for t in range(len(frames)):
            if t + 1 < len(frames):
                player.submit(*frames[t + 1])
            for c, i in enumerate(idx):
                outs[(t, c)] = player.render(i, tar)
            if t + 1 < len(frames):
                player.flip()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    for key, ref in refs.items():
        assert_same(outs[key], ref)
    assert not torch.equal(refs[(0, 0)]["rgb_level1"], refs[(1, 0)]["rgb_level1"])


def test_all_256_values_through_the_bilinear_path_at_weight_one():
    """fx = fy = 64, an integer principal point and zero coefficients map every pixel onto itself EXACTLY, so the bilinear sample is
    1 * x + 0 + 0 + 0: the tap values must be the correctly rounded u8 / 255 bit for bit."""
    lib, dev = _lib(), _dev()
    img = all_values_image().to(dev)
    K = torch.tensor([[[64.0, 0.0, 8.0], [0.0, 64.0, 2.0], [0.0, 0.0, 1.0]]], device=dev)
    assert torch.equal(lib.ingest_raw_u8(img, K, torch.zeros((1, 5), device=dev)), lib.ingest_views_u8(img))
