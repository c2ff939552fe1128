"""``enerf_ingest_raw_u8`` (raw camera frames: undistort, area resize, crop) on the CPU lane emulator, against the float64 restatement
of its specification (tests/ingest_raw_cases.py) under the derived bound (2 (9 + n) + 1) 2^-24, and the ``raw=`` wiring of the
source-view caches and the sequence player.  The GPU twins are in tests/test_ingest_raw_gpu.py.

Worst |err| / bound measured on the emulator: 0.14 (area only), 0.19 (undistort + area); every case prints its own."""
import numpy as np
import pytest
import torch

import __graft_entry__ as G
import ingest_raw_cases as R
from emu_lib import emu_lib
from enerf_amd.config import EnerfConfig
from enerf_amd.lib import EnerfError
from enerf_amd.raw_ingest import RawIngest
from sequence_cases import all_values_image, edge_masks

DEV = "cpu"


# -- 1. identity -------------------------------------------------------------------------------------
def test_identity_all_256_values():
    lib = emu_lib()
    img = all_values_image()
    assert torch.equal(lib.ingest_raw_u8(img), lib.ingest_views_u8(img))


@pytest.mark.parametrize("dilate", [0, 5])
@pytest.mark.parametrize("hw", [(13, 22), (16, 24)], ids=["byte_path_13x22", "aligned_16x24"])
def test_identity_equals_ingest_views_u8(hw, dilate):
    lib = emu_lib()
    H, W = hw
    img = R.raw_frame(2, H, W, seed=H * W + dilate)
    mask = edge_masks(H, W, 255)
    want = lib.ingest_views_u8(img, mask, dilate)
    assert bool((want == -1).any()) and bool((want != -1).any())
    mo = torch.full((2, H, W), 7, dtype=torch.uint8)
    assert torch.equal(lib.ingest_raw_u8(img, None, None, mask, dilate, mask_out=mo), want)
    for v in range(2):
        assert np.array_equal(mo[v].numpy(), R._dilate(mask[v].numpy() != 0, dilate).astype(np.uint8))
    assert torch.equal(lib.ingest_raw_u8(img), lib.ingest_views_u8(img))
    # intrinsics without a distortion tensor are not read: still the identity
    K, _ = R.cams(2, H, W)
    assert torch.equal(lib.ingest_raw_u8(img, K, None, mask, dilate), want)


# -- 2. area only --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.AREA_CASES, ids=[c[0] for c in R.AREA_CASES])
def test_area_only(case):
    name, Hraw, Wraw, r = case
    img = R.raw_frame(2, Hraw, Wraw, seed=Hraw + Wraw)
    out, ref, _ = R.check(emu_lib(), DEV, name, img, r=r)
    assert tuple(out.shape[2:]) == R.geometry(Hraw, Wraw, r) == emu_lib().ingest_raw_geometry(Hraw, Wraw, r)
    if name == "half_40x56":                                             # the 2x2 mean
        x = img.double() / 255
        mean = (x[:, 0::2, 0::2] + x[:, 0::2, 1::2] + x[:, 1::2, 0::2] + x[:, 1::2, 1::2]) / 4
        assert float((out.double() - (2 * mean - 1).permute(0, 3, 1, 2)).abs().max()) <= R.bound(4)


# -- 3. undistort -----------------------------------------------------------------------------------
def test_zero_coefficients_take_the_bilinear_path_and_agree_with_the_identity():
    lib = emu_lib()
    img = R.raw_frame(1, 16, 24, seed=3)
    K, D = R.cams(1, 16, 24, coef=(0.0,) * 5, off=(1.5, -0.75))
    out, ref, _ = R.check(lib, DEV, "zero_coefficients", img, K, D)
    assert float((out - lib.ingest_views_u8(img)).abs().max()) <= R.bound(ref["n"])


@pytest.mark.parametrize("case", [("d_48x64_r075", 48, 64, 0.75), ("d_41x55_r05", 41, 55, 0.5), ("d_40x56_r025", 40, 56, 0.25),
                                  ("d_37x53_r1", 37, 53, 1.0)], ids=lambda c: c[0])
def test_undistort_off_centre_principal_point(case):
    name, Hraw, Wraw, r = case
    K, D = R.cams(1, Hraw, Wraw, off=(2.25, -1.5))
    R.check(emu_lib(), DEV, name, R.raw_frame(1, Hraw, Wraw, seed=Hraw), K, D, r=r)


def test_three_views_with_their_own_cameras():
    V, Hraw, Wraw = 3, 37, 53
    K, D = R.per_view_cameras(V, Hraw, Wraw)
    img = R.raw_frame(V, Hraw, Wraw, seed=8)
    out, _, _ = R.check(emu_lib(), DEV, "three_views", img, K, D, r=0.75)
    # the cameras matter: view 1 through view 0's camera is something else
    other, _ = R.run(emu_lib(), DEV, img[1:2], K[0:1], D[0:1], r=0.75)
    assert not torch.equal(other[0], out[1])


def test_strong_distortion_pushes_a_band_outside():
    Hraw, Wraw = 40, 56
    K, D = R.cams(1, Hraw, Wraw, coef=R.STRONG)
    img = R.raw_frame(1, Hraw, Wraw, seed=11).clamp_(min=1)              # no zero byte: -1 only where nothing was sampled
    out, ref, _ = R.check(emu_lib(), DEV, "strong", img, K, D, r=0.5)
    band = torch.from_numpy((ref["out"] == -1.0).all(axis=1))
    assert 0.1 < float(band.float().mean()) < 0.9
    assert bool((out.permute(0, 2, 3, 1)[band] == -1.0).all()) and bool((out.permute(0, 2, 3, 1)[~band] != -1.0).any())


# -- 4. crop ------------------------------------------------------------------------------------------
def test_outdoor_crop_is_a_slice_and_moves_the_intrinsics():
    lib = emu_lib()
    Hraw, Wraw, r = 64, 88, 0.75
    Hs, Ws = lib.ingest_raw_geometry(Hraw, Wraw, r)
    assert (Hs, Ws) == (48, 66)
    y0, x0 = RawIngest.outdoor_crop(Hs, Ws, 32, 64)
    assert (y0, x0) == (10, 1)
    K, D = R.cams(2, Hraw, Wraw, off=(1.25, 2.5))
    img = R.raw_frame(2, Hraw, Wraw, seed=21)
    full, _ = R.run(lib, DEV, img, K, D, r=r)
    out, _, _ = R.check(lib, DEV, "crop", img, K, D, r=r, crop=(y0, x0, 32, 64))
    assert torch.equal(out, full[:, :, y0:y0 + 32, x0:x0 + 64])
    rig = RawIngest(K, D, Hraw, Wraw, input_ratio=r, crop=(y0, x0, 32, 64), lib=lib)
    assert (rig.H, rig.W) == (32, 64) and torch.equal(rig(img), out)
    ixt = K.double().numpy().copy()                                      # enerf_outdoor/enerf.py:139-151
    ixt[:, :2] *= r
    ixt[:, 1, 2] -= y0
    ixt[:, 0, 2] -= x0
    assert np.array_equal(rig.ixts.numpy(), ixt.astype(np.float32)) and rig.ixts.dtype == torch.float32


# -- 5. tiles ---------------------------------------------------------------------------------------------
def test_more_than_one_tile_with_partial_last_tiles():
    """Raw 28 x 100 at 0.75 is 21 x 75: three 8-row and three 32-column tiles, the last of each partial."""
    Hraw, Wraw = 28, 100
    K, D = R.cams(1, Hraw, Wraw, off=(-3.0, 1.0))
    mask = R.blob_mask(1, Hraw, Wraw, seed=2)
    out, _, _ = R.check(emu_lib(), DEV, "tiles", R.raw_frame(1, Hraw, Wraw, seed=5), K, D, mask, 3, r=0.75)
    assert tuple(out.shape) == (1, 3, 21, 75)


# -- 6. mask, ZJU order ---------------------------------------------------------------------------
@pytest.mark.parametrize("dilate", [0, 5])
def test_mask_dilate_undistort_nearest_resize(dilate):
    lib = emu_lib()
    V, Hraw, Wraw = 2, 41, 55
    K, D = R.cams(V, Hraw, Wraw, off=(1.0, 0.5))
    img, mask = R.raw_frame(V, Hraw, Wraw, seed=31), R.blob_mask(V, Hraw, Wraw, seed=7)
    out, ref, _ = R.check(lib, DEV, f"mask_dilate{dilate}", img, K, D, mask, dilate, r=0.5)
    assert not ref["tie"].any() and 0.05 < ref["keep"].mean() < 0.95
    # a bool mask and a mask that is not dword-aligned in memory give the same bits
    assert torch.equal(lib.ingest_raw_u8(img, K, D, mask != 0, dilate, 0.5), out)
    buf = torch.zeros(mask.numel() + 1, dtype=torch.uint8)
    buf[1:] = mask.flatten()
    assert torch.equal(lib.ingest_raw_u8(img, K, D, buf[1:].view(V, Hraw, Wraw), dilate, 0.5), out)
    # ... and without distortion (the nearest resize of the dilated raw mask)
    R.check(lib, DEV, f"mask_area_dilate{dilate}", img, None, None, mask, dilate, r=0.5)


# -- 7. guards (emulator only: the GPU file keeps to the finite strong distortion) ------------------
@pytest.mark.parametrize("what", ["nan", "inf", "1e30", "fx0", "nan_K"])
def test_wild_cameras_give_minus_one_and_leave_the_neighbours_alone(what):
    lib = emu_lib()
    V, Hraw, Wraw = 3, 24, 40
    K, D = R.cams(V, Hraw, Wraw, off=(0.3, 0.4))                         # (no pixel sits on the principal point, where any D maps to itself)
    img, mask = R.raw_frame(V, Hraw, Wraw, seed=4).clamp_(min=1), R.blob_mask(V, Hraw, Wraw, seed=4)
    good, _ = R.run(lib, DEV, img, K, D, mask, 3, r=0.5, want_mask=True)
    K, D = K.clone(), D.clone()
    if what == "nan":
        D[1, 0] = float("nan")
    elif what == "inf":
        D[1, 2] = float("inf")
    elif what == "1e30":
        D[1] = torch.tensor([1e30, -1e30, 1e30, 1e30, 1e30])
    elif what == "fx0":
        K[1, 0, 0] = 0.0
    else:
        K[1, 1, 2] = float("nan")
    for m in (None, mask):
        out, mo = R.run(lib, DEV, img, K, D, m, 3 if m is not None else 0, r=0.5, want_mask=m is not None)
        assert bool((out[1] == -1.0).all()), what
        if m is not None:
            assert torch.equal(out[0], good[0]) and torch.equal(out[2], good[2]) and int(mo[1].max()) == 0


# -- 8. refusals ----------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    lib = emu_lib()
    img = torch.zeros((1, 8, 8, 3), dtype=torch.uint8)
    mask = torch.ones((1, 8, 8), dtype=torch.uint8)
    scratch = torch.zeros((1, 8, 8), dtype=torch.uint8)
    out = torch.full((1, 3, 4, 4), 7.0)
    call, err = lib.dll.enerf_ingest_raw_u8, lib.dll.enerf_last_error
    ip, mp, sp, op = img.data_ptr(), mask.data_ptr(), scratch.data_ptr(), out.data_ptr()
    EINVAL = -1

    def refused(text, *args):
        assert call(*args) == EINVAL and text in err(), (text, err())

    #                  img  mask ixts  dist  V  Hraw Wraw r   y0 x0 H  W  dil scratch out mask_out stream
    refused(b"null img", None, None, None, None, 1, 8, 8, 0.5, 0, 0, 4, 4, 0, None, op, None, None)
    refused(b"null out", ip, None, None, None, 1, 8, 8, 0.5, 0, 0, 4, 4, 0, None, None, None, None)
    refused(b"V=0", ip, None, None, None, 0, 8, 8, 0.5, 0, 0, 4, 4, 0, None, op, None, None)
    for r in (0.2, 1.01, float("nan"), 0.0, -0.5):
        refused(b"input_ratio", ip, None, None, None, 1, 8, 8, r, 0, 0, 4, 4, 0, None, op, None, None)
    for y0, x0, H, W in ((1, 0, 4, 4), (0, 1, 4, 4), (-1, 0, 4, 4), (0, 0, 5, 4), (0, 0, 4, 0)):
        refused(b"leaves the resized image", ip, None, None, None, 1, 8, 8, 0.5, y0, x0, H, W, 0, None, op, None, None)
    for dilate in (4, 11, 2, -3, 1):
        refused(b"dilate=%d" % dilate, ip, mp, None, None, 1, 8, 8, 0.5, 0, 0, 4, 4, dilate, sp, op, None, None)
    refused(b"mask_scratch", ip, mp, None, None, 1, 8, 8, 0.5, 0, 0, 4, 4, 5, None, op, None, None)
    assert bool((out == 7.0).all()) and bool((scratch == 0).all())       # nothing was launched
    assert call(ip, mp, None, None, 1, 8, 8, 0.5, 0, 0, 4, 4, 5, sp, op, None, None) == 0 and bool((out == -1.0).all())
    hs = lib.dll.enerf_ingest_raw_geometry
    assert hs(8, 8, 0.5, None, None) == EINVAL
    with pytest.raises(EnerfError, match="uint8"):
        lib.ingest_raw_u8(img.float())
    with pytest.raises(EnerfError, match=r"dist must be .*\(1, 5\)"):
        lib.ingest_raw_u8(img, torch.eye(3)[None], torch.zeros((1, 4)))
    with pytest.raises(EnerfError, match="out must be"):
        lib.ingest_raw_u8(img, input_ratio=0.5, out=torch.zeros((1, 3, 8, 8)))
    with pytest.raises(EnerfError, match="leaves the resized image"):
        lib.ingest_raw_u8(img, input_ratio=0.5, crop=(2, 2, 4, 4))
    with pytest.raises(ValueError, match="leaves the resized image"):
        RawIngest(torch.eye(3)[None], None, 8, 8, 0.5, crop=(2, 2, 4, 4))


def test_identity_across_the_dilation_kernels_tile_seams():
    """20 x 260 spans two 256-pixel tiles across and two 16-row tiles down of the mask dilation; nine 32-column output tiles."""
    lib = emu_lib()
    img = R.raw_frame(1, 20, 260, seed=5)
    mask = torch.zeros((1, 20, 260), dtype=torch.uint8)
    for y, x in ((15, 255), (16, 256), (3, 254), (17, 100), (14, 258)):
        mask[0, y, x] = 9
    for dilate in (0, 3, 9):
        assert torch.equal(lib.ingest_raw_u8(img, mask=mask, dilate=dilate), lib.ingest_views_u8(img, mask, dilate)), dilate


# -- 9. wiring -------------------------------------------------------------------------------------
CFG = EnerfConfig().with_cas(volume_planes=(8, 8), render_if=(False, True))


def test_source_cache_from_raw_frames_and_rebuild_in_place():
    lib = emu_lib()
    R.source_cache_case(lib, DEV, G._seeded_network(CFG, "cpu", lib=lib), CFG)


def test_composite_cache_from_raw_image_and_raw_background():
    R.composite_cache_case(emu_lib(), torch.device("cpu"), rebuild=False)       # (the in-place rebuild: tests/test_ingest_raw_gpu.py)


def test_sequence_player_over_four_raw_time_frames():
    from enerf_amd.sequence import SequencePlayer
    from sequence_cases import assert_same, play
    lib = emu_lib()
    H, W, V = 32, 64, 5
    net = G._seeded_network(CFG, "cpu", lib=lib)
    rig, exts, frames, tar, refs = R.player_scene(lib, "cpu", net, CFG, H, W, V, seeds=(3, 4, 5, 6))
    player = SequencePlayer(net, exts, rig.ixts, rig.H, rig.W, slots=2, dilate=5, raw=rig)
    assert tuple(player._img_u8.shape) == (V, 2 * H, 2 * W, 3) and tuple(player._mask_scratch.shape) == (V, 2 * H, 2 * W)
    outs = play(player, frames, tar, "cpu")
    assert sorted(outs) == sorted(refs)
    for key, ref in refs.items():
        assert_same(outs[key], ref)
    assert not torch.equal(outs[(0, 0)]["rgb_level1"], outs[(1, 0)]["rgb_level1"])
    with pytest.raises(ValueError, match=r"uint8 \(5,64,128,3\)"):
        player.submit(frames[0][0][:, :H, :W].contiguous())
    with pytest.raises(ValueError, match="raw= gives"):
        SequencePlayer(net, exts, rig.ixts, H, W + 32, raw=rig)


def test_all_256_values_through_the_bilinear_path_at_weight_one():
    """fx = fy = 64, an integer principal point and zero coefficients map every pixel onto itself EXACTLY (the divisions by a power of
    two round-trip), so the bilinear sample is 1 * x + 0 + 0 + 0: the tap values must be the correctly rounded u8 / 255 bit for bit."""
    lib = emu_lib()
    img = all_values_image()
    K = torch.tensor([[[64.0, 0.0, 8.0], [0.0, 64.0, 2.0], [0.0, 0.0, 1.0]]])
    assert torch.equal(lib.ingest_raw_u8(img, K, torch.zeros((1, 5))), lib.ingest_views_u8(img))
