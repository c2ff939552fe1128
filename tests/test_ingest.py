"""``enerf_ingest_views_u8`` and ``enerf_bounds_near_far`` on the CPU lane emulator, and the uint8 form of the source-view cache
(``Network.cache_sources`` on uint8 images, ``SourceCache.rebuild``).  The ingest is BIT-exact by contract: every comparison of
image data in this file is ``torch.equal`` against the float32 expression ``u8.float() / 255 * 2 - 1`` with the zeroing in between
(tests/sequence_cases.py ``restate``).  The GPU twins are in tests/test_sequence_gpu.py."""
import pytest
import torch

import __graft_entry__ as G
from emu_lib import emu_lib
from enerf_amd.config import EnerfConfig
from enerf_amd.lib import EnerfError
from sequence_cases import (NEAR_FAR_CASES, all_values_image, assert_same, by_hand, check_near_far, edge_masks, ext_matrix, restate,
                            time_frames)

CFG = EnerfConfig().with_cas(volume_planes=(8, 8), render_if=(False, True))


def test_all_256_values_bit_exact():
    lib = emu_lib()
    img = all_values_image()
    for c in range(3):
        assert sorted(img[0, :, :, c].flatten().tolist()) == list(range(256))
    out = lib.ingest_views_u8(img)
    ref = img.float() / 255 * 2 - 1
    assert out.shape == (1, 3, 4, 64) and torch.equal(out, ref.permute(0, 3, 1, 2))


@pytest.mark.parametrize("dilate", [0, 3, 5, 9])
@pytest.mark.parametrize("second", [0, 255], ids=["view1_all_zero", "view1_all_255"])
@pytest.mark.parametrize("hw", [(13, 22), (16, 24)], ids=["byte_path_13x22", "aligned_16x24"])
def test_mask_dilation_and_unaligned_rows(hw, second, dilate):
    lib = emu_lib()
    H, W = hw
    g = torch.Generator().manual_seed(H * W + dilate)
    img = torch.randint(0, 256, (2, H, W, 3), generator=g, dtype=torch.uint8)
    mask = edge_masks(H, W, second)
    out = lib.ingest_views_u8(img, mask, dilate)
    ref = restate(img, mask, dilate)
    assert torch.equal(out, ref)
    keep = (ref != -1).any(dim=1)                                       # a masked-out pixel is exactly -1 in all three channels
    r = dilate // 2
    want = torch.zeros((H, W), dtype=torch.bool)
    for y, x in mask[0].nonzero().tolist():
        want[max(y - r, 0):y + r + 1, max(x - r, 0):x + r + 1] = True
    assert bool((out[0][:, ~want] == -1).all()) and bool((out[1] == -1).all()) == (second == 0)
    assert bool((keep[0] <= want).all())
    # a bool mask and a mask that is not dword-aligned in memory (a view one byte into a buffer) give the same bits
    assert torch.equal(lib.ingest_views_u8(img, mask != 0, dilate), ref)
    buf = torch.zeros(mask.numel() + 1, dtype=torch.uint8)
    buf[1:] = mask.flatten()
    assert torch.equal(lib.ingest_views_u8(img, buf[1:].view(2, H, W), dilate), ref)


def test_more_than_one_tile_in_both_directions():
    """20 x 260 spans two 256-pixel tiles across and two 16-row tiles down: the dilation crosses both seams."""
    lib = emu_lib()
    H, W = 20, 260
    g = torch.Generator().manual_seed(5)
    img = torch.randint(0, 256, (1, H, W, 3), generator=g, dtype=torch.uint8)
    mask = torch.zeros((1, H, W), dtype=torch.uint8)
    for y, x in ((15, 255), (16, 256), (3, 254), (17, 100), (14, 258)):
        mask[0, y, x] = 9
    for dilate in (0, 3, 9):
        assert torch.equal(lib.ingest_views_u8(img, mask, dilate), restate(img, mask, dilate)), dilate


def test_refusals():
    lib = emu_lib()
    img = torch.zeros((1, 4, 4, 3), dtype=torch.uint8)
    out = torch.full((1, 3, 4, 4), 7.0)
    for dilate in (4, 11, 2, -3, 1):
        with pytest.raises(EnerfError, match=r"dilate=%d" % dilate):
            lib.ingest_views_u8(img, None, dilate, out=out)
    call = lib.dll.enerf_ingest_views_u8
    assert call(img.data_ptr(), None, 0, 0, 4, 4, out.data_ptr(), None) == -1           # ENERF_EINVAL
    assert b"V=0" in lib.dll.enerf_last_error()
    assert call(None, None, 0, 1, 4, 4, out.data_ptr(), None) == -1
    assert b"null img" in lib.dll.enerf_last_error()
    assert call(img.data_ptr(), None, 0, 1, 4, 4, None, None) == -1
    assert b"null out" in lib.dll.enerf_last_error()
    assert bool((out == 7.0).all())                                      # nothing was launched
    with pytest.raises(EnerfError, match="uint8"):
        lib.ingest_views_u8(img.float())
    with pytest.raises(EnerfError, match="null pointer"):
        lib._check(lib.dll.enerf_bounds_near_far(None, 8, out.data_ptr(), 1, 0.05, out.data_ptr(), None), "bounds_near_far")


# -- the uint8 cache --------------------------------------------------------------------------------
H, W, V = 32, 64, 5


def test_cache_from_uint8_equals_cache_from_its_float_restatement_and_rebuilds_in_place():
    net = G._seeded_network(CFG, "cpu", lib=emu_lib())
    frames, exts, ixts, tar = time_frames(CFG, H, W, V, seeds=(3, 4))
    (u8a, ma), (u8b, mb) = frames
    fa, fb = restate(u8a, ma, 5), restate(u8b, mb, 5)
    assert bool((fa == -1).any()) and not torch.equal(fa, fb)
    cache = net.cache_sources(u8a, exts, ixts, ma, dilate=5)
    ref_a = net.cache_sources(fa, exts, ixts)

    def same_buffers(x, y):
        assert len(x.buffers) == len(y.buffers)
        for p, q in zip(x.buffers, y.buffers):
            assert (p is None) == (q is None) and (p is None or torch.equal(p, q))

    same_buffers(cache, ref_a)
    idx = [3, 1, 4]
    out = net.forward_cached(cache, torch.tensor(idx, dtype=torch.int32), tar)
    assert_same(out, net(by_hand(fa, exts, ixts, tar, idx)))
    # in place: the same tensors and the same struct afterwards
    ptrs = [None if b is None else b.data_ptr() for b in cache.buffers]
    st = cache.struct
    assert cache.rebuild(u8b, masks=mb, dilate=5) is cache
    assert ptrs == [None if b is None else b.data_ptr() for b in cache.buffers] and cache.struct is st
    same_buffers(cache, net.cache_sources(fb, exts, ixts))
    out = net.forward_cached(cache, torch.tensor(idx, dtype=torch.int32), tar)
    assert_same(out, net(by_hand(fb, exts, ixts, tar, idx)))
    # a float frame rebuilds too, with new cameras, and with caller-owned scratch for the uint8 form
    ixts2 = ixts.clone()
    ixts2[:, :2] *= 1.01
    cache.rebuild(fa, exts, ixts2)
    same_buffers(cache, net.cache_sources(fa, exts, ixts2))
    image, ws = torch.empty((V, 3, H, W)), net.lib.source_cache_build_workspace(H, W, "cpu")
    cache.rebuild(u8a, exts, ixts, masks=ma, dilate=5, image=image, workspace=ws)
    same_buffers(cache, ref_a)
    assert torch.equal(image, fa)
    # the generation follows the weights
    net.load_state_dict(net.state_dict())
    with pytest.raises(RuntimeError, match="weights changed"):
        net.forward_cached(cache, torch.tensor(idx, dtype=torch.int32), tar)
    cache.rebuild(u8a, masks=ma, dilate=5)
    assert_same(net.forward_cached(cache, torch.tensor(idx, dtype=torch.int32), tar), net(by_hand(fa, exts, ixts, tar, idx)))
    # refusals: another V, H or W; masks with a float image; Network.forward on uint8
    with pytest.raises(ValueError, match="V=5"):
        cache.rebuild(u8a[:4], masks=ma[:4], dilate=5)
    with pytest.raises(ValueError, match="32x64"):
        cache.rebuild(torch.zeros((V, H, W + 4, 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match="uint8"):
        cache.rebuild(fa, masks=ma)
    with pytest.raises(RuntimeError, match="float32"):
        net(dict(by_hand(fa, exts, ixts, tar, idx), src_inps=u8a[idx].permute(0, 3, 1, 2)[None].contiguous()))


# -- bounds_near_far --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(NEAR_FAR_CASES))
def test_bounds_near_far_against_float64(case):
    vertices, exts, near_min = NEAR_FAR_CASES[case]
    got = check_near_far(emu_lib(), vertices, exts, near_min)
    if case == "box_straddles_the_camera_plane":
        assert float(got[0, 0]) == float(torch.tensor(0.1, dtype=torch.float32)) and float(got[0, 1]) > 0.5
    if case == "two_cameras":
        assert not torch.equal(got[0], got[1])
        per_set = check_near_far(emu_lib(), torch.stack([vertices, vertices + 5.0]), exts, near_min)     # (B,n,3) vertices
        assert torch.equal(per_set[0], got[0]) and not torch.equal(per_set[1], got[1])


def test_bounds_near_far_more_vertices_than_lanes():
    """n = 150 > 64 lanes: the strided loop and the wave reduction (the SMPL-sized vertex sets of zjumocap/enerf.py)."""
    g = torch.Generator().manual_seed(2)
    vertices = torch.randn((150, 3), generator=g) * torch.tensor([0.4, 0.9, 0.3]) + torch.tensor([0.0, 0.0, 2.5])
    check_near_far(emu_lib(), vertices, ext_matrix(0.2, -0.3, (0.1, 0.0, 0.3))[None], 0.1)
