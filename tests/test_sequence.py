"""``enerf_amd.sequence.SequencePlayer`` on the CPU lane emulator: four uint8 time frames streamed through two slots the way a
viewer drives it; every output of every rendered level must equal ``Network.forward`` on the float restatement of the same time
frame's views, bit for bit.  (On a CPU device the player has no streams: this file checks its bookkeeping and its arithmetic; the
overlap itself is exercised on the MI355X in tests/test_sequence_gpu.py.)"""
import pytest
import torch

import __graft_entry__ as G
from emu_lib import emu_lib
from enerf_amd.config import EnerfConfig
from enerf_amd.sequence import SequencePlayer
from sequence_cases import CAMERAS, assert_same, by_hand, play, restate, time_frames

CFG = EnerfConfig().with_cas(volume_planes=(8, 8), render_if=(False, True))
H, W, V, DILATE = 32, 64, 5, 5
SEEDS = (3, 4, 5, 6)


def test_four_time_frames_through_two_slots():
    net = G._seeded_network(CFG, "cpu", lib=emu_lib())
    frames, exts, ixts, tar = time_frames(CFG, H, W, V, SEEDS)
    player = SequencePlayer(net, exts, ixts, H, W, slots=2, dilate=DILATE)
    with pytest.raises(RuntimeError, match="no front slot"):
        player.render(torch.tensor(CAMERAS[0], dtype=torch.int32), tar)
    with pytest.raises(RuntimeError, match="nothing was submitted"):
        player.flip()
    builds = []
    rebuild = type(player.slots[0].cache).rebuild

    def counting(self, *a, **k):
        builds.append(player.slots.index(next(s for s in player.slots if s.cache is self)))
        return rebuild(self, *a, **k)

    for s in player.slots:
        s.cache.rebuild = counting.__get__(s.cache)
    outs = play(player, frames, tar, "cpu")
    assert builds == [0, 1, 0, 1]                                       # every slot rebuilt while the other was the front
    for t, (u8, mask) in enumerate(frames):
        views = restate(u8, mask, DILATE)
        for c, idx in enumerate(CAMERAS):
            assert_same(outs[(t, c)], net(by_hand(views, exts, ixts, tar, idx)))
    assert not torch.equal(outs[(0, 0)]["rgb_level1"], outs[(1, 0)]["rgb_level1"])
    # a second submit without a flip: the only other slot holds an unflipped frame
    player.submit(*frames[0])
    with pytest.raises(RuntimeError, match="no free slot"):
        player.submit(*frames[1])
    assert_same(player.render(torch.tensor(CAMERAS[1], dtype=torch.int32), tar), outs[(3, 1)])      # the front is untouched
    player.flip()
    assert_same(player.render(torch.tensor(CAMERAS[1], dtype=torch.int32), tar), outs[(0, 1)])
    # what it holds: two caches + uint8 frame and mask + float image + workspace
    own = V * H * W * (3 + 1 + 12) + player._workspace.numel() * 4
    assert player.nbytes() == own + 2 * player.slots[0].cache.nbytes() and player.pinned_nbytes() == 0
    with pytest.raises(ValueError, match=r"uint8 \(5,32,64,3\)"):
        player.submit(frames[0][0][:4])
    with pytest.raises(ValueError, match="slots"):
        SequencePlayer(net, exts, ixts, H, W, slots=1)


def test_three_slots_drop_the_older_unflipped_submission_and_frames_without_masks():
    net = G._seeded_network(CFG, "cpu", lib=emu_lib())
    frames, exts, ixts, tar = time_frames(CFG, H, W, V, SEEDS[:3])
    player = SequencePlayer(net, exts, ixts, H, W, slots=3, dilate=DILATE)
    idx = torch.tensor(CAMERAS[0], dtype=torch.int32)
    player.submit(frames[0][0])                                         # no mask: nothing is zeroed, whatever `dilate` says
    player.submit(*frames[1])
    player.flip()                                                       # the most recent one; frame 0 is dropped
    assert_same(player.render(idx, tar), net(by_hand(restate(*frames[1], DILATE), exts, ixts, tar, CAMERAS[0])))
    player.submit(frames[2][0], frames[2][1] != 0)                      # a bool mask; the slot never used yet is the oldest
    assert player._latest is player.slots[2]
    player.flip()
    assert_same(player.render(idx, tar), net(by_hand(restate(*frames[2], DILATE), exts, ixts, tar, CAMERAS[0])))
    player.submit(frames[0][0])                                         # then the dropped one
    assert player._latest is player.slots[0]
    player.flip()
    assert_same(player.render(idx, tar), net(by_hand(restate(frames[0][0]), exts, ixts, tar, CAMERAS[0])))


def test_human_network_with_mask_at_box_renders_through_the_player():
    net = G._seeded_network(CFG, "cpu", human=True, lib=emu_lib())
    net.static_shapes = True
    frames, exts, ixts, tar = time_frames(CFG, H, W, V, SEEDS[:2], mask_box=True)
    player = SequencePlayer(net, exts, ixts, H, W, slots=2, dilate=DILATE)
    outs = play(player, frames, tar, "cpu")
    m = int(tar["mask_at_box"].bool().sum())
    assert 1 < m < H * W
    for t, (u8, mask) in enumerate(frames):
        views = restate(u8, mask, DILATE)
        for c, idx in enumerate(CAMERAS):
            ref = net(by_hand(views, exts, ixts, tar, idx))
            out = outs[(t, c)]
            assert int(out["num_rays_level1"][0]) == m
            assert_same(out, ref, ("rgb_level1", "depth_mvs_level1", "std_level1"))
            for k in ("depth_level1", "weights_level1"):               # rows past the count are never written
                assert torch.equal(out[k][:, :m], ref[k][:, :m]), k
