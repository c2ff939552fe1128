"""``enerf_vhull_bounds`` on a real MI355X, through libenerf_hip.so: the GPU twins of tests/test_vhull.py.  The arbiter — the float64
restatement of the model in tests/vhull_cases.py — runs on the CPU.  Besides the shared cases: a captured graph replayed over
changed masks (what tests that the enqueued work resets its own accumulators) and the sequence player with its build stream.

Worst undecided share measured on an MI355X run: 10 of 599,040 voxels (0.0017 %, cap 0.1 %) in the 130 x 64 x 72 later-passes case, whose
count then lies between the arbiter's two; 0 in every other case (asserted per case); every case prints its own."""
import numpy as np
import pytest
import torch

import __graft_entry__ as G
import vhull_cases as C
from enerf_amd.config import EnerfConfig

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU (run with -m gpu on the MI355X box)")]
CFG = EnerfConfig().with_cas(volume_planes=(8, 8), render_if=(False, True))


def _dev():
    return torch.device("cuda:0")


def _lib():
    from enerf_amd.lib import get_lib
    return get_lib()


def test_ellipsoid_every_voxel_inside_the_shrunk_ellipsoid_is_occupied():
    C.case_ellipsoid(_lib(), _dev())


@pytest.mark.parametrize("name", sorted(C.GRID_SHAPES))
def test_grid_shapes(name):
    C.case_grid(_lib(), _dev(), name)


def test_a_grid_larger_than_the_launch_makes_later_passes():
    """130 x 64 x 72 is 13,824 runs (three along x, the last of two voxels), 3,456 blocks' worth against the 2,048 that 256 CUs are
    given: waves take second runs.  All-ones masks: every voxel every camera sees is occupied, and the count is the arbiter's."""
    masks, exts, ixts, scene, _ = C.ellipsoid_case()
    grid = (130, 64, 72)
    t = lambda a: torch.from_numpy(a).to(_dev())                           # noqa: E731
    bounds, counts, flags, _ = _lib().vhull_bounds(t(np.ones_like(masks)), t(exts), t(ixts), scene, grid=grid, min_views=4)
    arb = C.arbiter(np.ones_like(masks), exts, ixts, scene, grid, min_views=4)
    n_und = int(arb["undecided"].sum())
    print(f"later_passes: {n_und} undecided of {arb['undecided'].size} voxels")
    assert n_und <= C.UNDECIDED_CAP * arb["undecided"].size
    lo, hi = int((arb["occ"][0] & ~arb["undecided"]).sum()), int((arb["occ"][0] | arb["undecided"]).sum())
    assert lo <= int(counts[0]) <= hi and lo > 0
    if n_und == 0:
        want, _, f = C.box_of(arb["occ"][0], scene, grid, 0.0)
        assert np.array_equal(bounds[0].cpu().numpy(), want) and int(flags[0]) == f


def test_two_labelled_layers_that_occlude_each_other():
    C.case_layers(_lib(), _dev())


def test_abstention_behind_outside_nan_and_fx0():
    C.case_abstention(_lib(), _dev())


def test_all_zero_masks_inside_a_buffer_of_ones():
    C.case_guard(_lib(), _dev())


def test_flags_and_pad():
    C.case_flags(_lib(), _dev())


def test_two_calls_give_identical_bits():
    C.case_determinism(_lib(), _dev())


def test_corners_feed_bounds_near_far_and_bounds_feed_layer_boxes():
    C.case_corners(_lib(), _dev())


def test_refusals_enqueue_nothing():
    C.case_refusals(_lib(), _dev())


def test_captured_graph_replayed_over_changed_masks():
    """ONE capture; the mask tensor's contents change in place between replays: the new masks' bounds, then the old masks' again.  A
    replay that inherited the previous one's accumulators would keep the union of both."""
    lib, dev = _lib(), _dev()
    exts, ixts = C.ring()
    old, new = C.two_time_frames(4, C.H, C.W, exts, ixts)
    scene, grid = np.array([[-1.0, -0.9, -0.8], [1.1, 0.8, 0.9]], np.float32), (21, 13, 17)
    kw = dict(min_views=4, max_miss=0, pad=0.01)
    want = {}
    for name, m in (("replay_a", old), ("replay_b", new)):
        want[name], _ = C.check(lib, dev, name, m, exts, ixts, scene, grid, **kw)
    assert not np.array_equal(want["replay_a"]["bounds"], want["replay_b"]["bounds"])
    t = lambda a: torch.from_numpy(a).to(dev)                              # noqa: E731
    masks, e, k = t(old.copy()), t(exts), t(ixts)
    out = (torch.zeros((1, 2, 3), device=dev), torch.zeros((1,), dtype=torch.int32, device=dev),
           torch.zeros((1,), dtype=torch.int32, device=dev), torch.zeros((1, 8, 3), device=dev))
    occ = torch.zeros(grid[::-1], dtype=torch.uint8, device=dev)
    ws = lib.vhull_workspace(1, dev)
    run = lambda: lib.vhull_bounds(masks, e, k, scene, grid=grid, out=out, occupancy=occ, workspace=ws, **kw)      # noqa: E731
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        run()
    for name, m in (("replay_b", new), ("replay_a", old), ("replay_b", new)):
        masks.copy_(t(m))
        graph.replay()
        torch.cuda.synchronize()
        w = want[name]
        for key, x in zip(("bounds", "counts", "flags", "corners", "occupancy"), out + (occ,)):
            assert x.cpu().numpy().tobytes() == w[key].tobytes(), (name, key)


@pytest.mark.parametrize("raw", [False, True], ids=["masks", "raw"])
def test_sequence_player_carves_each_time_frame(raw):
    dev = _dev()
    C.case_player(_lib(), dev, G._seeded_network(CFG, dev), CFG, raw)
    torch.cuda.synchronize()
