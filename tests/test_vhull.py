"""``enerf_vhull_bounds`` (the foreground's world-space box carved from the masks) on the CPU lane emulator, against the float64
arbiter of tests/vhull_cases.py, and the ``hull=`` wiring of the sequence player.  The GPU twins are in tests/test_vhull_gpu.py.

Worst undecided share measured: 0 of every case's voxels (the arbiter's own count, asserted per case; the GPU file's one larger grid has
10 of 599,040); every case prints its own."""
import numpy as np
import pytest
import torch

import __graft_entry__ as G
import vhull_cases as C
from emu_lib import emu_cu_count, emu_lib, emu_trace
from enerf_amd.config import EnerfConfig

DEV = "cpu"
CFG = EnerfConfig().with_cas(volume_planes=(8, 8), render_if=(False, True))


def test_ellipsoid_every_voxel_inside_the_shrunk_ellipsoid_is_occupied():
    C.case_ellipsoid(emu_lib(), DEV)


@pytest.mark.parametrize("name", sorted(C.GRID_SHAPES))
def test_grid_shapes(name):
    C.case_grid(emu_lib(), DEV, name)


def test_persistent_loop_makes_later_passes_under_two_cus():
    """70 x 5 x 9 is 90 runs of 23 blocks; two CUs cap the grid at 16 blocks, so waves take second runs — and the result is the one of
    the uncapped grid."""
    lib = emu_lib()
    masks, exts, ixts, scene, _ = C.ellipsoid_case()
    grid = (70, 5, 9)
    with emu_cu_count(lib, 2), emu_trace(lib) as trace:
        got, _ = C.check(lib, DEV, "grid_70x5x9_two_cus", masks, exts, ixts, scene, grid, min_views=3)
    launches = [t for t in trace if t[0] == "launch"]
    assert [t[1].split("<")[0].strip("(") for t in launches] == ["k_zero", "k_vhull_carve", "k_vhull_finish"]
    assert launches[1][2] == (16, 1, 1) and launches[2][2] == (1, 1, 1)
    wide = C.run(lib, DEV, masks, exts, ixts, scene, grid, min_views=3)
    for k in got:
        assert got[k].tobytes() == wide[k].tobytes(), k
    assert int(got["counts"][0]) > 0


def test_two_labelled_layers_that_occlude_each_other():
    C.case_layers(emu_lib(), DEV)


def test_abstention_behind_outside_nan_and_fx0():
    C.case_abstention(emu_lib(), DEV)


def test_no_read_outside_the_masks():
    C.case_guard(emu_lib(), DEV)


def test_flags_and_pad():
    C.case_flags(emu_lib(), DEV)


def test_two_calls_give_identical_bits():
    C.case_determinism(emu_lib(), DEV)


def test_corners_feed_bounds_near_far_and_bounds_feed_layer_boxes():
    C.case_corners(emu_lib(), DEV)


def test_refusals_enqueue_nothing():
    C.case_refusals(emu_lib(), DEV)


def test_the_early_exit_changes_the_work_never_the_result():
    """A voxel's loop over the views stops once its fate is sealed, so WHICH views it reads depends on their order; the result must
    not.  Five views (the fifth an all-ones mask through camera 0), forwards and backwards: at max_miss = 0 a voxel is sealed at its
    first outside vote, which comes early in one order and late in the other."""
    lib = emu_lib()
    masks, exts, ixts, scene, grid = C.ellipsoid_case()
    extra = np.concatenate([masks, np.full_like(masks[:1], 1)])
    e5, k5 = np.concatenate([exts, exts[:1]]), np.concatenate([ixts, ixts[:1]])
    got, arb = C.check(lib, DEV, "ellipsoid", extra, e5, k5, scene, grid, min_views=4, max_miss=0)
    first = C.run(lib, DEV, extra[::-1].copy(), e5[::-1].copy(), k5[::-1].copy(), scene, grid, min_views=4, max_miss=0)
    for k in got:                                                          # the order of the views never shows
        assert got[k].tobytes() == first[k].tobytes(), k


@pytest.mark.parametrize("raw", [False, True], ids=["masks", "raw"])
def test_sequence_player_carves_each_time_frame(raw):
    lib = emu_lib()
    C.case_player(lib, DEV, G._seeded_network(CFG, "cpu", lib=lib), CFG, raw)
