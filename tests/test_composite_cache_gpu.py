"""The composite network's source-view cache on an MI355X: the value cases of composite_cache_cases.py (test_composite_cache.py runs
them, the trace properties and the refusals on the emulator).  Here the forked chains really overlap: three cached frames in a row
with the lane on, alternating two index rows, must each equal ``forward`` on the views gathered by hand — the only check that sees
a scratch region shared across the fork.  No test here sends an index outside the cache."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import composite_cache_cases as KC
import composite_driver_cases as DC

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]


def _gpu():
    from enerf_amd.lib import get_lib
    return get_lib(), torch.device("cuda:0")


@pytest.mark.parametrize("name", DC.RUN_CASES)
def test_build_is_one_call_per_net_whatever_the_chunk_on_gpu(name):
    KC.build_case(*_gpu(), name)


@pytest.mark.parametrize("big", [False, True], ids=["small", "big"])
def test_indexed_prep_holds_the_plain_preps_bits_on_gpu(big):
    KC.indexed_prep_case(*_gpu(), big)


@pytest.mark.parametrize("name", DC.RUN_CASES)
def test_cached_frame_equals_forward_three_frames_in_a_row_on_gpu(name):
    KC.frame_case(*_gpu(), name, frames=3)


def test_rebuild_in_place_stale_and_empty_caches_on_gpu():
    KC.rebuild_case(*_gpu())


@pytest.mark.parametrize("name", ["b", "a"])
def test_graphed_select_views_and_cached_frame_replays_equal_eager(name):
    KC.graph_case(*_gpu(), name)


def test_build_selection_and_cached_frame_do_not_synchronise():
    KC.no_sync_case(*_gpu())


def test_uint8_build_equals_the_float_build_of_the_ingested_images():
    KC.uint8_case(*_gpu())
