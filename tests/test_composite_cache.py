"""The composite network's source-view cache on the CPU lane emulator (tests/emu): the cases of composite_cache_cases.py.  The cached
frame must equal ``forward`` on the same views gathered by hand BIT FOR BIT, and what a GPU run cannot show — which kernels run and
where, the refusals' empty traces, an index outside the cache — is checked here.  test_composite_cache_gpu.py runs the value cases
on an MI355X, where the chains really overlap."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import composite_cache_cases as KC
import composite_driver_cases as DC


def _emu():
    from emu_lib import emu_lib
    return emu_lib(), torch.device("cpu")


@pytest.mark.parametrize("name", DC.RUN_CASES)
def test_build_is_one_call_per_net_whatever_the_chunk(name):
    KC.build_case(*_emu(), name)


@pytest.mark.parametrize("big", [False, True], ids=["small", "big"])
def test_indexed_prep_holds_the_plain_preps_bits(big):
    KC.indexed_prep_case(*_emu(), big)


@pytest.mark.parametrize("name", DC.RUN_CASES)
def test_cached_frame_equals_forward_on_hand_gathered_views(name):
    KC.frame_case(*_emu(), name)


def test_rebuild_in_place_stale_and_empty_caches():
    KC.rebuild_case(*_emu())


@pytest.mark.parametrize("name", DC.RUN_CASES)
def test_trace_no_feature_net_one_prep_two_gathers(name):
    KC.trace_case(*_emu(), name)


@pytest.mark.parametrize("which", list(KC.CACHE_REFUSALS))
def test_cache_refusals_name_the_field_and_enqueue_nothing(which):
    KC.cache_refusal_case(*_emu(), which)


def test_null_cache_index_and_args_are_refused():
    KC.null_refusals_case(*_emu())


@pytest.mark.parametrize("which", ["window outside", "small workspace"])
def test_frame_refusals_through_the_cached_entry(which):
    KC.frame_refusal_case(*_emu(), which)


@pytest.mark.parametrize("name", ["a", "b"])
def test_out_of_range_index_makes_every_output_nan_not_a_wild_read(name):
    KC.out_of_range_case(*_emu(), name)
