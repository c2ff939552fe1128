"""The composite network's kernels on an MI355X through the C ABI: the cases of composite_cases.py (test_composite.py runs them on
the emulator).

Worst errors measured on an MI355X (max|x - f64| / max|f64|): see README, "Composite network"."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import composite_cases as CC

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]
WORST = {}


def _gpu():
    from enerf_amd.lib import get_lib
    return get_lib(), torch.device("cuda:0")


@pytest.mark.parametrize("C", [32, 16])
def test_window_volume_is_the_crop_on_gpu(C):
    CC.window_volume_case(*_gpu(), C)


@pytest.mark.parametrize("depth_inv", [False, True])
@pytest.mark.parametrize("D", [8, 32])
def test_window_regression_is_the_padded_regression_on_gpu(D, depth_inv):
    CC.window_regression_case(*_gpu(), D, depth_inv)


@pytest.mark.parametrize("ns", [1, 2])
@pytest.mark.parametrize("S", [2, 3, 4])
@pytest.mark.parametrize("level", [0, 1])
def test_raw_render_matches_float64_on_gpu(level, S, ns):
    CC.raw_render_case(*_gpu(), True, level, S, ns, WORST)
    print(f"[composite] worst so far: {WORST}")


@pytest.mark.parametrize("level", [0, 1])
def test_raw_render_window_selection_on_gpu(level):
    CC.raw_selection_case(*_gpu(), True, level)


@pytest.mark.parametrize("level", [0, 1])
def test_raw_render_tile_deal_on_gpu(level):
    CC.raw_tile_walk_case(*_gpu(), True, level)


@pytest.mark.parametrize("L,name,ns", CC.COMPOSITE_CASES)
def test_layer_composite_matches_float64_on_gpu(L, name, ns):
    CC.composite_case(*_gpu(), L, name, ns, WORST)
    print(f"[composite] worst so far: {WORST}")


def test_composite_refusals_on_gpu():
    CC.composite_refusals(*_gpu())


def test_window_entry_refusals_on_gpu():
    CC.window_refusals(*_gpu())


@pytest.mark.parametrize("name", list(CC.NETWORK_CASES))
def test_network_matches_reference_on_gpu(name):
    """Every output and every regressed depth / std map of both fixtures within 1e-4; strict state-dict load; training mode raises;
    weight rows sum to less than 1; outside every box the image is the background's own composite."""
    CC.network_case(*_gpu(), name, WORST)
    print(f"[composite] worst so far: {WORST}")
