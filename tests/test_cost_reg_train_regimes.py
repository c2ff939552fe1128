"""The training-mode cost-volume networks (autograd.cost_reg_train: _Block, _BatchNormTrain, the train.hip BatchNorm entries and
enerf_conv3d_layer in its forward and input-gradient roles, the fused 8 -> 16 heads between slice_channels / concat_channels) and
the BatchNorm block alone, against float64, at the sizes a window of the composite network's training step can have: volumes that
are no multiple of a conv box, one box row or column, B = 2, and position counts ragged against the channel kernels' steps.

Reference: tests/torch_twins.py::cost_reg_forward on a deep copy of the same CostRegParams (A) / nn.BatchNorm1d (B) in float64,
``.train()`` mode, under autograd.  Yardstick: the same in fp32 on the CPU.  Per tensor e = max|x - f64| / max|f64| and
    e_hip <= max(TAU, 3 e_ref)                                      (the rule of test_feature_net_sizes.py),
with num_batches_tracked equal.  TAU is five times the worst e_ref of the family, rounded up to one digit; it is measured from
the two references, never from the kernels.

A. The stage at cost_reg_train_cases.STAGE_SHAPES: feat, prob, d vol, every parameter gradient, every running statistic.  Each case
   also asserts e_ref <= 1e-5, so an ill-conditioned case cannot hide behind 3 e_ref (with 2 positions at the deepest level the
   fp32 twin is 6e-4 from float64: such a shape is not in the list).  On the first Min and the first full shape also: only prob
   with an upstream gradient (the composite step; feat_conv.weight's gradient is exactly zero), a second backward through the same
   graph (deferred weight-gradient reductions: the same bits), the conv routes the sizes do not pick themselves
   (Options(conv3d_lds_min_voxels=1), Options(conv3d_global_only=1); the emulator entries read the launch trace: forward and
   backward together 8 k_conv3d_s1_lds, 2 k_conv3d_s2_lds and 4 k_conv3d_t2_all launches under the first, nothing but k_conv3d —
   not the default's k_conv3d_wl either — under the second), and two sensitivity checks on the reference alone: the
   float64 twin with (a) the skip share of d c2 dropped, (b) the last voxel left out of every layer's batch statistics must move a
   compared tensor by more than 10 bounds (measured: (a) 38775 / 37642 bounds, gradients only; (b) 28919 / 27266 bounds).

B. _BatchNormTrain forward + backward on z (n, C) = sigma randn + mu: C in {8, 16, 32, 64}, n in {2, 60, 777, 4099} (ragged against
   256 / (C/4) positions x 4 per step; 2 is the smallest count torch accepts), (ReLU, residual) in all four combinations, momentum
   0.1 and None (cumulative average) over three consecutive batches, mu / sigma in {0, 1, 30} through three forms: the fused one
   _BatchNormTrain picks, the three-launch entries (bn_train_stats / bn_train_bwd_stats + channel_affine), and the coefficient
   entries with the position count as a one-element float64 device tensor (SyncBatchNorm's path without a process group).
   y, dz, dgamma, dbeta, running_mean, running_var, num_batches_tracked.  Under a ReLU, the elements whose float64 pre-activation
   is within 64 roundings of zero (in units of its two terms) get a zero upstream gradient on every side: an fp32 evaluation may
   take the other side of the gate there (one such element moved torch's own fp32 dz by 0.12 of its maximum); at most
   max(2, 1e-3 of the elements) may be such, which the case generator asserts.
   The cases differ in conditioning by design, so TAU is derived per class (n == 2, mu / sigma), each five times the worst e_ref
   of its own class — every one at or below what one TAU over the whole family (3e-3) would be:
     * the kernels normalise as z scale + shift and g scale + z k2 + k3 with fp32 coefficients, torch as (z - mean) invstd with an
       fp32 mean: either way the error is |mean| invstd 2^-24 of the output's unit, which is why mu / sigma = 30 has its own class;
     * at n = 2 a channel's two values may lie close together (std << |z| by chance, whatever mu is): y is then ill-conditioned in
       fp32 for torch and the kernels alike (e_ref up to 3e-4 at mu / sigma = 30, where n >= 60 has 3e-6), and the kernels'
       uncentred z k2 + k3 loses more of dz than torch's centred form does.  With the TAU of the n >= 60 class three n = 2 cases
       miss on the emulator (y 9.8e-5 and 2.6e-4 against 3 e_ref = 5.3e-5 and 1.9e-4; dz 8.9e-6 against 6e-6): no kernel is wrong
       there, the class is.  A level that small does not train anything (the guard refuses 1 position; the stage's own shapes
       keep >= 12).
     * dz at n = 2 is analytically eps / (var + eps) of its terms (two normalised values are +-1 whatever z is), so max|f64| of dz
       is ~1e-5 of what is summed and every fp32 evaluation is far from it in those units: dz at n = 2 is measured against the
       magnitude of its terms, max|g| max|gamma invstd| (the ``natural`` scale of backward_cases.scales), e_ref and e_hip alike.

Measured (the references on the CPU of the machine the emulator ran on; e_hip over all three forms):
    family                      worst e_ref (where)                                              TAU    worst e_hip emulator | MI355X
    stage                       2.24e-6 (grad conv3.bn.weight, (16, True, 2, 8, 16, 24))         2e-5   3.3e-6 | 2.7e-6  (both: lds route)
    BatchNorm n >= 60, mu/s 0   1.01e-6 (dbeta, C = 8, n = 4099)                                 6e-6   2.2e-7 | 2.2e-7
    BatchNorm n >= 60, mu/s 1   1.02e-6 (dbeta, C = 8, n = 4099)                                 6e-6   1.8e-7 | 1.5e-7
    BatchNorm n >= 60, mu/s 30  1.07e-5 (dgamma, C = 16, n = 4099)                               6e-5   1.3e-6 | 8.9e-7
    BatchNorm n = 2, mu/s 0     1.19e-5 (y, C = 64)                                              6e-5   2.9e-5 | 8.6e-6
    BatchNorm n = 2, mu/s 1     1.16e-5 (y, C = 64)                                              6e-5   2.2e-5 | 1.2e-5
    BatchNorm n = 2, mu/s 30    4.11e-4 (dgamma, C = 32)                                         3e-3   3.4e-4 | 2.3e-4
No kernel had to change.  The guard (autograd.check_cost_reg_train_shape) is host code: its tests run on the emulator only and
assert through the launch trace that a refused shape launches nothing.
Run time: about 2 minutes for the CPU entries (the longest single one 12 s); the MI355X entries take 6 s together.
"""
import functools
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import cost_reg_train_cases as K          # noqa: E402
import torch_twins as T                   # noqa: E402
from enerf_amd.lib import Options         # noqa: E402

TAU_STAGE = 2e-5
TAU_BN = {(False, 0.0): 6e-6, (False, 1.0): 6e-6, (False, 30.0): 6e-5,         # (n == 2, mu / sigma): one per conditioning class
          (True, 0.0): 6e-5, (True, 1.0): 6e-5, (True, 30.0): 3e-3}
E_REF_CAP = 1e-5
WORST = {}
ROUTES = {"lds": dict(conv3d_lds_min_voxels=1), "global": dict(conv3d_global_only=1)}


def _emu():
    from emu_lib import emu_lib
    return emu_lib(), torch.device("cpu")


def _gpu():
    from enerf_amd.lib import get_lib
    return get_lib(), torch.device("cuda:0")


def _note(family, kind, value, where):
    w = WORST.setdefault(family, {"e_ref": (0.0, ""), "e_hip": (0.0, "")})
    if value > w[kind][0]:
        w[kind] = (value, where)


def _report(family):
    w = WORST[family]
    print(f"[{family}] worst so far: e_ref {w['e_ref'][0]:.2e} ({w['e_ref'][1]}) e_hip {w['e_hip'][0]:.2e} ({w['e_hip'][1]})")


def _bound(tau, e_ref):
    return max(tau, 3.0 * e_ref)


# ---- A. the whole stage ---------------------------------------------------------------------------------------------------------
def _compare_stage(tag, got, nbt, r64, e_ref, want_nbt, skip=()):
    """Print every tensor's line, then assert the bound of each."""
    assert set(r64) - set(skip) <= set(got), (tag, sorted(set(r64) - set(got)))
    assert nbt == want_nbt, (tag, nbt, want_nbt)
    errs = {}
    for k, r in r64.items():
        if k in skip:
            continue
        assert got[k].shape == r.shape, (tag, k, got[k].shape, r.shape)
        errs[k] = K.rel(got[k], r)
        _note("stage", "e_ref", e_ref[k], f"{k}, {tag}")
        _note("stage", "e_hip", errs[k], f"{k}, {tag}")
    kw, kr = max(errs, key=errs.get), max(e_ref, key=e_ref.get)
    print(f"[stage] {tag}: {len(errs)} tensors; worst e_hip {errs[kw]:.2e} ({kw}, e_ref {e_ref[kw]:.2e}); worst e_ref {e_ref[kr]:.2e} ({kr}); "
          + "; ".join(f"{k} e_hip {errs[k]:.1e} e_ref {e_ref[k]:.1e}" for k in ("feat", "prob", "d vol") if k in errs))
    for k, e in errs.items():
        assert e_ref[k] <= E_REF_CAP, f"{tag}: {k} is ill-conditioned in the reference itself: e_ref {e_ref[k]:.3e} > {E_REF_CAP:.0e}"
        assert e <= _bound(TAU_STAGE, e_ref[k]), f"{tag}: {k} e_hip {e:.3e} > max({TAU_STAGE:.0e}, 3 x e_ref {e_ref[k]:.3e})"
    return errs


def _stage_case(gpu, shape):
    lib, dev = _gpu() if gpu else _emu()
    r64, e_ref, want_nbt = K.stage_reference(shape)
    got, nbt, _ = K.stage_hip(lib, dev, shape)
    _compare_stage(f"{shape}", got, nbt, r64, e_ref, want_nbt)
    _report("stage")


def _stage_route_case(gpu, shape, route):
    lib, dev = _gpu() if gpu else _emu()
    r64, e_ref, want_nbt = K.stage_reference(shape)
    if gpu:
        got, nbt, _ = K.stage_hip(lib, dev, shape, options=Options(**ROUTES[route]))
    else:               # the options reach every layer: read off the launch trace (forward, heads and input-gradient layers)
        from emu_lib import emu_trace
        with emu_trace(lib) as rows:
            got, nbt, _ = K.stage_hip(lib, dev, shape, options=Options(**ROUTES[route]))
        convs = [r[1] for r in rows if r[0] == "launch" and "k_conv3d" in r[1] and "pack" not in r[1]]
        count = lambda name: sum(name in k for k in convs)
        assert len(convs) == 2 * (11 if shape[1] else 8), (shape, route, convs)
        if route == "lds":      # forward and backward: conv0 / conv2 / conv4 / heads (and their dgrads), conv1 + d conv11, conv9 / conv11 + d conv1 / d conv3
            assert (count("k_conv3d_s1_lds<"), count("k_conv3d_s2_lds<"), count("k_conv3d_t2_all<")) == (8, 2, 4), (shape, convs)
        else:                   # nothing but the global-load kernel, the deep levels' k_conv3d_wl of the default route included
            assert count("k_conv3d<") == len(convs), (shape, convs)
    _compare_stage(f"{shape} {route}", got, nbt, r64, e_ref, want_nbt)
    _report("stage")


def _stage_prob_only_case(gpu, shape):
    """Only prob has an upstream gradient (train_path_composite.py drops feat); and a second backward of the same graph."""
    lib, dev = _gpu() if gpu else _emu()
    r64, e_ref, want_nbt = K.stage_reference(shape, True)
    assert "grad feat_conv.0.weight" not in r64 and "grad depth_conv.0.weight" in r64
    got, nbt, second = K.stage_hip(lib, dev, shape, prob_only=True, twice=True)
    assert float(got["grad feat_conv.0.weight"].abs().max()) == 0.0
    _compare_stage(f"{shape} prob only", got, nbt, r64, e_ref, want_nbt)
    for k, t in second.items():
        assert torch.equal(t, got[k]), (shape, k, "the second backward differs")
    # both upstream gradients, twice as well
    got, _, second = K.stage_hip(lib, dev, shape, twice=True)
    for k, t in second.items():
        assert torch.equal(t, got[k]), (shape, k, "the second backward differs")
    _report("stage")


def _stage_sensitivity(shape):
    """On the reference alone: a defective float64 twin must leave the true one by more than 10 bounds in some compared tensor."""
    r64, e_ref, _ = K.stage_reference(shape)
    sound, _ = K.stage_twin(shape, torch.float64, forward=K._defective_forward, stats=False)
    for k in sound:                       # the restated forward without a defect is the twin itself
        assert K.rel(sound[k], r64[k]) <= 1e-12, (k, K.rel(sound[k], r64[k]))
    for what, kw in (("(a) the skip share of d c2 dropped", dict(detach_skip=True)), ("(b) the last voxel outside the batch statistics", dict(drop_last=True))):
        bad, _ = K.stage_twin(shape, torch.float64, forward=functools.partial(K._defective_forward, **kw), stats=False)
        moved = {k: K.rel(bad[k], r64[k]) / _bound(TAU_STAGE, e_ref[k]) for k in bad}
        top = max(moved, key=moved.get)
        print(f"[stage] {shape} sensitivity {what}: moves {top} by {moved[top]:.0f} bounds ({sum(v > 10 for v in moved.values())} of {len(moved)} "
              f"tensors by more than 10)")
        assert moved[top] > 10, (shape, what, top, moved[top])
        if "detach_skip" in kw:          # the forward is untouched: only gradients may move
            assert moved["feat"] == 0.0 and moved["prob"] == 0.0


# ---- B. the BatchNorm block alone -----------------------------------------------------------------------------------------------
def _bn_scale(k, n, inputs, start, r64):
    """None = max|f64|; dz at n = 2: the magnitude of its terms (module docstring)."""
    if k != "dz" or n != 2:
        return None
    z, _, g = inputs
    invstd = 1.0 / torch.sqrt(z.double().var(0, unbiased=False) + start.eps)
    return float(g.abs().max()) * float((start.weight.detach().double().abs() * invstd).max())


def _bn_case(gpu, C, n):
    import copy
    lib, dev = _gpu() if gpu else _emu()
    forms = K.bn_forms(lib)
    for ratio in K.BN_RATIOS:
        for relu, res in K.BN_VARIANTS:
            for momentum, batches in K.BN_MOMENTA:
                start, steps = K.bn_reference(C, n, ratio, relu, res, momentum, batches)
                worst = {}
                for form, run in forms.items():
                    bn = copy.deepcopy(start).to(dev)
                    for it, (inputs, r64, e_ref, want_nbt) in enumerate(steps):
                        z, r, g = (None if t is None else t.to(dev) for t in inputs)
                        y, dz, dgamma, dbeta = run(bn, relu, z, r, g)
                        got = {"y": y, "dz": dz, "dgamma": dgamma, "dbeta": dbeta, "running_mean": bn.running_mean, "running_var": bn.running_var}
                        assert int(bn.num_batches_tracked) == want_nbt == it + 1, (form, it)
                        for k, ref in r64.items():
                            tag = f"C={C} n={n} mu/sigma={ratio:g} relu={int(relu)} res={int(res)} momentum={momentum} batch {it}"
                            assert got[k].shape == ref.shape, (tag, form, k)
                            e_hip, e_r = K.rel(got[k], ref), e_ref[k]
                            natural = _bn_scale(k, n, inputs, start, ref)
                            if natural is not None:
                                unit = max(float(ref.abs().max()), 1e-300) / natural
                                e_hip, e_r = e_hip * unit, e_r * unit
                            fam = f"bn {ratio:g}" + (" n=2" if n == 2 else "")
                            _note(fam, "e_ref", e_r, f"{k}, {tag}")
                            _note(fam, "e_hip", e_hip, f"{k}, {form}, {tag}")
                            worst[k] = max(worst.get(k, (0.0, 0.0)), (e_hip, e_r))
                            tau = TAU_BN[n == 2, ratio]
                            assert e_hip <= _bound(tau, e_r), f"{tag} {form}: {k} e_hip {e_hip:.3e} > max({tau:.0e}, 3 x e_ref {e_r:.3e})"
                print(f"[bn] C={C} n={n} mu/sigma={ratio:g} relu={int(relu)} res={int(res)} momentum={momentum}: "
                      + "; ".join(f"{k} e_hip {v[0]:.1e} e_ref {v[1]:.1e}" for k, v in worst.items()))
    for ratio in K.BN_RATIOS:
        _report(f"bn {ratio:g}" + (" n=2" if n == 2 else ""))


# ---- 2. the guard (host code: the same on both libraries) -----------------------------------------------------------------------
def _refusal(shape):
    return "Expected more than 1 value per channel when training" if shape == (32, False, 1, 4, 4, 4) else "divisible"


@pytest.mark.parametrize("shape", K.REFUSED_SHAPES)
def test_cost_reg_train_refuses_sizes_its_levels_cannot_halve_before_any_launch(shape):
    from emu_lib import emu_trace
    from enerf_amd.autograd import cost_reg_train
    lib, _ = _emu()
    cin, full, B, D, h, w = shape
    m = K.stage_module(cin, full)
    vol = torch.zeros(B, cin, D, h, w, requires_grad=True)
    with emu_trace(lib) as trace:
        with pytest.raises(ValueError, match=_refusal(shape)):
            cost_reg_train(lib, m, vol)
    assert not [t for t in trace if t[0] == "launch"], trace
    assert all(int(b) == 0 for n, b in m.named_buffers() if n.endswith("num_batches_tracked"))


@pytest.mark.parametrize("shape", K.REFUSED_SHAPES)
def test_float64_twin_raises_on_the_refused_sizes(shape):
    import copy
    cin, full, B, D, h, w = shape
    m64 = copy.deepcopy(K.stage_module(cin, full)).double().train()
    with pytest.raises((RuntimeError, ValueError), match="must match the size|Expected more than 1 value per channel"):
        T.cost_reg_forward(m64, torch.zeros(B, cin, D, h, w, dtype=torch.float64))


def test_composite_training_step_names_the_window_it_refuses():
    """A box whose level-0 window is 10 voxels wide (int(bbox * 0.125): any size): the step refuses it by layer and window, in the
    training blocks' words, before the window's volume is built."""
    import numpy as np
    import composite_train_cases as TC
    from enerf_amd.network_composite import _scaled_box
    from enerf_amd.synth import make_batch
    lib, dev = _emu()
    name, H, W = "t", 32, 96
    cfg = TC.train_config(name)
    scale = cfg.cas.volume_scale[0]
    box = next((0, 0, bw, H) for bw in range(4, W + 1) if _scaled_box((0, 0, bw, H), scale)[2] == 10)
    win = _scaled_box(box, scale)
    assert win[2] == 10 and win[3] % 4 == 0 and cfg.cas.volume_planes[0] % 4 == 0          # the width alone is at fault
    b = make_batch(H, W, 3, cfg, seed=24, textured=True)
    near, far = float(b["near_far"][0, 0]), float(b["near_far"][0, 1])
    b["near_far"] = np.array([[(near + 0.2 * (far - near), near + 0.7 * (far - near)), (near, far)]], np.float32)
    b["bbox"] = np.array([[box]], np.float32)
    b["bg_src_inps"] = np.random.default_rng(124).uniform(-1, 1, size=b["src_inps"].shape).astype(np.float32)
    batch = {k: torch.from_numpy(v).to(dev) for k, v in b.items()}
    net = TC.train_network(lib, dev, name)
    with pytest.raises(ValueError, match="divisible") as info:
        net(batch)
    msg = str(info.value)
    assert "cost_reg_0_layer0" in msg and str(tuple(win)) in msg, msg


# ---- emulator -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", K.STAGE_SHAPES)
def test_cost_reg_train_stage_emulated(shape):
    _stage_case(False, shape)


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("shape", [K.FIRST_MIN, K.FIRST_FULL])
def test_cost_reg_train_stage_forced_conv_routes_emulated(shape, route):
    _stage_route_case(False, shape, route)


@pytest.mark.parametrize("shape", [K.FIRST_MIN, K.FIRST_FULL])
def test_cost_reg_train_stage_prob_only_and_second_backward_emulated(shape):
    _stage_prob_only_case(False, shape)


@pytest.mark.parametrize("shape", [K.FIRST_MIN, K.FIRST_FULL])
def test_cost_reg_train_stage_reference_is_sensitive_to_a_dropped_skip_gradient_and_a_dropped_voxel(shape):
    _stage_sensitivity(shape)


@pytest.mark.parametrize("n", K.BN_COUNTS)
@pytest.mark.parametrize("C", K.BN_CHANNELS)
def test_batchnorm_train_block_emulated(C, n):
    _bn_case(False, C, n)


# ---- MI355X ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")
@pytest.mark.parametrize("shape", K.STAGE_SHAPES)
def test_cost_reg_train_stage_on_gpu(shape):
    _stage_case(True, shape)


@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("shape", [K.FIRST_MIN, K.FIRST_FULL])
def test_cost_reg_train_stage_forced_conv_routes_on_gpu(shape, route):
    _stage_route_case(True, shape, route)


@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")
@pytest.mark.parametrize("shape", [K.FIRST_MIN, K.FIRST_FULL])
def test_cost_reg_train_stage_prob_only_and_second_backward_on_gpu(shape):
    _stage_prob_only_case(True, shape)


@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")
@pytest.mark.parametrize("n", K.BN_COUNTS)
@pytest.mark.parametrize("C", K.BN_CHANNELS)
def test_batchnorm_train_block_on_gpu(C, n):
    _bn_case(True, C, n)
