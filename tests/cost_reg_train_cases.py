"""Helper of tests/test_cost_reg_train_regimes.py: the modules, inputs and CPU references of the training-mode cost-reg stage and of
the BatchNorm block alone, the defective float64 references of the sensitivity checks, and the comparison every check shares.

Per tensor e = max|x - f64| / max|f64|; ``e_ref`` is that of the same torch code in fp32 on the CPU and ``e_hip`` that of the
kernels.  A reference is computed once per case (CPU) and shared by the emulator and the MI355X tests; nothing writes to it.
"""
import copy
import functools

import torch
import torch.nn.functional as F

import torch_twins as T
from enerf_amd.network import CostRegParams

# (in_channels, full, B, D, h, w)
STAGE_SHAPES = [(32, False, 1, 8, 12, 20), (32, False, 2, 8, 8, 12), (32, False, 1, 8, 4, 36), (16, False, 1, 8, 36, 4),
                (16, False, 1, 8, 20, 28), (16, True, 1, 8, 24, 40), (16, True, 2, 8, 16, 24)]
FIRST_MIN, FIRST_FULL = STAGE_SHAPES[0], STAGE_SHAPES[5]
REFUSED_SHAPES = [(32, False, 1, 8, 10, 12), (16, True, 1, 8, 12, 16), (32, False, 1, 6, 8, 8), (32, False, 1, 4, 4, 4)]

BN_CHANNELS = (8, 16, 32, 64)
BN_COUNTS = (2, 60, 777, 4099)
BN_RATIOS = (0.0, 1.0, 30.0)                 # |mean| / std of the normalised tensor
BN_SIGMA = 2.0
BN_NEAR = 64 * 2.0 ** -24                    # backward_cases.NEAR
BN_VARIANTS = ((False, False), (False, True), (True, False), (True, True))      # (relu, residual)
BN_MOMENTA = ((0.1, 1), (None, 3))           # (momentum, consecutive batches through one module)


def rel(x, r64):
    return float((x.detach().cpu().double() - r64).abs().max()) / max(float(r64.abs().max()), 1e-300)


# ---- A. the whole stage ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stage_module(cin, full):
    """A ``CostRegParams`` with seeded random weights, BatchNorm gamma in [0.5, 1.5] and beta ~ N(0, 0.1), in training mode (fp32, CPU)."""
    with torch.random.fork_rng():
        torch.manual_seed(7100 + cin + int(full))
        m = CostRegParams(cin, full)
        with torch.no_grad():
            for mod in m.modules():
                if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm):
                    mod.weight.uniform_(0.5, 1.5)
                    mod.bias.normal_(0.0, 0.1)
    return m.train()


@functools.lru_cache(maxsize=None)
def stage_inputs(shape):
    cin, full, B, D, h, w = shape
    g = torch.Generator().manual_seed(7200 + sum(p * v for p, v in zip((1, 3, 5, 7, 11, 13), map(int, shape))))
    return (torch.randn(B, cin, D, h, w, generator=g), torch.randn(B, 8, D, h, w, generator=g), torch.randn(B, D, h, w, generator=g))


def _bn_without_last(bn, z):
    """Defect (b): training-mode BatchNorm whose batch statistics leave out the last voxel (the running statistics are not compared)."""
    C = z.shape[1]
    flat = z.transpose(0, 1).reshape(C, -1)[:, :-1]
    shape = (1, C) + (1,) * (z.dim() - 2)
    mean, var = flat.mean(1), flat.var(1, unbiased=False)
    return (z - mean.view(shape)) / torch.sqrt(var.view(shape) + bn.eps) * bn.weight.view(shape) + bn.bias.view(shape)


def _defective_forward(m, x, detach_skip=False, drop_last=False):
    """torch_twins.cost_reg_forward with one defect: (a) ``detach_skip``: c2's skip share of the gradient is dropped; (b) ``drop_last``."""
    norm = (lambda bn, t: _bn_without_last(bn, t)) if drop_last else (lambda bn, t: bn(t))
    cbr = lambda blk, t: F.relu(norm(blk.bn, blk.conv(t)))
    up = lambda seq, t: norm(seq[1], seq[0](t))
    c0 = cbr(m.conv0, x)
    c2 = cbr(m.conv2, cbr(m.conv1, c0))
    c4 = cbr(m.conv4, cbr(m.conv3, c2))
    y = c4
    if m.full:
        y = c4 + up(m.conv7, cbr(m.conv6, cbr(m.conv5, c4)))
    y = (c2.detach() if detach_skip else c2) + up(m.conv9, y)
    y = c0 + up(m.conv11, y)
    return m.feat_conv[0](y), m.depth_conv[0](y).squeeze(1)


def collect(m, vol, feat, prob, stats=True):
    """Every compared tensor of one forward + backward, by name."""
    out = {"feat": feat.detach(), "prob": prob.detach(), "d vol": vol.grad}
    for n, p in m.named_parameters():
        if p.grad is not None:
            out["grad " + n] = p.grad
    if stats:
        for n, b in m.named_buffers():
            if n.endswith(("running_mean", "running_var")):
                out["stat " + n] = b.detach().clone()
    return out


def tracked(m):
    return {n: int(b) for n, b in m.named_buffers() if n.endswith("num_batches_tracked")}


def stage_twin(shape, dtype, prob_only=False, forward=T.cost_reg_forward, stats=True):
    cin, full = shape[:2]
    m = copy.deepcopy(stage_module(cin, full)).to(dtype).train()
    vol, g_feat, g_prob = stage_inputs(shape)
    x = vol.to(dtype).clone().requires_grad_(True)
    feat, prob = forward(m, x)
    if prob_only:
        prob.backward(g_prob.to(dtype))
    else:
        torch.autograd.backward([feat, prob], [g_feat.to(dtype), g_prob.to(dtype)])
    return collect(m, x, feat, prob, stats), tracked(m)


@functools.lru_cache(maxsize=None)
def stage_reference(shape, prob_only=False):
    """(float64 tensors, e_ref per tensor, num_batches_tracked) of one stage case."""
    r64, nbt = stage_twin(shape, torch.float64, prob_only)
    r32, nbt32 = stage_twin(shape, torch.float32, prob_only)
    assert nbt == nbt32 and set(r64) == set(r32)
    return r64, {k: rel(r32[k], r64[k]) for k in r64}, nbt


def stage_hip(lib, dev, shape, prob_only=False, options=None, twice=False):
    """The same forward + backward on the kernels.  ``twice``: also a second backward through the same graph -> (tensors, nbt, second)."""
    from enerf_amd.autograd import cost_reg_train
    cin, full = shape[:2]
    m = copy.deepcopy(stage_module(cin, full)).to(dev).train()
    vol, g_feat, g_prob = (t.to(dev) for t in stage_inputs(shape))
    x = vol.clone().requires_grad_(True)
    feat, prob = cost_reg_train(lib, m, x, options=options)
    outs, ups = ([prob], [g_prob]) if prob_only else ([feat, prob], [g_feat, g_prob])
    torch.autograd.backward(outs, ups, retain_graph=twice)
    got = collect(m, x, feat, prob)
    second = None
    if twice:
        leaves = [x] + [p for _, p in m.named_parameters()]
        second = dict(zip(["d vol"] + ["grad " + n for n, _ in m.named_parameters()], torch.autograd.grad(outs, leaves, ups)))
    return got, tracked(m), second


# ---- B. the BatchNorm block alone -----------------------------------------------------------------------------------------------
def bn_module(C, momentum, seed):
    with torch.random.fork_rng():
        torch.manual_seed(seed)
        bn = torch.nn.BatchNorm1d(C, momentum=momentum).train()
        with torch.no_grad():
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.normal_(0.0, 0.5)
    return bn


@functools.lru_cache(maxsize=None)
def bn_reference(C, n, ratio, relu, res, momentum, batches):
    """Per consecutive batch: the inputs (z, residual or None, g), the float64 results and e_ref per tensor; the module as it started."""
    seed = 7300 + C + 7 * n + int(ratio) + 2 * int(relu) + int(res) + (0 if momentum is None else 50)
    start = bn_module(C, momentum, seed)
    m32, m64 = copy.deepcopy(start), copy.deepcopy(start).double()
    g_ = torch.Generator().manual_seed(seed)
    steps = []
    for _ in range(batches):
        z = BN_SIGMA * torch.randn(n, C, generator=g_) + ratio * BN_SIGMA
        r = torch.randn(n, C, generator=g_) if res else None
        g = torch.randn(n, C, generator=g_)
        if relu:
            # rounding-decided gates (backward_cases.py's rule): where the float64 pre-activation z scale + shift is within NEAR of zero
            # in units of its two terms, an fp32 evaluation may take the other side of the ReLU; those elements get a zero upstream
            # gradient on every side, and only a few may be such
            with torch.no_grad():
                zd = z.double()
                invstd = 1.0 / torch.sqrt(zd.var(0, unbiased=False) + m64.eps)
                scale = m64.weight * invstd
                shift = m64.bias - zd.mean(0) * scale
                near = (zd * scale + shift).abs() <= BN_NEAR * ((zd * scale).abs() + shift.abs())
            assert int(near.sum()) <= max(2, 1e-3 * near.numel()), (C, n, ratio, int(near.sum()))
            g = g * ~near
        both = []
        for m, dt in ((m64, torch.float64), (m32, torch.float32)):
            m.zero_grad()
            zl = z.to(dt).clone().requires_grad_(True)
            y = m(zl)
            y = torch.relu(y) if relu else y
            y = y + r.to(dt) if res else y
            y.backward(g.to(dt))
            both.append({"y": y.detach(), "dz": zl.grad, "dgamma": m.weight.grad.clone(), "dbeta": m.bias.grad.clone(),
                         "running_mean": m.running_mean.clone(), "running_var": m.running_var.clone()})
        assert int(m64.num_batches_tracked) == int(m32.num_batches_tracked)
        steps.append(((z, r, g), both[0], {k: rel(both[1][k], both[0][k]) for k in both[0]}, int(m64.num_batches_tracked)))
    return start, steps


def bn_forms(lib):
    """name -> f(bn, relu, z, residual, g) -> (y, dz, dgamma, dbeta): the three ways the library runs one BatchNorm direction pair."""
    from enerf_amd.autograd import _BatchNormTrain

    def fused(bn, relu, z, r, g):
        blk = _BatchNormTrain(lib, bn, relu)
        y = blk.forward(z, residual=r)
        assert blk.fused
        return (y,) + tuple(blk.backward(g))

    def mask_of(relu, z, ss):
        return dict(z_mask=z, mask_scale=ss[0], mask_shift=ss[1]) if relu else {}

    def three_launch(bn, relu, z, r, g):            # as test_training.py::_check_bn_two_launch_form calls them
        mi, ss, cnt = lib.bn_train_stats(z, bn)
        assert cnt == z.shape[0]
        y = lib.channel_affine(z, ss[0], ss[1], residual=r, relu=relu)
        mask = mask_of(relu, z, ss)
        dgb, k23 = lib.bn_train_bwd_stats(g, z, mi, ss[0], **mask)
        return y, lib.channel_affine(g, ss[0], k23[1], b=z, q=k23[0], **mask), dgb[0], dgb[1]

    def count_on_device(bn, relu, z, r, g):         # SyncBatchNorm's path without a process group: local == global sums
        cnt = torch.full((1,), float(z.shape[0]), dtype=torch.float64, device=z.device)
        mi, ss = lib.bn_train_coeffs(lib.channel_sums_raw(z, z), cnt, bn)
        y = lib.channel_affine(z, ss[0], ss[1], residual=r, relu=relu)
        mask = mask_of(relu, z, ss)
        local = lib.channel_sums_raw(g, z, **mask)
        dgb, k23 = lib.bn_train_bwd_coeffs(local, local, cnt, mi, ss[0])
        return y, lib.channel_affine(g, ss[0], k23[1], b=z, q=k23[0], **mask), dgb[0], dgb[1]
    return {"fused": fused, "three-launch": three_launch, "count-on-device": count_on_device}
