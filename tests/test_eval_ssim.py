"""Device-side SSIM of the evaluators (enerf_eval_ssim, io.hip), PINNED to skimage itself: ``tests/golden/ssim_cases.npz`` holds what
``skimage.metrics.structural_similarity(gt, pred, multichannel=True)`` (scikit-image 0.18.3, the reference's call in
lib/evaluators/enerf.py:76 and enerf_human.py:66) returned for the inputs of tests/ssim_cases.py after the evaluators' own
preprocessing (tools/make_golden_ssim.py).  Layers:

* the numpy float64 twin below (sliding 7x7 windows, direct summation) against every fixture value, <= 1e-12 — observed
  against the committed fixture: largest gap 3.3e-14 (smooth), 1.8e-14 at 1024 wide (full_zju, skimage's running-sum filter included), so the
  bound stays;
* the kernel sources on the CPU lane emulator and the gfx950 library (-m gpu) against the fixture, <= 1e-9 absolute.  Derived, not
  measured: inputs and their products are exact in float64, a 49-term sum carries <= 49 * 2^-53 relative error, the variance
  terms are divided by at least C2 = 3.6e-3, so each S moves by <~ 1e-10; a decade is left for the reductions;
* the evaluator surface (DeviceEvaluator(eval_ssim=True), DeviceEvaluatorHuman) against the twin on the same arrays, <= 1e-9;
* argument errors.
"""
import os

import numpy as np
import pytest
import torch

import ssim_cases

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ssim_cases.npz")
TOL = 1e-9          # kernel vs skimage (see above)
TWIN_TOL = 1e-12    # twin vs skimage

_needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")
_CASES = {}


def _case(name):
    """The case's arrays, after asserting that they are the arrays the fixture was computed from."""
    if name not in _CASES:
        g = np.load(GOLD)
        c = ssim_cases.build(name)
        for k, v in ssim_cases.sha1s(c).items():
            assert str(g[f"sha1/{name}/{k}"]) == v, f"{name}/{k}: the recipe in tests/ssim_cases.py no longer produces the fixture's input"
        c["expected"] = g[f"expected/{name}"]
        c["windows"] = g[f"windows/{name}"]
        assert c["expected"].dtype == np.float64 and c["expected"].shape == (c["pred"].shape[0],)
        _CASES[name] = c
    return _CASES[name]


# ---- the twin: skimage/metrics/_structural_similarity.py restated with direct window sums, float64, numpy only -------------
def _window_mean(a):
    h, w = a.shape
    out = np.zeros((h - 6, w - 6), np.float64)
    for dy in range(7):
        for dx in range(7):
            out += a[dy:dy + h - 6, dx:dx + w - 6]
    return out / 49.0


def twin_ssim(gt, pred):
    """ssim(gt, pred, multichannel=True) for (h,w,3) float32 arrays: only the windows wholly inside the image (crop(S, 3))."""
    assert gt.dtype == np.float32 and pred.dtype == np.float32 and gt.shape == pred.shape and gt.shape[2] == 3
    if gt.shape[0] < 7 or gt.shape[1] < 7:
        raise ValueError("win_size exceeds image extent")
    C1, C2, cov = (0.01 * 2.0) ** 2, (0.03 * 2.0) ** 2, 49.0 / 48.0       # data_range = 2 for float32 inputs
    per_channel = []
    for ch in range(3):
        x, y = gt[..., ch].astype(np.float64), pred[..., ch].astype(np.float64)
        ux, uy, uxx, uyy, uxy = (_window_mean(a) for a in (x, y, x * x, y * y, x * y))
        vx, vy, vxy = cov * (uxx - ux * ux), cov * (uyy - uy * uy), cov * (uxy - ux * uy)
        S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
        per_channel.append(S.mean())
    return float(np.mean(per_channel))


def bounding_rect(on):
    """cv2.boundingRect of a boolean mask -> (x, y, w, h); all zero when nothing is on."""
    ys, xs = np.nonzero(on)
    if ys.size == 0:
        return 0, 0, 0, 0
    return int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)


def evaluator_images(gt, pred, mask, evaluator, center):
    """What the reference's evaluator hands to ssim() for one image: (h,w,3) gt / pred, (h,w) mask or None."""
    gt, pred = gt.copy(), pred.copy()
    h, w = gt.shape[:2]
    if evaluator == "enerf":                                               # enerf.py:48-54,67-69
        on = np.ones((h, w), bool) if mask is None else mask >= 1
        if center:
            ch, cw = int(h * 0.1), int(w * 0.1)
            gt, pred, on = gt[ch:h - ch, cw:w - cw], pred[ch:h - ch, cw:w - cw], on[ch:h - ch, cw:w - cw]
        gt[~on] = 0
        pred[~on] = 0
        return gt, pred
    on = np.ones((h, w), bool) if mask is None else mask == 1              # enerf_human.py:39-42,54-56,64-66
    gt[~on] = 0
    pred[~on] = 0
    x, y, bw, bh = bounding_rect(on)
    return gt[y:y + bh, x:x + bw], pred[y:y + bh, x:x + bw]


def _case_images(c, b):
    return evaluator_images(c["gt"][b], c["pred"][b], None if c["mask"] is None else c["mask"][b], c["evaluator"], c["center"])


@pytest.mark.parametrize("name", ssim_cases.CASE_NAMES)
def test_twin_matches_skimage(name):
    c = _case(name)
    for b in range(c["pred"].shape[0]):
        gt, pred = _case_images(c, b)
        assert (gt.shape[0] - 6) * (gt.shape[1] - 6) == c["windows"][b]
        got = twin_ssim(gt, pred)
        print(f"twin {name}[{b}]: {got!r} vs skimage {c['expected'][b]!r}: {abs(got - c['expected'][b]):.3e}")
        assert abs(got - c["expected"][b]) <= TWIN_TOL
    if name == "identical":
        assert c["expected"][0] == 1.0


# ---- the kernels -------------------------------------------------------------------------------------------------------------
def _run_case(lib, dev, c):
    """(B,2) float64 {ssim, windows} of a fixture case through EnerfLib.eval_ssim, as the evaluators call it."""
    B, h, w, _ = c["pred"].shape
    T = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    pred, gt = T(c["pred"]).reshape(B, h * w, 3), T(c["gt"]).reshape(B, h * w, 3)
    mask = None if c["mask"] is None else T(c["mask"]).reshape(B, h * w)
    if c["evaluator"] == "human":
        kw = dict(bbox=True, mask_is_one=True)
    else:
        kw = dict(crop=(int(h * 0.1), int(w * 0.1)) if c["center"] else (0, 0))
    return lib.eval_ssim(pred, gt, mask, image_hw=(h, w), sync=False, **kw)


def _check_case(lib, dev, name):
    c = _case(name)
    out = _run_case(lib, dev, c).cpu().numpy()
    assert out.shape == (c["pred"].shape[0], 2)
    for b in range(out.shape[0]):
        print(f"{dev.type} {name}[{b}]: {out[b, 0]!r} vs skimage {c['expected'][b]!r}: {abs(out[b, 0] - c['expected'][b]):.3e}")
    for b in range(out.shape[0]):
        assert out[b, 1] == c["windows"][b]
        assert abs(out[b, 0] - c["expected"][b]) <= TOL
    if name == "identical":
        assert out[0, 0] == 1.0                                            # every S is x / x: bit-equal, not approximately
    return out


@pytest.mark.parametrize("name", ssim_cases.CASE_NAMES)       # full_zju included: under a second on the emulator
def test_eval_ssim_emulated(name):
    from emu_lib import emu_lib
    _check_case(emu_lib(), torch.device("cpu"), name)


def test_eval_ssim_wrapper_and_mask_types_emulated():
    """sync=True returns the floats; bool / uint8 / int32 masks and the two mask modes select the same pixels where they must."""
    from emu_lib import emu_lib
    lib = emu_lib()
    c = _case("mask012")
    B, h, w, _ = c["pred"].shape
    pred, gt = torch.from_numpy(c["pred"]).reshape(B, h * w, 3), torch.from_numpy(c["gt"]).reshape(B, h * w, 3)
    m = torch.from_numpy(c["mask"]).reshape(B, h * w)
    ref = lib.eval_ssim(pred, gt, m, image_hw=(h, w))
    assert isinstance(ref, list) and len(ref) == 1 and abs(ref[0] - c["expected"][0]) <= TOL
    assert lib.eval_ssim(pred, gt, m.to(torch.int32), image_hw=(h, w)) == ref
    assert lib.eval_ssim(pred, gt, m >= 1, image_hw=(h, w)) == ref
    assert lib.eval_ssim(pred[0], gt[0], m[0], image_hw=(h, w)) == ref               # (h*w,3) without the batch axis
    one = lib.eval_ssim(pred, gt, m, image_hw=(h, w), mask_is_one=True)             # value 2 is off now
    g, p = evaluator_images(c["gt"][0], c["pred"][0], (c["mask"][0] == 1).astype(np.uint8), "enerf", False)
    assert abs(one[0] - twin_ssim(g, p)) <= TOL and abs(one[0] - ref[0]) > 1e-3
    # the bounding box of a >= 1 mask (mask_is_one=False), the human evaluator's box of the same pixels
    hb = _case("human_box")
    pred, gt = torch.from_numpy(hb["pred"]).reshape(2, -1, 3), torch.from_numpy(hb["gt"]).reshape(2, -1, 3)
    m = torch.from_numpy(hb["mask"]).reshape(2, -1)
    wide = lib.eval_ssim(pred, gt, m, image_hw=(128, 128), bbox=True)
    for b in range(2):
        on = hb["mask"][b] >= 1
        g, p = hb["gt"][b].copy(), hb["pred"][b].copy()
        g[~on] = 0
        p[~on] = 0
        x, y, bw, bh = bounding_rect(on)
        assert abs(wide[b] - twin_ssim(g[y:y + bh, x:x + bw], p[y:y + bh, x:x + bw])) <= TOL


def _check_errors(lib, dev):
    from enerf_amd.lib import EnerfError
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
    with pytest.raises(EnerfError, match="unsupported"):                   # skimage: ValueError (win_size exceeds image extent)
        lib.eval_ssim(z(6 * 40, 3), z(6 * 40, 3), image_hw=(6, 40))
    with pytest.raises(EnerfError, match="unsupported"):
        lib.eval_ssim(z(40 * 6, 3), z(40 * 6, 3), image_hw=(40, 6))
    with pytest.raises(EnerfError, match="unsupported"):                   # 20 - 2*7 = 6 rows left
        lib.eval_ssim(z(20 * 40, 3), z(20 * 40, 3), image_hw=(20, 40), crop=(7, 2))
    assert len(lib.eval_ssim(z(20 * 40, 3), z(20 * 40, 3), image_hw=(20, 40), crop=(6, 2))) == 1
    m = torch.ones((20, 80), dtype=torch.uint8, device=dev)
    with pytest.raises(EnerfError, match="contiguous"):
        lib.eval_ssim(z(20 * 40, 3), z(20 * 40, 3), m[:, ::2], image_hw=(20, 40))
    with pytest.raises(EnerfError, match="int32 / uint8 / bool"):
        lib.eval_ssim(z(20 * 40, 3), z(20 * 40, 3), torch.ones(20 * 40, dtype=torch.float32, device=dev), image_hw=(20, 40))
    with pytest.raises(EnerfError, match="float32"):
        lib.eval_ssim(z(20 * 40, 3).double(), z(20 * 40, 3), image_hw=(20, 40))
    with pytest.raises(EnerfError):
        lib.eval_ssim(z(20 * 40, 3), z(20 * 41, 3), image_hw=(20, 40))
    with pytest.raises(EnerfError, match="needs a mask"):
        lib.eval_ssim(z(20 * 40, 3), z(20 * 40, 3), image_hw=(20, 40), bbox=True)
    # the C ABI itself: null pointers, bad modes; nothing is launched (the output keeps its fill)
    out = torch.full((1, 2), 7.0, dtype=torch.float64, device=dev)
    ws = torch.zeros(64, dtype=torch.float64, device=dev)
    a, b = z(20 * 40, 3), z(20 * 40, 3)
    st = lib.stream_of(a)
    f = lib.dll.enerf_eval_ssim
    assert f(None, b.data_ptr(), None, 0, 0, 1, 20, 40, 0, 0, 0, ws.data_ptr(), out.data_ptr(), st) == -1
    assert b"null" in lib.dll.enerf_last_error()
    assert f(a.data_ptr(), b.data_ptr(), None, 0, 0, 1, 20, 40, 0, 0, 0, None, out.data_ptr(), st) == -1
    assert f(a.data_ptr(), b.data_ptr(), None, 0, 0, 1, 20, 40, 0, 0, 0, ws.data_ptr(), None, st) == -1
    assert f(a.data_ptr(), b.data_ptr(), None, 0, 2, 1, 20, 40, 0, 0, 0, ws.data_ptr(), out.data_ptr(), st) == -1
    assert f(a.data_ptr(), b.data_ptr(), None, 0, 0, 1, 20, 40, 3, 0, 0, ws.data_ptr(), out.data_ptr(), st) == -1
    assert f(a.data_ptr(), b.data_ptr(), ws.data_ptr(), 2, 0, 1, 20, 40, 0, 0, 0, ws.data_ptr(), out.data_ptr(), st) == -1
    assert f(a.data_ptr(), b.data_ptr(), None, 0, 0, 0, 20, 40, 0, 0, 0, ws.data_ptr(), out.data_ptr(), st) == -1
    assert f(a.data_ptr(), b.data_ptr(), None, 0, 0, 1, 6, 40, 0, 0, 0, ws.data_ptr(), out.data_ptr(), st) == -1
    assert b"unsupported" in lib.dll.enerf_last_error()
    assert lib.dll.enerf_eval_ssim_workspace_bytes(1, 6, 40, 0, 0, 0) == 0
    assert lib.dll.enerf_eval_ssim_workspace_bytes(1, 20, 40, 1, 7, 2) == 0
    nb = lib.dll.enerf_eval_ssim_workspace_bytes(2, 20, 40, 0, 0, 0)       # the boxes and at least one partial sum per image
    assert nb >= 2 * 16 + 2 * 8 and nb % 8 == 0
    assert out.cpu().tolist() == [[7.0, 7.0]]
    # an all-zero mask_at_box, and a box under 7 pixels: known on the device only -> NaN, 0 windows, no fault
    rng = np.random.default_rng(0)
    pred = torch.from_numpy(rng.uniform(0, 1, (3, 20 * 40, 3)).astype(np.float32)).to(dev)
    gt = torch.from_numpy(rng.uniform(0, 1, (3, 20 * 40, 3)).astype(np.float32)).to(dev)
    m = torch.zeros((3, 20, 40), dtype=torch.int32, device=dev)
    m[1, 4:10, 3:30] = 1                                                   # 6 rows
    m[2, 4:11, 3:10] = 1                                                   # exactly 7 x 7: one window
    res = lib.eval_ssim(pred, gt, m.reshape(3, -1), image_hw=(20, 40), bbox=True, mask_is_one=True, sync=False).cpu().numpy()
    assert np.isnan(res[0, 0]) and res[0, 1] == 0 and np.isnan(res[1, 0]) and res[1, 1] == 0
    g, p = gt[2].cpu().numpy().reshape(20, 40, 3)[4:11, 3:10], pred[2].cpu().numpy().reshape(20, 40, 3)[4:11, 3:10]
    assert res[2, 1] == 1 and abs(res[2, 0] - twin_ssim(g, p)) <= TOL


def test_eval_ssim_errors_emulated():
    from emu_lib import emu_lib
    _check_errors(emu_lib(), torch.device("cpu"))


# ---- the evaluator surface ------------------------------------------------------------------------------------------------------
def _psnr64(pred, gt, on):
    return 10 * np.log10(1.0 / np.mean((pred[on].astype(np.float64) - gt[on].astype(np.float64)) ** 2))


def _check_device_evaluator(lib, dev):
    """DeviceEvaluator(eval_ssim=True) on a rendered tiny_s3 frame with random gt / masks: ssim, ssim_level0/1 equal the twin on the
    same arrays; the default constructor's dictionary is exactly what it was."""
    from enerf_amd.evaluator import DeviceEvaluator
    from enerf_amd.network import Network
    from golden_cases import case_batch, case_config, load_weights
    cfg, batch = case_config("tiny_s3"), case_batch("tiny_s3")
    net = Network(cfg, lib=lib).eval()
    net.load_state_dict(load_weights(), strict=False)
    net = net.to(dev)
    batch = {k: v.to(dev) for k, v in batch.items()}
    out = net(batch)
    rng = np.random.default_rng(1)
    sizes = ((8, 16), (32, 64))
    for i, (h, w) in enumerate(sizes):
        # gt near the rendering, so that SSIM is far from 0 and the variance terms matter
        gt = out[f"rgb_level{i}"].cpu().numpy().reshape(1, h * w, 3) + rng.normal(0, 0.05, (1, h * w, 3)).astype(np.float32)
        batch[f"rgb_{i}"] = torch.from_numpy(gt.astype(np.float32)).to(dev)
        batch[f"msk_{i}"] = torch.from_numpy((rng.uniform(size=(1, h * w)) > 0.2).astype(np.uint8) * rng.integers(1, 3, (1, h * w)).astype(np.uint8)).to(dev)
    plain = DeviceEvaluator(cfg, lib=lib)
    plain.evaluate(out, batch)
    s0 = plain.summarize()
    assert sorted(s0) == ["psnr", "psnr_level0", "psnr_level1"]            # today's keys, nothing added by default
    ev = DeviceEvaluator(cfg, eval_ssim=True, lib=lib)
    ev.evaluate(out, batch)
    ev.evaluate(out, batch)                                                # two frames: the mean of two equal values
    s = ev.summarize()
    assert sorted(s) == ["psnr", "psnr_level0", "psnr_level1", "ssim", "ssim_level0", "ssim_level1"]
    # the psnr accumulator adds with fp64 atomics on the GPU: equal to rounding, not bit for bit, from call to call
    assert s["psnr"] == pytest.approx(s0["psnr"], rel=1e-12) and s["psnr_level0"] == pytest.approx(s0["psnr_level0"], rel=1e-12)
    for i, (h, w) in enumerate(sizes):
        pred = out[f"rgb_level{i}"][0].cpu().numpy().reshape(h, w, 3)
        gt = batch[f"rgb_{i}"][0].cpu().numpy().reshape(h, w, 3)
        msk = batch[f"msk_{i}"][0].cpu().numpy().reshape(h, w)
        g, p = evaluator_images(gt, pred, msk, "enerf", False)
        want = twin_ssim(g, p)
        print(f"{dev.type} evaluator level {i}: {s[f'ssim_level{i}']!r} vs twin {want!r}")
        assert abs(s[f"ssim_level{i}"] - want) <= TOL
        assert s[f"psnr_level{i}"] == pytest.approx(_psnr64(pred, gt, msk >= 1), rel=1e-9)
    assert s["ssim"] == s["ssim_level1"]
    assert np.isnan(ev.summarize()["psnr"])                                # summarize() resets


def _check_synthetic_frames(lib, dev):
    """Both evaluators on frames that need no network (the evaluators only read rgb_level{i}): eval_center with non-zero crops at
    both levels, B = 2, depth statistics next to SSIM, and the human evaluator's all-ones levels."""
    from enerf_amd.config import EnerfConfig
    from enerf_amd.evaluator import DeviceEvaluator, DeviceEvaluatorHuman
    cfg = EnerfConfig().with_cas(render_if=(True, True))
    rng = np.random.default_rng(2)
    B, H, W = 2, 40, 64
    sizes = [(int(H * s), int(W * s)) for s in cfg.cas.render_scale]
    T = lambda a: torch.from_numpy(a).to(dev)
    out, batch = {}, {"src_inps": torch.zeros((B, 2, 3, H, W), device=dev)}
    for i, (h, w) in enumerate(sizes):
        gt = rng.uniform(0, 1, (B, h * w, 3)).astype(np.float32)
        out[f"rgb_level{i}"] = T(np.clip(gt + rng.normal(0, 0.1, gt.shape), 0, 1).astype(np.float32))
        batch[f"rgb_{i}"] = T(gt)
        batch[f"msk_{i}"] = T((rng.uniform(size=(B, h * w)) > 0.3).astype(np.uint8))
    h, w = sizes[-1]
    out[f"depth_level{len(sizes) - 1}"] = T(rng.uniform(400, 900, (B, h * w)).astype(np.float32))
    batch["tar_dpt"] = out[f"depth_level{len(sizes) - 1}"].reshape(B, h, w) + 1.0
    mab = np.zeros((B, h, w), np.int32)
    mab[0, 0:h // 2, 3:w - 5] = 1
    mab[1, 7:h - 2, 0:w // 3] = 1
    mab[1, 1, w - 1] = 2                                                   # not == 1
    batch["mask_at_box"] = T(mab)
    ev = DeviceEvaluator(cfg, eval_center=True, eval_depth=True, eval_ssim=True, lib=lib)
    ev.evaluate(out, batch)
    s = ev.summarize()
    ref = DeviceEvaluator(cfg, eval_center=True, eval_depth=True, lib=lib)
    ref.evaluate(out, batch)
    r = ref.summarize()
    assert sorted(k for k in s if not k.startswith("ssim")) == sorted(r)   # psnr / depth numbers are the plain evaluator's
    for k, v in r.items():
        assert s[k] == pytest.approx(v, rel=1e-12)
    hs = DeviceEvaluatorHuman(cfg, lib=lib)
    hs.evaluate(out, batch)
    sh = hs.summarize()
    assert sorted(sh) == ["psnr", "psnr_level0", "psnr_level1", "ssim", "ssim_level0", "ssim_level1"]
    for i, (h, w) in enumerate(sizes):
        assert int(h * 0.1) > 0 and int(w * 0.1) > 0
        want, want_h, want_p = [], [], []
        for b in range(B):
            pred = out[f"rgb_level{i}"][b].cpu().numpy().reshape(h, w, 3)
            gt = batch[f"rgb_{i}"][b].cpu().numpy().reshape(h, w, 3)
            want.append(twin_ssim(*evaluator_images(gt, pred, batch[f"msk_{i}"][b].cpu().numpy().reshape(h, w), "enerf", True)))
            m = mab[b] if i == len(sizes) - 1 else None
            want_h.append(twin_ssim(*evaluator_images(gt, pred, m, "human", False)))
            want_p.append(_psnr64(pred, gt, np.ones((h, w), bool) if m is None else m == 1))
        assert abs(s[f"ssim_level{i}"] - np.mean(want)) <= TOL
        assert abs(sh[f"ssim_level{i}"] - np.mean(want_h)) <= TOL
        assert sh[f"psnr_level{i}"] == pytest.approx(np.mean(want_p), rel=1e-9)
    assert s["ssim"] == s["ssim_level1"] and sh["ssim"] == sh["ssim_level1"] and sh["psnr"] == sh["psnr_level1"]


def _check_human_evaluator(lib, dev, name):
    """DeviceEvaluatorHuman on a rendered human frame: psnr by the float64 expression over mask == 1, ssim by the twin on the
    mask's bounding rectangle."""
    from enerf_amd.evaluator import DeviceEvaluatorHuman
    from enerf_amd.network import NetworkHuman
    from golden_cases import CASES, case_batch, case_config, load_weights
    cfg, batch = case_config(name), case_batch(name)
    H, W = CASES[name]["H"], CASES[name]["W"]
    net = NetworkHuman(cfg, lib=lib).eval()
    net.load_state_dict(load_weights(), strict=False)
    net = net.to(dev)
    batch = {k: v.to(dev) for k, v in batch.items()}
    out = net(batch)
    pred = out["rgb_level1"][0].cpu().numpy().reshape(H, W, 3)
    rng = np.random.default_rng(3)
    gt = (pred + rng.normal(0, 0.05, pred.shape)).astype(np.float32)
    batch["rgb_1"] = torch.from_numpy(gt.reshape(1, H * W, 3)).to(dev)
    ev = DeviceEvaluatorHuman(cfg, lib=lib)
    ev.evaluate(out, batch)
    s = ev.summarize()
    assert sorted(s) == ["psnr", "psnr_level1", "ssim", "ssim_level1"]
    m = batch["mask_at_box"][0].cpu().numpy().reshape(H, W)
    assert 0 < (m == 1).sum() < H * W
    want = twin_ssim(*evaluator_images(gt, pred, m, "human", False))
    print(f"{dev.type} human evaluator {name}: {s['ssim']!r} vs twin {want!r}")
    assert abs(s["ssim"] - want) <= TOL and s["ssim"] == s["ssim_level1"]
    assert s["psnr"] == pytest.approx(_psnr64(pred, gt, m == 1), rel=1e-9)


def test_device_evaluator_ssim_emulated():
    from emu_lib import emu_lib
    _check_device_evaluator(emu_lib(), torch.device("cpu"))


def test_evaluators_on_synthetic_frames_emulated():
    from emu_lib import emu_lib
    _check_synthetic_frames(emu_lib(), torch.device("cpu"))


def test_device_evaluator_human_emulated():
    from emu_lib import emu_lib
    _check_human_evaluator(emu_lib(), torch.device("cpu"), "tiny_s4_mask")


# ---- the gfx950 library ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@_needs_gpu
@pytest.mark.parametrize("name", ssim_cases.CASE_NAMES)
def test_eval_ssim_gpu(name):
    from enerf_amd.lib import get_lib
    dev = torch.device("cuda:0")
    first = _check_case(get_lib(), dev, name)
    again = _run_case(get_lib(), dev, _case(name)).cpu().numpy()
    assert first.tobytes() == again.tobytes()                              # fixed summation order: bit-equal from call to call


@pytest.mark.gpu
@_needs_gpu
def test_eval_ssim_errors_gpu():
    from enerf_amd.lib import get_lib
    _check_errors(get_lib(), torch.device("cuda:0"))


@pytest.mark.gpu
@_needs_gpu
def test_evaluators_gpu():
    from enerf_amd.lib import get_lib
    dev = torch.device("cuda:0")
    _check_device_evaluator(get_lib(), dev)
    _check_synthetic_frames(get_lib(), dev)
    _check_human_evaluator(get_lib(), dev, "tiny_s4_mask")
    _check_human_evaluator(get_lib(), dev, "zju_small")


@pytest.mark.gpu
@_needs_gpu
def test_eval_ssim_has_no_implicit_host_sync():
    """box -> moments -> reduction enqueue only: under ``torch.cuda.set_sync_debug_mode("error")`` any synchronisation raises."""
    from enerf_amd.lib import get_lib
    dev = torch.device("cuda:0")
    lib = get_lib()
    c = _case("human_box")
    pred, gt = torch.from_numpy(c["pred"]).to(dev).reshape(2, -1, 3), torch.from_numpy(c["gt"]).to(dev).reshape(2, -1, 3)
    m = torch.from_numpy(c["mask"]).to(dev).reshape(2, -1)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = lib.eval_ssim(pred, gt, m, image_hw=(128, 128), bbox=True, mask_is_one=True, sync=False)
        acc = lib.eval_stats(pred[0], gt[0], m[0], image_hw=(128, 128), sync=False)
        both = torch.cat([acc, out.reshape(-1)])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    res = both.cpu().numpy()
    assert np.abs(res[[6, 8]] - c["expected"]).max() <= TOL and list(res[[7, 9]]) == list(c["windows"])
