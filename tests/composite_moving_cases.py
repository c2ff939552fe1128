"""Cases of the composite network with boxes that move — sizes on the host, positions on the device (enerf_forward_composite_moving,
enerf_forward_composite_cached_moving, the _at kernels, enerf_layer_boxes; Network's ``bbox_size`` / ``bbox_xy``) — shared by the
emulator tests (test_composite_moving.py) and the MI355X tests (test_composite_moving_gpu.py): every function takes the library and
the device and asserts.

    same_bits_case     forward / forward_cached with bbox_size + bbox_xy == the same with bbox = (x, y, w, h): every output, every
                       depth / std map, torch.equal; ONE shape, the same buffers and workspace over the whole position list, where the
                       host path makes a shape per position; at the fixture's own position the reference's fixture within REL_TOL
    clamp_case         positions outside the image, huge and non-finite == the host path at the clamped box; bit 0 of bbox_flags
    kernels alone      the windowed volume, the windowed regression and the merge with a corner table == their scalar-argument twins
    layer_boxes_case   enerf_layer_boxes against a float64 numpy restatement of enerf_outdoor/enerf.py:156-164
    graph_case         (GPU) layer_boxes -> forward_cached captured once, replayed for cameras whose boxes land elsewhere
    refusals

Nothing but layer_boxes' near_far has a tolerance: the two paths run the same arithmetic on the same integers.

Shapes: composite_cases.NETWORK_CASES "a" (L = 2, windows 64 x 64 and 64 x 32) and "b" (L = 1, 32 x 32) at 64 x 96 with the
reference's weights — the smallest frames at which a window can sit at every edge and truncate at both scales."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import composite_cases as CC
from enerf_amd.lib import CompositeFrameArgs, EnerfError
from enerf_amd.network_composite import Network
from enerf_amd.synth import make_batch

EINVAL = -1
V = 4                                   # cached views
# the first entry of each list is the fixture's own position; (5,3), (63,31), (37,9), (7,0), (29,13): x * 0.25 and x * 0.5 truncate
POSITIONS = {
    "b": [[(32, 16)], [(0, 0)], [(64, 32)], [(5, 3)], [(63, 31)], [(37, 9)]],
    "a": [[(32, 0), (0, 0)], [(7, 0), (29, 13)], [(0, 0), (32, 32)]],
}
INDEX_ROW = {3: [3, 0, 1], 2: [2, 0]}
# (positions, the box the resolution makes of them, bit 0 per layer): fixture "b" is 32 x 32 in 96 x 64, so x in [0, 64], y in
# [0, 32]; fixture "a"'s layer 0 is 64 x 64 (x in [0, 32], y = 0), its layer 1 stays where it is and must not be flagged
CLAMPS = {
    "b": [([(-3.0, 200.0)], [(0, 32)], [1]), ([(1e9, -1e9)], [(64, 0)], [1]), ([(float("nan"), float("inf"))], [(0, 0)], [1])],
    "a": [([(-3.0, 200.0), (0.0, 0.0)], [(0, 0), (0, 0)], [1, 0])],
}


def _same(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert torch.equal(a, b), (what, float((a - b).abs().max()))


def _load(lib, dev, name, **kw):
    """A network with the reference's weights of the fixture (composite_cases.network_case's loading)."""
    net = Network(CC.network_config(name), CC.NETWORK_CASES[name]["L"], lib=lib, **kw)
    full = dict(net.state_dict())
    full.update(CC.network_weights(name))
    net.load_state_dict(full, strict=True)
    return net.to(dev).eval()


class Rig:
    """Fixture ``name``: two networks with the same weights — ``mov`` only ever sees bbox_size / bbox_xy, ``host`` only bbox —, the
    fixture's batch without its boxes, and a cache of V views for each network."""

    def __init__(self, lib, dev, name):
        c = CC.NETWORK_CASES[name]
        self.name, self.lib, self.dev, self.case = name, lib, dev, c
        self.sizes = [(b[2], b[3]) for b in c["boxes"]]
        self.mov, self.host = _load(lib, dev, name).prepare(), _load(lib, dev, name).prepare()
        self.batch = {k: torch.from_numpy(v).to(dev) for k, v in CC.network_batch(name).items() if k != "bbox"}
        b = make_batch(c["H"], c["W"], V, CC.network_config(name), seed=c["seed"] + 7, textured=True)
        bg = np.random.default_rng(c["seed"] + 300).uniform(-1, 1, size=(V, 3, c["H"], c["W"])).astype(np.float32)
        self.views = tuple(torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (b["src_inps"][0], bg, b["src_exts"][0], b["src_ixts"][0]))
        self.tar = {k: v for k, v in self.batch.items() if not k.startswith("src_") and k != "bg_src_inps"}
        self.caches = {}
        self.view_idx = torch.tensor(INDEX_ROW[c["S"]], dtype=torch.int32, device=dev)

    def cache(self, net):
        if id(net) not in self.caches:
            self.caches[id(net)] = net.cache_sources(*self.views)
        return self.caches[id(net)]

    def xy(self, positions):
        return torch.tensor(positions, dtype=torch.float32).to(self.dev)

    def run(self, net, cached, extra):
        """(outputs, intermediates) of one frame with ``extra`` = the batch's box keys, cloned."""
        b = dict(self.tar if cached else self.batch, **extra)
        with torch.no_grad():
            out = net.forward_cached(self.cache(net), self.view_idx, b) if cached else net(b)
            return {k: v.clone() for k, v in out.items()}, {k: v.clone() for k, v in net.intermediates.items()}

    def moving(self, positions, cached=False, sizes=None):
        return self.run(self.mov, cached, {"bbox_size": sizes or self.sizes, "bbox_xy": self.xy(positions)})

    def on_host(self, boxes_xy, cached=False):
        boxes = [(x, y, w, h) for (x, y), (w, h) in zip(boxes_xy, self.sizes)]
        return self.run(self.host, cached, {"bbox": torch.tensor([boxes], dtype=torch.float32)})


_RIGS = {}


def rig(lib, dev, name):
    key = (name, dev.type)
    if key not in _RIGS:
        _RIGS[key] = Rig(lib, dev, name)
    return _RIGS[key]


def assert_frames_equal(got, ref, what, flags=None):
    cas_keys = {k for k in got[1] if k != "bbox_flags"}
    assert sorted(got[0]) == sorted(ref[0]) and cas_keys == set(ref[1]), what
    assert any(k.startswith("depth_") for k in cas_keys) and any(k.startswith("std_") for k in cas_keys)
    for k in ref[0]:
        _same(got[0][k], ref[0][k], (what, k))
        assert bool(torch.isfinite(got[0][k]).all()), (what, k, "finite")
    for k in ref[1]:
        _same(got[1][k], ref[1][k], (what, k))
    if flags is not None:
        f = got[1]["bbox_flags"]
        assert f.dtype == torch.int32 and f.device.type == got[0][next(iter(got[0]))].device.type
        assert f.cpu().tolist() == list(flags), (what, f.cpu().tolist(), flags)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1 + 2. the same bits as the host path, without re-planning
def _shape_state(net):
    (st,) = net._shapes.values()
    return {k: v.data_ptr() for k, v in st["call.outs"].items()}, st["call.ws"].data_ptr()


def same_bits_case(lib, dev, name, cached):
    r = rig(lib, dev, name)
    c, cas = r.case, CC.network_config(name).cas
    r.mov._shapes.clear(), r.host._shapes.clear()
    want_keys = {f"{k}_level{i}" for i in range(cas.num) if cas.render_if[i] for k in ("rgb", "depth", "weights", "net_output", "z_vals")}
    state, frames = None, []
    for n, pos in enumerate(POSITIONS[name]):
        got = r.moving(pos, cached)
        assert set(got[0]) == want_keys
        assert_frames_equal(got, r.on_host(pos, cached), (name, "cached" if cached else "forward", pos), flags=[0] * c["L"])
        assert len(r.mov._shapes) == 1, "a moved box is not a new shape"
        if state is None:
            state = _shape_state(r.mov)
        assert _shape_state(r.mov) == state, "the outputs and the workspace stay where they are"
        frames.append(got[0])
    last = f"rgb_level{cas.num - 1}"
    assert not torch.equal(frames[0][last], frames[1][last]), "the box moved"
    assert len(r.host._shapes) > 1, "the host path keys its buffers by the whole box: a shape per position"
    assert_frames_equal(r.moving(POSITIONS[name][0], cached), (frames[0], r.on_host(POSITIONS[name][0], cached)[1]), (name, "first again"))
    if not cached:                     # the fixture's own position: the reference's fixture, within the bar of test_composite.py
        gold = np.load(os.path.join(CC.GOLDEN, f"composite_{name}.npz"))
        got = r.moving(POSITIONS[name][0])
        have = dict(got[0], **{f"mid/{k}": v for k, v in got[1].items() if k != "bbox_flags"})
        assert set(have) == set(gold.files)
        for k in gold.files:
            a, b = have[k].cpu().double(), torch.from_numpy(gold[k]).double()
            e = float((a - b).abs().max()) / float(b.abs().max())
            print(f"[composite moving] case {name} {k}: e {e:.2e}")
            assert e <= CC.REL_TOL, (name, k, e)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. clamp and flags
def clamp_case(lib, dev, name, cached=False):
    r = rig(lib, dev, name)
    for pos, clamped, flags in CLAMPS[name]:
        assert_frames_equal(r.moving(pos, cached), r.on_host(clamped, cached), (name, "clamp", pos), flags=flags)
    # a host list (converted and uploaded first) and a (1,L,2) float64 tensor are the same frame
    pos = POSITIONS[name][1]
    ref = r.moving(pos, cached)
    for form in ([list(p) for p in pos], torch.tensor([pos], dtype=torch.float64)):
        got = r.run(r.mov, cached, {"bbox_size": r.sizes, "bbox_xy": form})
        assert_frames_equal(got, (ref[0], {k: v for k, v in ref[1].items() if k != "bbox_flags"}), (name, "host positions"), flags=[0] * r.case["L"])


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the kernels alone: a corner table against the scalar arguments
GRID_H, GRID_W = 8, 12
PLACES = {"corner": (0, 0), "odd": (3, 1), "far edge": (GRID_W - 4, GRID_H - 4)}          # of a 4 x 4 window


def _corner(dev, *xy):
    return torch.tensor(xy, dtype=torch.int32).reshape(-1).to(dev)


def volume_at_case(lib, dev, Cc):
    from enerf_amd.config import EnerfConfig
    S, D, h, w = 3, 4, GRID_H, GRID_W
    cas = EnerfConfig().cas
    batch = {k: torch.from_numpy(v).to(dev) for k, v in make_batch(4 * h, 4 * w, S, EnerfConfig(), seed=11, B=1).items()}
    g = torch.Generator().manual_seed(300 + Cc)
    feat = torch.randn(1, S, h, w, Cc, generator=g).to(dev)
    near, far = float(batch["near_far"][0, 0]), float(batch["near_far"][0, 1])
    dv = (near + (far - near) * torch.rand(1, D, h, w, generator=g)).to(dev)
    proj = lib.get_proj_mats(batch["src_ixts"], batch["src_exts"], batch["tar_ixt"], batch["tar_ext"], cas.im_feat_scale[0], cas.volume_scale[0])
    seen = []
    for where, (x0, y0) in PLACES.items():
        for ww, wh in ((4, 4), (8, 4)):
            x = min(x0, w - ww)
            want = lib.build_feature_volume_window(feat, proj, dv, Cc, (x, y0, ww, wh))
            got = lib.build_feature_volume_window_at(feat, proj, dv, Cc, _corner(dev, x, y0), (ww, wh))
            _same(got, want, ("volume_at", Cc, where, ww))
            seen.append(want)
    assert float(seen[0].abs().max()) > 0 and not torch.equal(seen[0], seen[2])


def regression_at_case(lib, dev, D):
    h, w = GRID_H, GRID_W
    g = torch.Generator().manual_seed(400 + D)
    dv = (0.3 + 2.0 * torch.rand(1, D, h, w, generator=g)).to(dev)
    prob = (3.0 * torch.randn(1, D, 4, 4, generator=g)).to(dev)
    for depth_inv in (True, False):
        outs = []
        for where, (x0, y0) in PLACES.items():
            want = lib.depth_regression_window(prob, dv, depth_inv, (x0, y0, 4, 4))
            got = lib.depth_regression_window_at(prob, dv, depth_inv, _corner(dev, x0, y0), (4, 4))
            for nm, a, b in zip(("depth", "std"), got, want):
                _same(a, b, ("regression_at", D, depth_inv, where, nm))
            outs.append(want[0])
        assert not torch.equal(outs[0], outs[1])


def layers_at_case(lib, dev, L):
    """A 16 x 24 image (two blocks of 256 pixels); L windows of different sizes, all in a corner, at odd offsets, at the far edge."""
    H, W, Ns = 16, 24, 2
    sizes = [(8, 6), (5, 9), (12, 4), (3, 3)][:L]
    g = torch.Generator().manual_seed(500 + L)

    def samples(n, lo, hi):
        raw = torch.rand(n, Ns, 4, generator=g)
        raw[..., 3] = -torch.log(torch.rand(n, Ns, generator=g).clamp_min(1e-3)) * 2.0
        return raw.to(dev), (lo + (hi - lo) * torch.rand(n, Ns, generator=g)).to(dev)

    fg = [samples(ww * wh, 1.0 + 0.3 * l, 3.0 + 0.3 * l) for l, (ww, wh) in enumerate(sizes)]
    bg = samples(H * W, 4.0, 9.0)
    places = {"corner": [(0, 0)] * L, "odd": [(3 + 2 * l, 1 + l) for l in range(L)], "far edge": [(W - ww, H - wh) for ww, wh in sizes]}
    outs = []
    for where, xy in places.items():
        wins = [(x, y, ww, wh) for (x, y), (ww, wh) in zip(xy, sizes)]
        want = lib.composite_layers(fg, wins, bg, H, W)
        got = lib.composite_layers_at(fg, _corner(dev, *xy), sizes, bg, H, W)
        assert set(got) == set(want)
        for k in want:
            _same(got[k], want[k], ("layers_at", L, where, k))
        outs.append(want["rgb"])
    assert not torch.equal(outs[0], outs[2])


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. layer_boxes against enerf_outdoor/enerf.py:156-164 in float64, the cv2 lines replaced by the rectangle of the rounded corners
IMG_H, IMG_W = 64, 96
_K = np.array([[110.0, 0.0, 47.3], [0.0, 108.0, 31.6], [0.0, 0.0, 1.0]])


def _pose(rx, ry, rz, t):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    R = (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]]) @ np.array([[cy, 0, sy], [0, 1.0, 0], [-sy, 0, cy]])
         @ np.array([[1.0, 0, 0], [0, cx, -sx], [0, sx, cx]]))
    E = np.eye(4)
    E[:3, :3], E[:3, 3] = R, t
    return E


# name -> (bounds (L,2,3), extrinsic, sizes or None = (w_ori, h_ori) of the float64 rectangle, flags expected)
BOX_CASES = {
    "inside": (np.array([[[-0.30, -0.22, 4.0], [0.25, 0.31, 4.6]]]), _pose(0.03, -0.05, 0.02, [0.1, 0.05, 0.3]), [(32, 32)], [0]),
    "cut left and top": (np.array([[[-2.1, -1.4, 4.0], [-1.5, -0.9, 4.5]]]), _pose(0.02, 0.04, -0.03, [0.0, 0.0, 0.2]), [(32, 32)], [0]),
    "larger than the window": (np.array([[[-0.9, -0.6, 3.0], [0.8, 0.7, 3.8]]]), _pose(0.0, 0.03, 0.01, [0.05, 0.0, 0.0]), [(32, 32)], [2]),
    "behind the camera": (np.array([[[-0.3, -0.2, -0.5], [0.3, 0.2, 1.5]]]), _pose(0.01, 0.02, 0.0, [0.0, 0.0, 0.1]), [(32, 32)], [4]),
    "misses the image": (np.array([[[4.0, -0.2, 3.0], [4.5, 0.3, 3.5]]]), _pose(0.0, 0.0, 0.0, [0.0, 0.0, 0.0]), [(32, 32)], [8]),
    "w_ori == w": (np.array([[[-0.41, -0.27, 4.1], [0.33, 0.36, 4.9]]]), _pose(-0.02, 0.03, 0.04, [0.02, -0.03, 0.1]), None, [0]),
    "four layers": (np.array([[[-0.30, -0.22, 4.0], [0.25, 0.31, 4.6]], [[-1.3, -0.5, 5.0], [-0.7, 0.1, 5.5]],
                              [[0.6, 0.2, 3.5], [1.0, 0.6, 4.1]], [[-0.2, -0.9, 6.0], [0.9, -0.1, 7.0]]]),
                    _pose(0.03, -0.02, 0.05, [0.0, 0.1, 0.2]), [(32, 32), (64, 32), (32, 64), (32, 32)], [0, 0, 0, 0]),
}


def _corners(bounds):
    """base_utils.get_bound_corners."""
    (x0, y0, z0), (x1, y1, z1) = bounds
    return np.array([[x0, y0, z0], [x0, y0, z1], [x0, y1, z0], [x0, y1, z1], [x1, y0, z0], [x1, y0, z1], [x1, y1, z0], [x1, y1, z1]])


def boxes_reference(bounds, ext, K, H, W, sizes, near_min):
    """Float64.  Returns xy (L,2), near_far (L,2), flags (L), the projected coordinates (L,8,2), z (L,8), the near_far bound (L)
    and the clipped rectangle's (w_ori, h_ori) per layer."""
    xy, nf, flags, pix, zs, bound, ori = [], [], [], [], [], [], []
    R, t = ext[:3, :3], ext[:3, 3]
    for l, b in enumerate(bounds):
        p = _corners(b)
        cam = p @ R.T + t                                            # enerf.py:156
        z = cam[:, 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            uv = (cam @ K.T)[:, :2] / z[:, None]                     # base_utils.project, K's last row (0, 0, 1)
        r = np.round(uv)                                             # get_bound_2d_mask: np.round, half to even
        pix.append(uv), zs.append(z)
        bound.append(float((np.abs(p * R[2]).sum(1) + abs(t[2])).max()) * 8 * 2.0 ** -24)
        nf.append((max(z.min(), near_min), z.max()))                 # enerf.py:158 (+ the interactive dataset's near_min)
        if (z <= 0).any():
            xy.append((0.0, 0.0)), flags.append(4), ori.append((0, 0))
            continue
        x0, x1, y0, y1 = r[:, 0].min(), r[:, 0].max(), r[:, 1].min(), r[:, 1].max()
        f = 8 if (x1 < 0 or x0 > W - 1 or y1 < 0 or y0 > H - 1) else 0
        x0, x1, y0, y1 = (int(np.clip(v, 0, hi)) for v, hi in ((x0, W - 1), (x1, W - 1), (y0, H - 1), (y1, H - 1)))
        w_ori, h_ori = x1 - x0 + 1, y1 - y0 + 1                      # cv2.boundingRect of the rectangle's pixels
        w, h = sizes[l] if sizes is not None else (w_ori, h_ori)
        if w_ori > w or h_ori > h:
            f |= 2
        xy.append((float(x0 - (w - w_ori) // 2), float(y0 - (h - h_ori) // 2)))      # enerf.py:163-164
        flags.append(f), ori.append((w_ori, h_ori))
    return np.array(xy), np.array(nf), flags, np.array(pix), np.array(zs), bound, ori


def layer_boxes_case(lib, dev, which):
    bounds, ext, sizes, want_flags = BOX_CASES[which]
    ref = boxes_reference(bounds, ext, _K, IMG_H, IMG_W, sizes, 0.05)
    if sizes is None:
        sizes = ref[6]
        ref = boxes_reference(bounds, ext, _K, IMG_H, IMG_W, sizes, 0.05)
        assert ref[6] == sizes
    xy, nf, flags, pix, z, bound, _ = ref
    # the condition, on the float64 values alone: no projected coordinate of a corner in front of the camera lies within 1e-3 of a
    # half-integer, where float32 and float64 could round apart
    front = z > 0
    frac = np.abs(pix[front] - np.floor(pix[front]) - 0.5)
    assert front.any() and float(frac.min()) > 1e-3, (which, float(frac.min()))
    assert flags == want_flags, (which, flags)
    L = len(bounds)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    keep = torch.full((L + 1, 2), -7.0, device=dev)
    out = (torch.empty(L, 2, device=dev), keep, torch.empty(L, dtype=torch.int32, device=dev))
    got = lib.layer_boxes(t(bounds), t(ext[None]), t(_K[None]), IMG_H, IMG_W, sizes, near_min=0.05, out=out)
    assert got[2].cpu().tolist() == flags, (which, got[2].cpu().tolist(), flags)
    assert np.array_equal(got[0].cpu().numpy().astype(np.float64), xy), (which, got[0].cpu().numpy(), xy)
    assert keep[L].cpu().tolist() == [-7.0, -7.0], "the background's row is not touched"
    err = np.abs(got[1][:L].cpu().numpy().astype(np.float64) - nf)
    for l in range(L):
        print(f"[layer_boxes] {which} layer {l}: near_far error {err[l].max():.2e} (bound {bound[l]:.2e})")
        assert float(err[l].max()) <= bound[l], (which, l, err[l], bound[l])
    if which == "inside":                 # what the frame takes: the default output, no readback needed to use it
        xy2, nf2, fl2 = lib.layer_boxes(t(bounds), t(ext[None]), t(_K[None]), IMG_H, IMG_W, sizes, near_min=0.05)
        assert torch.equal(xy2, got[0]) and torch.equal(fl2, got[2]) and torch.equal(nf2[:L], got[1][:L])
        with pytest.raises(EnerfError, match="L sizes"):
            lib.layer_boxes(t(bounds), t(ext[None]), t(_K[None]), IMG_H, IMG_W, sizes + [(32, 32)])
        with pytest.raises(EnerfError, match="must be positive"):
            lib.layer_boxes(t(bounds), t(ext[None]), t(_K[None]), IMG_H, IMG_W, [(0, 32)])


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. graph replay (GPU only)
def _bounds_landing_at(r, want_xy):
    """A world box whose position for the fixture's target camera is ``want_xy`` (float64 search on the host, over sub-pixel shifts)."""
    ext = r.batch["tar_ext"][0].double().cpu().numpy()
    K = r.batch["tar_ixt"][0].double().cpu().numpy()
    (w, h), c = r.sizes[0], r.case
    depth = float(r.batch["near_far"][0, 0].mean())
    inv = np.linalg.inv(ext)
    for dx in np.arange(-1.5, 1.5, 0.0625):
        for dy in np.arange(-1.5, 1.5, 0.0625):
            u, v = want_xy[0] + w / 2 + dx, want_xy[1] + h / 2 + dy
            cam = np.array([(u - K[0, 2]) / K[0, 0] * depth, (v - K[1, 2]) / K[1, 1] * depth, depth, 1.0])
            centre = (inv @ cam)[:3]
            half = 0.3 * (w / 2) * depth / K[0, 0]
            bounds = np.array([[centre - half, centre + half]])
            ref = boxes_reference(bounds, ext, K, c["H"], c["W"], r.sizes, 0.0)
            frac = np.abs(ref[3] - np.floor(ref[3]) - 0.5)
            if tuple(ref[0][0]) == tuple(float(q) for q in want_xy) and ref[2] == [0] and float(frac.min()) > 1e-2:
                return bounds
    raise AssertionError("no box lands at the wanted position")


def graph_case(lib, dev):
    from enerf_amd.graph import GraphedFrame
    name = "b"
    r = rig(lib, dev, name)
    c = r.case
    H, W = c["H"], c["W"]
    own = POSITIONS[name][0][0]
    bounds = torch.from_numpy(_bounds_landing_at(r, own).astype(np.float32)).to(dev)
    cache = r.cache(r.mov)
    seen = {}

    def loop(b):
        xy, _, flags = lib.layer_boxes(b["bounds"], b["tar_ext"], b["tar_ixt"], H, W, r.sizes)
        out = dict(r.mov.forward_cached(cache, r.view_idx, dict(b, bbox_xy=xy)))
        out["bbox_xy"], out["box_flags"] = xy, flags
        return out

    base = dict(r.tar, bounds=bounds, bbox_size=r.sizes)
    shifts = [(0.0, 0.0), (22.0, 0.0), (-38.0, 12.0), (10.0, -17.0), (-20.0, -9.0)]       # the camera moves: the box lands elsewhere
    batches = []
    for sx, sy in shifts:
        ext = r.tar["tar_ext"].clone()
        ext[0, 0, 3] += sx
        ext[0, 1, 3] += sy
        batches.append(dict(base, tar_ext=ext))
    with torch.no_grad():
        eager = [{k: v.clone() for k, v in loop(b).items()} for b in batches]
    torch.cuda.synchronize()
    landed = [tuple(e["bbox_xy"].cpu().reshape(-1).tolist()) for e in eager]
    assert landed[0] == tuple(float(q) for q in own), (landed, "captured at the fixture's own position")
    assert len(set(landed)) == len(landed), (landed, "every camera's box lands somewhere else")
    # the eager frame at the own position is the frame of the position given directly
    direct = r.moving([own], cached=True)[0]
    for k in direct:
        _same(eager[0][k], direct[k], ("eager, own position", k))
    frame = GraphedFrame(r.mov, batches[0], fn=loop)
    graph = frame.graph
    for n, (b, e) in enumerate(list(zip(batches[1:], eager[1:])) + [(batches[0], eager[0])]):
        out = frame(b)
        torch.cuda.synchronize()
        for k in e:
            _same(out[k], e[k], ("replay", n, k))
    assert frame.graph is graph
    with pytest.raises(RuntimeError, match="bbox_size"):
        frame(dict(batches[1], bbox_size=[(64, 32)]))
    # with bbox the graph still refuses a moved box
    boxed = dict(r.tar, bbox=torch.tensor([[(own[0], own[1]) + tuple(r.sizes[0])]], dtype=torch.float32))
    host_frame = GraphedFrame(r.host, boxed, fn=lambda b: r.host.forward_cached(r.cache(r.host), r.view_idx, b))
    with pytest.raises(RuntimeError, match=r"batch\['bbox'\] changed"):
        host_frame(dict(boxed, bbox=torch.tensor([[(own[0] + 1, own[1]) + tuple(r.sizes[0])]], dtype=torch.float32)))


def no_sync_case(lib, dev, name="b"):
    """Under ``torch.cuda.set_sync_debug_mode("error")`` an implicit synchronisation raises: a frame with device positions has none."""
    r = rig(lib, dev, name)
    pos = r.xy(POSITIONS[name][3])
    ref = r.moving(POSITIONS[name][3], cached=True)[0]
    b = dict(r.tar, bbox_size=r.sizes, bbox_xy=pos)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.no_grad():
            out = r.mov.forward_cached(r.cache(r.mov), r.view_idx, b)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    for k in ref:
        _same(out[k], ref[k], ("no sync", k))


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. refusals
def _moving_args(r):
    r.mov._shapes.clear()
    r.moving(POSITIONS[r.name][0])
    (st,) = r.mov._shapes.values()
    return CompositeFrameArgs.from_buffer_copy(st["call.args"]), st


def network_refusals_case(lib, dev):
    r = rig(lib, dev, "b")
    own = POSITIONS["b"][0]
    both = dict(r.batch, bbox=torch.tensor([[(32, 16, 32, 32)]], dtype=torch.float32), bbox_size=r.sizes, bbox_xy=r.xy(own))
    with pytest.raises(ValueError, match="not both"):
        r.mov(both)
    with pytest.raises(ValueError, match=r"\(w, h\) for 1 layers"):
        r.mov(dict(r.batch, bbox_size=[(32, 32), (32, 32)], bbox_xy=r.xy(own)))
    with pytest.raises(ValueError, match="needs batch\\['bbox_xy'\\]"):
        r.mov(dict(r.batch, bbox_size=r.sizes))
    with pytest.raises(ValueError, match=r"must be \(1, 2\) or \(1, 1, 2\)"):
        r.mov(dict(r.batch, bbox_size=r.sizes, bbox_xy=r.xy([(1, 2), (3, 4)])))
    with pytest.raises(EnerfError, match="w > W"):
        r.moving(own, sizes=[(128, 32)])
    with pytest.raises(EnerfError, match="h > H"):
        r.moving(own, cached=True, sizes=[(32, 96)])
    with pytest.raises(EnerfError, match="divisible by 4"):                  # an existing refusal, evaluated for the box (0, 0, w, h)
        r.moving(own, sizes=[(48, 32)])
    staged = _load(lib, dev, "b", driver="staged")
    with pytest.raises(RuntimeError, match="no staged form"):
        staged(dict(r.batch, bbox_size=r.sizes, bbox_xy=r.xy(own)))
    r.mov.stage_hook = lambda stage: None
    try:
        with pytest.raises(RuntimeError, match="stage_hook"):
            r.mov(dict(r.batch, bbox_size=r.sizes, bbox_xy=r.xy(own)))
    finally:
        r.mov.stage_hook = None
    trainable = _load(lib, dev, "b", trainable=True).train()
    with pytest.raises(ValueError, match="training path takes batch\\['bbox'\\] only"):
        trainable(dict(r.batch, bbox_size=r.sizes, bbox_xy=r.xy(own)))
    assert_frames_equal(r.moving(own), r.on_host(own), "a good frame after the refused ones", flags=[0])


def c_refusals_case(lib, dev, traced):
    """Through the C entries and enerf_last_error(); ``traced`` (emulator): nothing was enqueued."""
    import contextlib
    r = rig(lib, dev, "b")
    a, keep = _moving_args(r)
    xy, flags = r.xy(POSITIONS["b"][0]), torch.zeros(1, dtype=torch.int32, device=dev)
    k = r.cache(r.mov).struct

    def refused(call, names, prefix):
        if traced:
            from emu_lib import emu_trace
            ctx = emu_trace(lib)
        else:
            ctx = contextlib.nullcontext([])
        with ctx as tr:
            rc = call()
        msg = lib.dll.enerf_last_error().decode()
        assert rc == EINVAL and re.search(names, msg) and msg.startswith(prefix), (rc, msg)
        assert tr == [], tr

    dll = lib.dll
    refused(lambda: dll.enerf_forward_composite_moving(C.byref(a), None, flags.data_ptr(), None), "null bbox_xy", "forward_composite_moving:")
    refused(lambda: dll.enerf_forward_composite_cached_moving(C.byref(a), C.byref(k), r.view_idx.data_ptr(), None, None, None),
            "null bbox_xy", "forward_composite_moving:")
    refused(lambda: dll.enerf_forward_composite_cached_moving(C.byref(a), None, r.view_idx.data_ptr(), xy.data_ptr(), None, None),
            "null cache", "forward_composite_cached:")
    refused(lambda: dll.enerf_forward_composite_moving(None, xy.data_ptr(), None, None), "null args", "forward_composite:")
    wide = CompositeFrameArgs.from_buffer_copy(a)
    wide.bbox[0][2] = 128.0
    refused(lambda: dll.enerf_forward_composite_moving(C.byref(wide), xy.data_ptr(), None, None), r"bbox\[0\].*128 x 32.*w > W", "forward_composite_moving:")
    assert dll.enerf_forward_composite_moving_workspace_bytes(C.byref(wide)) == 0
    assert dll.enerf_forward_composite_cached_moving_workspace_bytes(C.byref(wide), C.byref(k)) == 0
    tall = CompositeFrameArgs.from_buffer_copy(a)
    tall.bbox[0][3] = 68.0
    refused(lambda: dll.enerf_forward_composite_moving(C.byref(tall), xy.data_ptr(), None, None), r"bbox\[0\].*32 x 68.*h > H", "forward_composite_moving:")
    # bbox[l][0..1] are ignored: a position in the argument block that the host entry would refuse changes nothing
    far = CompositeFrameArgs.from_buffer_copy(a)
    far.bbox[0][0], far.bbox[0][1] = 500.0, -3.0
    assert dll.enerf_forward_composite_moving_workspace_bytes(C.byref(far)) == keep["call.ws"].numel() * 4
    lib._check(dll.enerf_forward_composite_moving(C.byref(far), xy.data_ptr(), None, None), "forward_composite_moving")      # flags are optional
    _same(keep["call.outs"]["rgb_level1"], r.on_host(POSITIONS["b"][0])[0]["rgb_level1"], "ignored bbox[l][0..1]")
    # the _at entries: a null corner, a window larger than the grid
    z = torch.zeros(4096, device=dev)
    refused(lambda: dll.enerf_build_feature_volume_window_at(z.data_ptr(), z.data_ptr(), z.data_ptr(), 1, 2, 16, 8, 12, 4, 8, 12, None, 4, 4,
                                                             z.data_ptr(), None), "null xy", "build_feature_volume_window_at:")
    refused(lambda: dll.enerf_depth_regression_window_at(z.data_ptr(), z.data_ptr(), 1, 4, 8, 12, flags.data_ptr(), 16, 4, 1, z.data_ptr(),
                                                         z.data_ptr(), None), "outside", "depth_regression_window_at:")
    refused(lambda: dll.enerf_composite_layers_at(None, None, None), "null win_xy", "composite_layers_at:")
    refused(lambda: dll.enerf_layer_boxes(z.data_ptr(), z.data_ptr(), z.data_ptr(), 5, 64, 96, (C.c_int * 10)(), 0.0, z.data_ptr(), z.data_ptr(),
                                          flags.data_ptr(), None), "L=5", "layer_boxes:")
    del keep
