"""Cases of the composite network's one-call driver (csrc/frame.hip CompositeRun, enerf_forward_composite) and of its preparation
kernel (k_composite_prep, enerf_composite_prep), shared by the emulator tests (test_composite_driver.py) and the MI355X tests
(test_composite_driver_gpu.py): every function takes the library and the device and asserts.

    prep_case          every output of the one preparation launch holds the bits of enerf_get_proj_mats, enerf_get_depth_values
                       (level 0) and enerf_window_ray_index called per level / cascade / window
    driver_case        Network(driver="staged") — one C call per stage, the path the reference fixtures check — against the default,
                       one enerf_forward_composite per frame: same keys, torch.equal on every output and every depth / std map
    boxes_case         a frame with other boxes (a new shape) and back
    trace properties   (emulator) which kernels run, where, and the fork / join discipline, on the launch trace
    refusal_case       everything the host can check is refused with its code and a message naming the field, nothing enqueued
    graph_case         (GPU) GraphedFrame replays equal the eager frame

Shapes: composite_cases.NETWORK_CASES "a" (L = 2, S = 3, both levels rendered) and "b" (L = 1, S = 2, last level only) at 64 x 96,
plus two unaligned boxes, L = 1, both levels rendered.  "u" is (36, 8, 64, 32): 36 * 0.125 = 4.5 truncates to 4, so its level-0
window (4, 1, 8, 4) just fits the 12-wide grid — but the box itself ends at x = 100 in a 96-wide image, and level 1's window
(18, 4, 32, 16) ends at 50 in the 48-wide grid (the render windows at 25 of 24 and 100 of 96): every path refuses that frame,
the staged one at its first window call, the one-call driver before it launches anything (unaligned_box_outside_case).  "v" is the
same corner with a box that stays inside, (36, 8, 32, 32): windows (4, 1, 4, 4) and (18, 4, 16, 16), run like "a" and "b".  Weights are the modules' seeded initialisation: the acceptance bar is bit-identity of
two drivers over the same kernels, the reference's values are test_composite.py's business."""
import ctypes as C
import os
import sys
from collections import Counter

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import composite_cases as CC
from enerf_amd.config import EnerfConfig
from enerf_amd.lib import CompositeFrameArgs, CompositePrepArgs, EnerfError, Options
from enerf_amd.network_composite import BG_PLANES, Network, _scaled_box
from enerf_amd.synth import make_batch

CASES = dict(CC.NETWORK_CASES)
CASES["u"] = dict(H=64, W=96, S=3, L=1, render_if=(True, True), boxes=[(36, 8, 64, 32)], ranges=[(0.3, 0.8), (0.0, 1.0)], seed=23)
CASES["v"] = dict(CASES["u"], boxes=[(36, 8, 32, 32)])
RUN_CASES = ("a", "b", "v")
OTHER_BOXES = {"a": [(0, 16, 32, 32), (48, 32, 32, 32)], "b": [(0, 0, 64, 32)], "v": [(20, 24, 32, 32)]}
LANE_STREAMS = ("side", "render")
EINVAL, EWORKSPACE = -1, -3


def config(name):
    return EnerfConfig(viewdir_agg=False).with_cas(volume_planes=(32, 8), num_samples=(2, 1), render_if=CASES[name]["render_if"])


def batch_np(name, H=None, W=None):
    """composite_cases.network_batch for every case of this file (and, for the refusals, other image sizes)."""
    c = CASES[name]
    b = make_batch(H or c["H"], W or c["W"], c["S"], config(name), seed=c["seed"], textured=True)
    n, f = float(b["near_far"][0, 0]), float(b["near_far"][0, 1])
    b["near_far"] = np.array([[(n + lo * (f - n), n + hi * (f - n)) for lo, hi in c["ranges"]]], np.float32)
    b["bbox"] = np.array([c["boxes"]], np.float32)
    b["bg_src_inps"] = np.random.default_rng(c["seed"] + 100).uniform(-1, 1, size=b["src_inps"].shape).astype(np.float32)
    return b


def _same(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert torch.equal(a, b), (what, float((a - b).abs().max()))


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the preparation kernel alone
def prep_case(lib, dev, depth_inv, big=False):
    """L = 2, foreground D = 32, background D = 16, the cascade's two levels; level 0's raster has windows (one touching the
    right and bottom edges), and so has level 1's when depth_inv is on — off, level 1 has none (a level that is not rendered).
    ``big``: a 32 x 48 grid (49152 and 24576 plane elements) and a 128 x 128 window (16384 rays) — jobs past the 32 blocks x 256
    threads a job gets, so that every thread strides over several elements, as at every real image size; beside them a job of 35
    elements and one of 8192 + 2."""
    cas = EnerfConfig().cas
    b = {k: torch.from_numpy(v).to(dev) for k, v in make_batch(64, 96, 3, EnerfConfig(), seed=31).items()}
    n, f = float(b["near_far"][0, 0]), float(b["near_far"][0, 1])
    near_far = torch.tensor([(n + lo * (f - n), n + hi * (f - n)) for lo, hi in ((0.5, 0.9), (0.1, 0.4), (0.0, 1.0))], dtype=torch.float32, device=dev)
    h, w, L = (32, 48, 2) if big else (8, 12, 2)
    scales = [(cas.im_feat_scale[i], cas.volume_scale[i]) for i in range(2)]
    rasters = [(16, 24), (64, 96) if depth_inv else None]
    windows = [[(16, 8, 8, 8), (0, 0, 5, 7)], [(32, 0, 64, 64), (3, 5, 33, 17)]]
    if big:
        rasters = [(128, 192), (256, 384)]
        windows = [[(64, 0, 128, 128), (0, 0, 5, 7)], [(1, 10, 241, 34), (100, 56, 284, 200)]]
    proj, dv, nf, index = lib.composite_prep(b["src_ixts"], b["src_exts"], b["tar_ixt"], b["tar_ext"], near_far, scales, 32, 16, h, w,
                                             depth_inv, rasters, windows)
    for i, (ss, ts) in enumerate(scales):
        _same(proj[i], lib.get_proj_mats(b["src_ixts"], b["src_exts"], b["tar_ixt"], b["tar_ext"], ss, ts), ("proj", i))
    for c in range(L + 1):
        D = 32 if c < L else 16
        want = lib.get_depth_values(near_far[c:c + 1].contiguous(), None, 1, D, h, w, depth_inv)
        _same(dv[c], want[0], ("dv", c, depth_inv))
        _same(nf[c], want[1], ("nf", c, depth_inv))
        assert float(dv[c].min()) > 0
    for i, ras in enumerate(rasters):
        if ras is None:
            assert index[i] is None
            continue
        for l in range(L):
            want = lib.window_ray_index(windows[i][l], ras[0], ras[1], dev)
            _same(index[i][l][0], want[0], ("index", i, l))
            _same(index[i][l][1], want[1], ("count", i, l))
            assert int(want[1].cpu()) == windows[i][l][2] * windows[i][l][3]


def prep_refusals(lib, dev):
    with pytest.raises(EnerfError, match="null args"):
        lib._check(lib.dll.enerf_composite_prep(None, None), "composite_prep")
    for L in (0, 5):
        with pytest.raises(EnerfError, match=f"L={L}"):
            lib._check(lib.dll.enerf_composite_prep(C.byref(CompositePrepArgs(L=L, S=3, num_levels=2)), None), "composite_prep")
    with pytest.raises(EnerfError, match="null camera"):
        lib._check(lib.dll.enerf_composite_prep(C.byref(CompositePrepArgs(L=1, S=3, num_levels=2)), None), "composite_prep")
    b = {k: torch.from_numpy(v).to(dev) for k, v in make_batch(64, 96, 3, EnerfConfig(), seed=31).items()}
    nf2 = b["near_far"].repeat(2, 1).contiguous()
    with pytest.raises(EnerfError, match="outside"):
        lib.composite_prep(b["src_ixts"], b["src_exts"], b["tar_ixt"], b["tar_ext"], nf2, [(0.25, 0.125)], 8, 8, 8, 12, True, [(16, 24)],
                           [[(20, 0, 8, 8)]])


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. one call = the staged path
class Pair:
    """The same seeded network twice — driver "staged" and the default — one batch, and the staged frame computed once."""

    def __init__(self, lib, dev, name):
        c = CASES[name]
        self.name, self.lib, self.dev, self.case = name, lib, dev, c
        torch.manual_seed(500 + c["seed"])
        self.staged = Network(config(name), c["L"], lib=lib, driver="staged")
        g = torch.Generator().manual_seed(c["seed"])
        with torch.no_grad():                   # BatchNorm statistics other than the identity
            for k, v in self.staged.state_dict().items():
                if k.endswith("running_mean"):
                    v.copy_(torch.randn(v.shape, generator=g) * 0.1)
                elif k.endswith("running_var"):
                    v.copy_(torch.rand(v.shape, generator=g) + 0.5)
        self.call = Network(config(name), c["L"], lib=lib)
        assert self.call.driver == "call"
        self.call.load_state_dict(self.staged.state_dict())
        self.staged, self.call = self.staged.to(dev).eval().prepare(), self.call.to(dev).eval().prepare()
        self.batch = self.make_batch(c["boxes"])
        self.ref = self.run(self.staged, self.batch)
        assert float(self.ref[0][f"rgb_level{config(name).cas.num - 1}"].abs().max()) > 0

    def make_batch(self, boxes):
        b = {k: torch.from_numpy(v).to(self.dev) for k, v in batch_np(self.name).items()}
        b["bbox"] = torch.tensor([boxes], dtype=torch.float32)               # on the host: no readback in the frame
        return b

    @staticmethod
    def run(net, batch, options=None):
        """(outputs, intermediates) of one frame, cloned: the next frame of the shape overwrites the buffers."""
        net.options = options
        with torch.no_grad():
            out = net(batch)
            return {k: v.clone() for k, v in out.items()}, {k: v.clone() for k, v in net.intermediates.items()}


_PAIRS = {}


def pair(lib, dev, name):
    key = (name, dev.type)
    if key not in _PAIRS:
        _PAIRS[key] = Pair(lib, dev, name)
    return _PAIRS[key]


def assert_frames_equal(got, ref, what):
    assert sorted(got[0]) == sorted(ref[0]) and sorted(got[1]) == sorted(ref[1]), what
    assert not any(k.startswith("idx") for k in got[0])
    for part, r in zip(got, ref):
        for k in r:
            _same(part[k], r[k], (what, k))


def driver_case(lib, dev, name, frames=1):
    """The default driver against the staged path: with the lane, on one stream, and (``frames`` > 1: the GPU, where chains really
    overlap) several frames in a row with the lane on — the only check that can see a scratch region shared across the fork."""
    p = pair(lib, dev, name)
    c = p.case
    cas = config(name).cas
    want_keys = {f"{k}_level{i}" for i in range(cas.num) if cas.render_if[i] for k in ("rgb", "depth", "weights", "net_output", "z_vals")}
    assert set(p.ref[0]) == want_keys
    assert set(p.ref[1]) == {f"{m}_{i}_{who}" for i in range(cas.num) for m in ("depth", "std")
                             for who in [f"layer{l}" for l in range(c["L"])] + ["bg"]}
    first = p.run(p.call, p.batch)
    assert_frames_equal(first, p.ref, (name, "lane"))
    for n in range(1, frames):
        assert_frames_equal(p.run(p.call, p.batch), first, (name, "lane, frame", n))
    assert_frames_equal(p.run(p.call, p.batch, Options(single_stream=1)), p.ref, (name, "single_stream"))
    assert_frames_equal(p.run(p.staged, p.batch, Options(single_stream=1)), p.ref, (name, "staged, single_stream"))


def boxes_case(lib, dev, name):
    """A frame with other boxes — a new shape: new windows, new workspace — and the first boxes again."""
    p = pair(lib, dev, name)
    other = p.make_batch(OTHER_BOXES[name])
    assert_frames_equal(p.run(p.call, other), p.run(p.staged, other), (name, "other boxes"))
    assert_frames_equal(p.run(p.call, p.batch), p.ref, (name, "first boxes again"))


def unaligned_box_outside_case(lib, dev):
    """Case "u": the windows are what the float32 product and the truncation make them — (4, 1, 8, 4) at level 0, named in the
    refusal of level 1's (18, 4, 32, 16), which leaves the 48 x 32 grid — and both drivers refuse the frame."""
    from emu_lib import emu_trace
    p = pair(lib, dev, "v")
    cas = config("u").cas
    box = CASES["u"]["boxes"][0]
    assert _scaled_box(box, cas.volume_scale[0]) == (4, 1, 8, 4) and _scaled_box(box, cas.volume_scale[1]) == (18, 4, 32, 16)
    batch = p.make_batch(CASES["u"]["boxes"])
    with pytest.raises(EnerfError, match="outside"):
        p.run(p.staged, batch)
    with pytest.raises(EnerfError, match=r"bbox\[0\] at level 0 is the window \(x0 9, y0 2, 16 x 8\), outside the 24 x 16 ray raster"):
        with emu_trace(lib) as tr:
            p.run(p.call, batch)
    assert tr == []


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. trace helpers (tests/test_frame_driver.py's, re-stated): a trace is a list of ("launch", kernel, grid, stream) |
# ("record", event, stream) | ("wait", event, stream)
def launches(tr, prefix, stream=None):
    return [i for i, r in enumerate(tr) if r[0] == "launch" and r[1].lstrip("(").startswith(prefix) and stream in (None, r[3])]


def source_of_wait(tr, w):
    """Index of the record a wait binds to: the last record of its event before it (None: never recorded in this call)."""
    for i in range(w - 1, -1, -1):
        if tr[i][0] == "record" and tr[i][1] == tr[w][1]:
            return i
    return None


def waits(tr, stream, event=None):
    return [i for i, r in enumerate(tr) if r[0] == "wait" and r[2] == stream and event in (None, r[1])]


def check_fork_join(tr):
    """No wait on an event this call did not record; a lane stream starts behind the caller's stream; the caller's stream leaves
    behind every lane stream."""
    for w in waits(tr, "main") + waits(tr, "side") + waits(tr, "render"):
        assert source_of_wait(tr, w) is not None, ("wait on an event not recorded in this call", w, tr[w])
    for s in LANE_STREAMS:
        on_s = [i for i, r in enumerate(tr) if r[0] == "launch" and r[3] == s]
        if not on_s:
            continue
        forks = [w for w in waits(tr, s) if w < on_s[0] and tr[source_of_wait(tr, w)][2] == "main"]
        assert forks, (s, "launches before it waited on the caller's stream")
        joins = [w for w in waits(tr, "main") if tr[source_of_wait(tr, w)][2] == s and source_of_wait(tr, w) > on_s[-1]]
        assert joins, (s, "the caller's stream returns without waiting for its last launch")
    assert all(r[3] in ("main",) + LANE_STREAMS for r in tr if r[0] == "launch"), "a launch on an unknown stream"


def kernel_names(tr):
    return Counter(r[1] for r in tr if r[0] == "launch")


def traced(lib, net, batch, options):
    from emu_lib import emu_trace
    net.options = options
    with torch.no_grad(), emu_trace(lib) as tr:
        net(batch)
    return tr


def staged_minus_prep(tr, name):
    """The staged frame's kernels without the launches k_composite_prep replaces — get_proj_mats of every level, level 0's
    get_depth_values of every cascade, the windows' ray lists (which the staged path fills on a shape's first frame only) — plus
    the one launch that replaces them."""
    c, cas = CASES[name], config(name).cas
    names = kernel_names(tr)
    assert names["k_proj_mats"] == cas.num and names["k_depth_values"] == cas.num * (c["L"] + 1)
    assert names["k_window_ray_index"] in (0, c["L"] * sum(cas.render_if))
    names = names - Counter({"k_proj_mats": cas.num, "k_depth_values": c["L"] + 1, "k_window_ray_index": names["k_window_ray_index"]})
    return names + Counter({"k_composite_prep": 1})


def trace_case(lib, dev, name):
    p = pair(lib, dev, name)
    c, cas = p.case, config(name).cas
    want = staged_minus_prep(traced(lib, p.staged, p.batch, None), name)
    # ---- one stream: launches only, all on the caller's stream ----
    one = traced(lib, p.call, p.batch, Options(single_stream=1))
    assert not [r for r in one if r[0] != "launch"] and {r[3] for r in one} == {"main"}
    assert kernel_names(one) == want, (kernel_names(one) - want, want - kernel_names(one))
    assert launches(one, "k_composite_prep") == [0] and one[0][2][0] <= 600
    # ---- with the lane ----
    tr = traced(lib, p.call, p.batch, None)
    assert kernel_names(tr) == want, (kernel_names(tr) - want, want - kernel_names(tr))
    check_fork_join(tr)
    prep = launches(tr, "k_composite_prep")
    records = [i for i, r in enumerate(tr) if r[0] == "record"]
    assert len(prep) == 1 and tr[prep[0]][3] == "main" and records and prep[0] < records[0], "the prep launch precedes every record"
    # the foreground's FeatureNet and its layers are on the lane, the background's stay with the caller
    assert len(launches(tr, "k_conv0_fused_cb", "side")) == 1 and len(launches(tr, "k_conv0_fused_cb", "main")) == 1
    vols = launches(tr, "k_feature_volume")
    on_lane = [v for v in vols if tr[v][3] in LANE_STREAMS]
    assert len(vols) == cas.num * (c["L"] + 1) and len(on_lane) == cas.num * c["L"]
    assert all("true" in tr[v][1] for v in on_lane) and not any("true" in tr[v][1] for v in vols if tr[v][3] == "main")   # <.., true>: windowed
    if c["L"] >= 2:
        assert {tr[v][3] for v in on_lane} == set(LANE_STREAMS), "two layers: one per lane stream"
    # every rendered level's merge is behind a join of each lane stream that carried one of the level's raw renders
    merges = launches(tr, "k_composite_layers")
    renders = launches(tr, "k_render_rays")
    assert len(merges) == sum(cas.render_if) and all(tr[m][3] == "main" for m in merges)
    assert len(renders) == len(merges) * (c["L"] + 1)
    lo = 0
    for m in merges:
        mine = [r for r in renders if lo < r < m]
        assert len(mine) == c["L"] + 1 and sum(tr[r][3] == "main" for r in mine) == 1
        for s in {tr[r][3] for r in mine} - {"main"}:
            last = max(i for i in range(m) if tr[i][0] == "launch" and tr[i][3] == s)
            joined = [w for w in waits(tr, "main") if w < m and tr[source_of_wait(tr, w)][2] == s and source_of_wait(tr, w) > last]
            assert joined, (name, "merge of the level before its layers' lane stream", s, "was joined")
        lo = m


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. refusals
def _args_of(p):
    """A private copy of the argument block the network built for the pair's shape (the pointers stay the network's)."""
    key = next((k for k, v in p.call._shapes.items() if k[3] == tuple(tuple(float(x) for x in b) for b in p.case["boxes"]) and "call.args" in v), None)
    if key is None:
        p.run(p.call, p.batch)
        key = list(p.call._shapes)[-1]                   # (most recently used last)
    st = p.call._shapes[key]
    return CompositeFrameArgs.from_buffer_copy(st["call.args"]), st


def _set_box(a, l, box):
    for k in range(4):
        a.bbox[l][k] = float(box[k])


REFUSALS = {      # name -> (mutation of a valid argument block, error code, what the message must name)
    "src_inps": (lambda a: setattr(a, "src_inps", None), EINVAL, "src_inps"),
    "tar_ext": (lambda a: setattr(a, "tar_ext", None), EINVAL, "tar_ext"),
    "near_far": (lambda a: setattr(a, "near_far", None), EINVAL, "near_far"),
    "feature_net_bg_packed": (lambda a: setattr(a, "feature_net_bg_packed", None), EINVAL, "feature_net_bg_packed"),
    "cost_reg_packed": (lambda a: a.cost_reg_packed[1].__setitem__(1, None), EINVAL, r"cost_reg_packed\[1\]\[1\]"),
    "nerf_packed": (lambda a: a.nerf_packed[1].__setitem__(0, None), EINVAL, r"nerf_packed\[1\]\[0\]"),
    "output": (lambda a: a.weights.__setitem__(1, None), EINVAL, "level 1 output"),
    "workspace": (lambda a: setattr(a, "workspace", None), EINVAL, "workspace is null"),
    "L=0": (lambda a: setattr(a, "L", 0), EINVAL, "L=0"),
    "L=5": (lambda a: setattr(a, "L", 5), EINVAL, "L=5"),
    "Ns=9": (lambda a: a.cas.num_samples.__setitem__(1, 9), EINVAL, r"cas.num_samples\[1\]=9"),
    "L*Ns": (lambda a: (setattr(a, "L", 3), a.cas.num_samples.__setitem__(1, 6)), EINVAL, r"L \* num_samples = 3 \* 6"),
    "window outside": (lambda a: _set_box(a, 0, (64, 16, 64, 32)), EINVAL, r"bbox\[0\].*outside"),
    "ww=6": (lambda a: _set_box(a, 0, (32, 16, 48, 32)), EINVAL, r"bbox\[0\] at level 0 is a 6 x 4 window.*divisible by 4"),
    "D": (lambda a: a.cas.volume_planes.__setitem__(0, 30), EINVAL, r"cas.volume_planes\[0\]=30"),
    "bg D": (lambda a: a.bg_volume_planes.__setitem__(1, 6), EINVAL, r"bg_volume_planes\[1\]=6"),
    "levels": (lambda a: a.bg_volume_planes.__setitem__(1, 0), EINVAL, "bg_volume_planes covers 1"),
    "48x80": (lambda a: (setattr(a, "H", 48), setattr(a, "W", 80)), EINVAL, r"h, w \(6, 10\) of H, W \(48, 80\) must be divisible by 4"),
    "S": (lambda a: setattr(a, "S", 5), EINVAL, "S=5"),
    "small workspace": (lambda a: setattr(a, "workspace_bytes", a.workspace_bytes - 256), EWORKSPACE, "workspace too small"),
}


def refusal_case(lib, dev, which):
    """Case "b" with one field spoiled: the code, the field in the message, and nothing enqueued."""
    import re
    from emu_lib import emu_trace
    p = pair(lib, dev, "b")
    a, keep = _args_of(p)
    mutate, code, names = REFUSALS[which]
    mutate(a)
    with emu_trace(lib) as tr:
        rc = lib.dll.enerf_forward_composite(C.byref(a), None)
    msg = lib.dll.enerf_last_error().decode()
    assert rc == code, (which, rc, msg)
    assert re.search(names, msg) and msg.startswith("forward_composite:"), (which, msg)
    assert tr == [], (which, tr)
    if code == EINVAL and which != "workspace":           # (the size query does not look at the workspace)
        assert lib.dll.enerf_forward_composite_workspace_bytes(C.byref(a)) == 0
    del keep


def refusal_null_args(lib, dev):
    from emu_lib import emu_trace
    with emu_trace(lib) as tr:
        assert lib.dll.enerf_forward_composite(None, None) == EINVAL
    assert "null args" in lib.dll.enerf_last_error().decode() and tr == []
    assert lib.dll.enerf_forward_composite_workspace_bytes(None) == 0


def refusal_through_the_network(lib, dev):
    """A 48 x 80 frame (level 0's grid is 6 x 10) and a box whose level-0 window is 6 wide: Network.forward raises what the plan
    says, and the frame has enqueued nothing."""
    from emu_lib import emu_trace
    p = pair(lib, dev, "b")
    small = {k: torch.from_numpy(v).to(dev) for k, v in batch_np("b", 48, 80).items()}
    small["bbox"] = torch.tensor([[(16, 16, 32, 16)]], dtype=torch.float32)
    for batch, names in ((small, "divisible by 4"), (p.make_batch([(32, 16, 48, 32)]), r"bbox\[0\].*6 x 4 window")):
        with pytest.raises(EnerfError, match=names):
            with torch.no_grad(), emu_trace(lib) as tr:
                p.call(batch)
        assert tr == []
    assert_frames_equal(p.run(p.call, p.batch), p.ref, "a good frame after the refused ones")


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. HIP graph (GPU only)
def graph_case(lib, dev, name):
    from enerf_amd.graph import GraphedFrame
    p = pair(lib, dev, name)
    net = Network(config(name), p.case["L"], lib=lib)
    net.load_state_dict(p.staged.state_dict())
    net = net.to(dev).eval().prepare()
    on_device = dict(p.batch)
    on_device["bbox"] = p.batch["bbox"].to(dev)
    with pytest.raises(RuntimeError, match="bbox"):
        GraphedFrame(net, on_device)
    frame = GraphedFrame(net, p.batch)
    moved = dict(p.batch)
    moved["tar_ext"] = p.batch["tar_ext"].clone()
    moved["tar_ext"][0, 0, 3] += 0.02
    for n, batch in enumerate((p.batch, moved)):
        with torch.no_grad():
            got = {k: v.clone() for k, v in frame(batch).items()}
        eager = p.run(p.call, batch)[0]
        assert sorted(got) == sorted(eager)
        for k in eager:
            _same(got[k], eager[k], (name, "replay", n, k))
    assert not torch.equal(got[f"rgb_level{config(name).cas.num - 1}"], p.ref[0][f"rgb_level{config(name).cas.num - 1}"]), "the camera moved"
    other = p.make_batch(OTHER_BOXES[name])
    with pytest.raises(RuntimeError, match="bbox"):
        frame(other)
