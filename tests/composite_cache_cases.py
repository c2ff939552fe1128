"""Cases of the composite network's source-view cache (enerf_composite_cache_build, enerf_composite_prep_indexed,
enerf_forward_composite_cached; Network.cache_sources / forward_cached of network_composite.py), shared by the emulator tests
(test_composite_cache.py) and the MI355X tests (test_composite_cache_gpu.py): every function takes the library and the device and
asserts.  Nothing here has a tolerance: a FeatureNet's maps of an image do not depend on the other images of the call, a gather
copies bits, and the indexed preparation runs the stand-alone preparation's arithmetic on the indexed rows.

    build_case         every buffer of both nets == ONE FeatureNet + texel-pack call over all V images, whatever the chunk
    indexed_prep_case  enerf_composite_prep on hand-gathered cameras == enerf_composite_prep_indexed on the (V,...) tables
    frame_case         forward_cached == forward on the views gathered by hand: every output, every depth / std map, lane and one stream
    rebuild_case       rebuild in place == a fresh cache; bg_inps=None keeps the colours; stale / empty caches are refused
    trace_case         (emulator) no FeatureNet, no texel pack, one preparation launch, two gathers; otherwise the uncached frame's kernels
    refusal_case       (emulator) everything the host can check about a cache, and two of the frame's own refusals through the cached entry
    out_of_range_case  (emulator) an index outside [0, V) gives NaN, not a wild read
    graph_case, no_sync_case, uint8_case   (GPU)

Shapes: composite_driver_cases.CASES "a", "b" and "v" at 64 x 96 with that file's seeded weights and randomised BN statistics; V = 5
cached views of one make_batch(64, 96, 5, ...) rig — a remainder chunk of one image, three chunks at chunk=2 — whose intrinsics are
made to differ per view (the synthetic rig shares one K), and an independent uniform image as bg_inps."""
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

import composite_driver_cases as DC
from enerf_amd.composite_cache import CompositeSourceCache
from enerf_amd.config import EnerfConfig
from enerf_amd.lib import CompositeCacheStruct, CompositeFrameArgs, EnerfError, Options, cascade_struct
from enerf_amd.synth import look_at_w2c, make_batch

V, H, W = 5, 64, 96
INDEX_ROWS = {3: ([4, 0, 2], [3, 3, 1], [0, 1, 2]), 2: ([4, 0], [2, 2], [0, 1])}
PREP_ROWS = ([4, 0, 2], [3, 3, 1], [0, 1, 2])
EINVAL, EWORKSPACE = DC.EINVAL, DC.EWORKSPACE


def _same(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert torch.equal(a, b), (what, float((a - b).abs().max()))


def views_np(name, seed_offset=0):
    """(inps, bg_inps, exts, ixts) of V views and the target side of the batch, as numpy."""
    c = DC.CASES[name]
    b = make_batch(H, W, V, DC.config(name), seed=c["seed"] + 7 + seed_offset, textured=True)
    ixts = b["src_ixts"][0].copy()
    for v in range(V):                      # one K for every view would hide a camera row gathered from the wrong view
        ixts[v, :2, :2] *= 1.0 + 0.01 * v
        ixts[v, 0, 2] += 0.5 * v
    bg = np.random.default_rng(c["seed"] + 300 + seed_offset).uniform(-1, 1, size=(V, 3, H, W)).astype(np.float32)
    n, f = float(b["near_far"][0, 0]), float(b["near_far"][0, 1])
    tar = {k: v for k, v in b.items() if not k.startswith("src_")}
    tar["near_far"] = np.array([[(n + lo * (f - n), n + hi * (f - n)) for lo, hi in c["ranges"]]], np.float32)
    return (b["src_inps"][0], bg, b["src_exts"][0], ixts), tar


class Rig:
    """One seeded network (composite_driver_cases.Pair's weights), V views, a cache built from them, and the target side of a batch."""

    def __init__(self, lib, dev, name):
        p = DC.pair(lib, dev, name)
        self.name, self.lib, self.dev, self.case, self.net = name, lib, dev, p.case, p.call
        views, tar = views_np(name)
        self.views = tuple(torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in views)
        self.tar = {k: torch.from_numpy(v).to(dev) for k, v in tar.items()}
        self.cache = self.net.cache_sources(*self.views)

    def target(self, boxes=None):
        b = dict(self.tar)
        b["bbox"] = torch.tensor([boxes or self.case["boxes"]], dtype=torch.float32)        # on the host: no readback in the frame
        return b

    def by_hand(self, idx, boxes=None, views=None):
        """The batch ``forward`` takes for the index row: the same views gathered on the host."""
        inps, bg, exts, ixts = views or self.views
        r = torch.as_tensor(idx, dtype=torch.long, device=inps.device)
        b = self.target(boxes)
        b.update(src_inps=inps[r][None].contiguous(), bg_src_inps=bg[r][None].contiguous(), src_exts=exts[r][None].contiguous(),
                 src_ixts=ixts[r][None].contiguous())
        return b

    def index(self, idx):
        return torch.tensor(idx, dtype=torch.int32, device=self.dev)

    def cached(self, idx, options=None, boxes=None, cache=None):
        """(outputs, intermediates) of one cached frame, cloned."""
        self.net.options = options
        with torch.no_grad():
            out = self.net.forward_cached(cache or self.cache, self.index(idx), self.target(boxes))
            return {k: v.clone() for k, v in out.items()}, {k: v.clone() for k, v in self.net.intermediates.items()}

    def reference(self, idx, options=None, boxes=None, views=None):
        return DC.Pair.run(self.net, self.by_hand(idx, boxes, views), options)


_RIGS = {}


def rig(lib, dev, name):
    key = (name, dev.type)
    if key not in _RIGS:
        _RIGS[key] = Rig(lib, dev, name)
    return _RIGS[key]


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the build
def expected_buffers(lib, net, views, cas):
    """{buffer name: tensor} from ONE feature_net_stage + pack_texels_cl call per net over all V images."""
    inps, bg, exts, ixts = views
    want = {"exts": exts.reshape(-1), "ixts": ixts.reshape(-1)}
    for who, name, rgb in (("fg", "feature_net", inps), ("bg", "feature_net_bg", bg)):
        bufs = lib.feature_net_alloc(inps)
        lib.feature_net_stage(net._packed_weights(name), inps, bufs, lib.FEAT_ALL)          # BOTH nets read inps
        for i in range(cas.num):
            want[f"{who}_feat{i}"] = bufs[i].reshape(-1)
            if cas.render_if[i]:
                f = bufs[cas.render_im_feat_level[i]]
                want[f"{who}_tex{i}"] = lib.pack_texels_cl(f, rgb, f.shape[1], f.shape[2]).reshape(-1)
                other = lib.pack_texels_cl(f, bg if who == "fg" else inps, f.shape[1], f.shape[2]).reshape(-1)
                assert not torch.equal(other, want[f"{who}_tex{i}"]), "the two images' colours differ"
    return want


def build_case(lib, dev, name):
    r = rig(lib, dev, name)
    cas = DC.config(name).cas
    want = expected_buffers(lib, r.net, r.views, cas)
    assert not any(k.endswith("feat2") for k in want)
    # the sum, written out: per net the level_0 and level_1 maps (no level_2 map), level 0's quarter-size texels of 32 + 3 values
    # padded to 36 where it is rendered, level 1's full-size texels of 8 + 3 padded to 12; the cameras once
    assert cas.num == 2 and cas.render_if[1] and tuple(cas.render_im_feat_level) == (0, 2)
    per_net = V * (16 * 24 * 32 + 32 * 48 * 16) + (V * 16 * 24 * 36 if cas.render_if[0] else 0) + V * 64 * 96 * 12
    floats = 2 * per_net + V * 16 + V * 9
    for chunk in (0, 1, 2):
        cache = r.cache if chunk == 0 else r.net.cache_sources(*r.views, chunk=chunk)
        got = cache.named_buffers()
        assert sorted(got) == sorted(want), (chunk, sorted(got), sorted(want))
        for k in want:
            _same(got[k], want[k], (name, "chunk", chunk, k))
        assert not cache.struct.fg_feat[2] and not cache.struct.bg_feat[2], "no buffer for level_2 features"
        assert cache.nbytes() == 4 * floats
    # (the colours: expected_buffers packs the foreground's texels with inps and the background's with bg_inps, and shows that
    # the other image would give other texels)
    assert lib.composite_cache_sizes(cascade_struct(DC.config(name)), V, H, W) == [0 if b is None else b.numel() for b in r.cache.buffers]
    with pytest.raises(EnerfError, match="chunk=5"):
        r.net.cache_sources(*r.views, chunk=5)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the indexed preparation alone (composite_driver_cases.prep_case's geometries)
def indexed_prep_case(lib, dev, big=False):
    cas = EnerfConfig().cas
    b = {k: torch.from_numpy(v).to(dev) for k, v in make_batch(64, 96, V, EnerfConfig(), seed=31).items()}
    exts, ixts = b["src_exts"][0].contiguous(), b["src_ixts"][0].clone()
    for v in range(V):
        ixts[v, :2, :2] *= 1.0 + 0.01 * v
    n, f = float(b["near_far"][0, 0]), float(b["near_far"][0, 1])
    near_far = torch.tensor([(n + lo * (f - n), n + hi * (f - n)) for lo, hi in ((0.5, 0.9), (0.1, 0.4), (0.0, 1.0))], dtype=torch.float32, device=dev)
    h, w = (32, 48) if big else (8, 12)
    scales = [(cas.im_feat_scale[i], cas.volume_scale[i]) for i in range(2)]
    rasters = [(16, 24), (64, 96)]
    windows = [[(16, 8, 8, 8), (0, 0, 5, 7)], [(32, 0, 64, 64), (3, 5, 33, 17)]]
    if big:
        rasters = [(128, 192), (256, 384)]
        windows = [[(64, 0, 128, 128), (0, 0, 5, 7)], [(1, 10, 241, 34), (100, 56, 284, 200)]]
    for row in PREP_ROWS:
        r = torch.tensor(row, dtype=torch.long, device=dev)
        hand_e, hand_k = exts[r][None].contiguous(), ixts[r][None].contiguous()
        want = lib.composite_prep(hand_k, hand_e, b["tar_ixt"], b["tar_ext"], near_far, scales, 32, 16, h, w, True, rasters, windows)
        got = lib.composite_prep(ixts, exts, b["tar_ixt"], b["tar_ext"], near_far, scales, 32, 16, h, w, True, rasters, windows,
                                 view_idx=torch.tensor(row, dtype=torch.int32, device=dev))
        for i in range(2):
            _same(got[0][i], want[0][i], ("proj", row, i))
            for l in range(2):
                _same(got[3][i][l][0], want[3][i][l][0], ("index", row, i, l))
                _same(got[3][i][l][1], want[3][i][l][1], ("count", row, i, l))
        for c in range(3):
            _same(got[1][c], want[1][c], ("dv", row, c))
            _same(got[2][c], want[2][c], ("nf", row, c))
        _same(got[4][0], hand_e, ("cam_exts", row))
        _same(got[4][1], hand_k, ("cam_ixts", row))
        assert bool(torch.isfinite(got[0][0]).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the frame
def frame_case(lib, dev, name, frames=1):
    """forward_cached against forward on hand-gathered views, with the lane and on one stream; (``frames`` > 1: the GPU, where the
    chains really overlap) that many frames in a row with the lane on, alternating two index rows; then other boxes and back."""
    r = rig(lib, dev, name)
    rows = INDEX_ROWS[r.case["S"]]
    refs = {}
    for row in rows:
        refs[tuple(row)] = r.reference(row)
        DC.assert_frames_equal(r.cached(row), refs[tuple(row)], (name, "lane", row))
        one = Options(single_stream=1)
        DC.assert_frames_equal(r.cached(row, one), r.reference(row, one), (name, "single_stream", row))
    cas = DC.config(name).cas
    assert set(refs[tuple(rows[0])][0]) == {f"{k}_level{i}" for i in range(cas.num) if cas.render_if[i]
                                            for k in ("rgb", "depth", "weights", "net_output", "z_vals")}
    assert not torch.equal(refs[tuple(rows[0])][0][f"rgb_level{cas.num - 1}"], refs[tuple(rows[1])][0][f"rgb_level{cas.num - 1}"])
    for n in range(frames if frames > 1 else 0):
        row = rows[n % 2]
        DC.assert_frames_equal(r.cached(row), refs[tuple(row)], (name, "lane, frame", n, row))
    other = DC.OTHER_BOXES[name]
    DC.assert_frames_equal(r.cached(rows[0], boxes=other), r.reference(rows[0], boxes=other), (name, "other boxes"))
    DC.assert_frames_equal(r.cached(rows[0]), refs[tuple(rows[0])], (name, "first boxes again"))


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. rebuild
def rebuild_case(lib, dev, name="b"):
    r = rig(lib, dev, name)
    row = INDEX_ROWS[r.case["S"]][0]
    views2 = tuple(torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in views_np(name, seed_offset=50)[0])
    assert not torch.equal(views2[0], r.views[0])
    fresh = r.net.cache_sources(*views2)
    cache = r.net.cache_sources(*r.views)
    ptrs = [None if b is None else b.data_ptr() for b in cache.buffers]
    assert cache.rebuild(views2[0], views2[1], views2[2], views2[3]) is cache
    assert ptrs == [None if b is None else b.data_ptr() for b in cache.buffers], "in place"
    for k, b in fresh.named_buffers().items():
        _same(cache.named_buffers()[k], b, ("rebuild", k))
    DC.assert_frames_equal(r.cached(row, cache=cache), r.cached(row, cache=fresh), "rebuilt cache, frame")
    DC.assert_frames_equal(r.cached(row, cache=cache), r.reference(row, views=views2), "rebuilt cache against forward")
    # bg_inps=None: the first rig's images again, the second rig's background colours stay
    cache.rebuild(r.views[0])
    mixed = (r.views[0], views2[1], views2[2], views2[3])
    want = r.net.cache_sources(*mixed)
    for k, b in want.named_buffers().items():
        _same(cache.named_buffers()[k], b, ("rebuild, bg kept", k))
    DC.assert_frames_equal(r.cached(row, cache=cache), r.reference(row, views=mixed), "bg kept, frame")
    # an empty cache is refused until it is rebuilt (and cannot be rebuilt without a background)
    empty = CompositeSourceCache.empty(r.net, V, H, W, r.views[2], r.views[3])
    with pytest.raises(RuntimeError, match="rebuild"):
        r.net.forward_cached(empty, r.index(row), r.target())
    with pytest.raises(ValueError, match="bg_inps"):
        empty.rebuild(r.views[0])
    empty.rebuild(r.views[0], r.views[1])
    DC.assert_frames_equal(r.cached(row, cache=empty), r.cached(row), "an empty cache, rebuilt")
    # stale after load_state_dict, until rebuild
    r.net.load_state_dict(r.net.state_dict())
    try:
        with pytest.raises(RuntimeError, match="rebuild"):
            r.net.forward_cached(cache, r.index(row), r.target())
        cache.rebuild(mixed[0])
        DC.assert_frames_equal(r.cached(row, cache=cache), r.reference(row, views=mixed), "rebuilt after load_state_dict")
    finally:
        r.net.prepare()
        r.cache.rebuild(r.views[0])             # the rig's own cache: current again for the cases after this one
    # modes that have no cached frame
    r.net.train()
    try:
        with pytest.raises(RuntimeError, match="eval"):
            r.net.cache_sources(*r.views)
        with pytest.raises(RuntimeError, match="inference only"):
            r.net.forward_cached(r.cache, r.index(row), r.target())
    finally:
        r.net.eval()
    r.net.stage_hook = lambda stage: None
    try:
        with pytest.raises(RuntimeError, match="stage_hook"):
            r.net.forward_cached(r.cache, r.index(row), r.target())
    finally:
        r.net.stage_hook = None
    with pytest.raises(ValueError, match="integer view indices"):
        r.net.forward_cached(r.cache, r.index(row).float(), r.target())


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. trace (emulator)
def _traced_cached(r, row, options):
    from emu_lib import emu_trace
    r.net.options = options
    with torch.no_grad(), emu_trace(r.lib) as tr:
        r.net.forward_cached(r.cache, r.index(row), r.target())
    return tr


def trace_case(lib, dev, name):
    from collections import Counter
    r = rig(lib, dev, name)
    row = INDEX_ROWS[r.case["S"]][0]
    from emu_lib import emu_trace
    cas = DC.config(name).cas
    batch = r.by_hand(row)
    r.cached(row), r.reference(row)                                     # both shapes sized
    # the kernels of one net's sources in the uncached frame: the FeatureNet and a texel pack per rendered level
    src = batch["src_inps"][0]
    bufs = lib.feature_net_alloc(src)
    with emu_trace(lib) as ft:
        lib.feature_net_stage(r.net._packed_weights("feature_net"), src, bufs, lib.FEAT_ALL)
        for i in range(cas.num):
            if cas.render_if[i]:
                f = bufs[cas.render_im_feat_level[i]]
                lib.pack_texels_cl(f, src, f.shape[1], f.shape[2])
    sources = DC.kernel_names(ft)
    packs = [k for k in sources if "pack_texels" in k]
    assert sources["k_conv0_fused_cb"] == 1 and packs
    for options in (None, Options(single_stream=1)):
        plain = DC.kernel_names(DC.traced(lib, r.net, batch, options))
        tr = _traced_cached(r, row, options)
        names = DC.kernel_names(tr)
        assert names["k_conv0_fused_cb"] == 0 and plain["k_conv0_fused_cb"] == 2, "no FeatureNet in a cached frame"
        assert not [k for k in names if "pack_texels" in k] and all(plain[k] == 2 * sources[k] for k in packs), "no texel pack"
        assert names["k_gather_sources"] == 2 and names["k_composite_prep"] == 1 and plain["k_gather_sources"] == 0
        # every other kernel runs as often as in the uncached frame
        assert names == plain - sources - sources + Counter({"k_gather_sources": 2}), (names, plain, sources)
        prep = DC.launches(tr, "k_composite_prep")
        gathers = DC.launches(tr, "k_gather_sources")
        assert prep == [min(i for i, t in enumerate(tr) if t[0] == "launch")] and tr[prep[0]][3] == "main" and tr[prep[0]][2][0] <= 600
        if options is None:
            DC.check_fork_join(tr)
            records = [i for i, t in enumerate(tr) if t[0] == "record"]
            assert records and prep[0] < records[0], "the prep launch precedes every record"
            assert sorted(tr[g][3] for g in gathers) == ["main", "side"]
            assert tr[gathers[0]][3] == "side", "the foreground's gather is enqueued first"
            assert tr[gathers[0]][2][1] == r.case["S"]
        else:
            assert not [t for t in tr if t[0] != "launch"] and {t[3] for t in tr} == {"main"}


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. refusals (emulator)
def _cached_args(r):
    row = INDEX_ROWS[r.case["S"]][0]
    r.cached(row)
    key = next(k for k in r.net._shapes if k[0] == "cached" and k[4] == tuple(tuple(float(x) for x in b) for b in r.case["boxes"]))
    st = r.net._shapes[key]
    return CompositeFrameArgs.from_buffer_copy(st["call.args"]), CompositeCacheStruct.from_buffer_copy(r.cache.struct), st


def _unalign(k, field, i):
    getattr(k, field)[i] = getattr(k, field)[i] + 4


CACHE_REFUSALS = {      # name -> (mutation of (args, cache struct), what the message must name)
    "V=0": (lambda a, k: setattr(k, "V", 0), "V=0"),
    "V=-2": (lambda a, k: setattr(k, "V", -2), "V=-2"),
    "H": (lambda a, k: setattr(k, "H", H + 4), r"built for 68x96 images \(H, W\)"),
    "W": (lambda a, k: setattr(k, "W", W - 4), r"built for 64x92 images \(H, W\)"),
    "fg feature map": (lambda a, k: k.fg_feat.__setitem__(0, None), r"fg_feat\[0\]"),
    "bg feature map": (lambda a, k: k.bg_feat.__setitem__(a.cas.num - 1, None), r"bg_feat\[\d\]"),
    "fg texels": (lambda a, k: k.fg_tex.__setitem__(a.cas.num - 1, None), r"fg_tex\[\d\].*rendered level"),
    "bg texels": (lambda a, k: k.bg_tex.__setitem__(a.cas.num - 1, None), r"bg_tex\[\d\].*rendered level"),
    "exts": (lambda a, k: setattr(k, "exts", None), "exts"),
    "unaligned map": (lambda a, k: _unalign(k, "bg_feat", 0), "16-byte aligned"),
    "unaligned texels": (lambda a, k: _unalign(k, "fg_tex", a.cas.num - 1), "16-byte aligned"),
    "unaligned cameras": (lambda a, k: setattr(k, "ixts", k.ixts + 4), "16-byte aligned"),
}


def cache_refusal_case(lib, dev, which):
    from emu_lib import emu_trace
    r = rig(lib, dev, "b")
    a, k, keep = _cached_args(r)
    mutate, names = CACHE_REFUSALS[which]
    mutate(a, k)
    idx = r.index(INDEX_ROWS[2][0])
    with emu_trace(lib) as tr:
        rc = lib.dll.enerf_forward_composite_cached(C.byref(a), C.byref(k), idx.data_ptr(), None)
    msg = lib.dll.enerf_last_error().decode()
    assert rc == EINVAL, (which, rc, msg)
    assert re.search(names, msg) and msg.startswith("forward_composite_cached:"), (which, msg)
    assert tr == [], (which, tr)
    assert lib.dll.enerf_forward_composite_cached_workspace_bytes(C.byref(a), C.byref(k)) == 0
    del keep


def null_refusals_case(lib, dev):
    from emu_lib import emu_trace
    r = rig(lib, dev, "b")
    a, k, keep = _cached_args(r)
    idx = r.index(INDEX_ROWS[2][0])
    with emu_trace(lib) as tr:
        assert lib.dll.enerf_forward_composite_cached(C.byref(a), None, idx.data_ptr(), None) == EINVAL
        assert "null cache" in lib.dll.enerf_last_error().decode()
        assert lib.dll.enerf_forward_composite_cached(C.byref(a), C.byref(k), None, None) == EINVAL
        assert "null view_idx" in lib.dll.enerf_last_error().decode()
        assert lib.dll.enerf_forward_composite_cached(None, C.byref(k), idx.data_ptr(), None) == EINVAL
        assert "null args" in lib.dll.enerf_last_error().decode()
    assert tr == []
    assert lib.dll.enerf_forward_composite_cached_workspace_bytes(C.byref(a), None) == 0
    assert lib.dll.enerf_forward_composite_cached_workspace_bytes(None, C.byref(k)) == 0
    # what the cached frame ignores may be anything
    for f in ("src_inps", "bg_src_inps", "src_exts", "src_ixts", "feature_net_packed", "feature_net_bg_packed"):
        setattr(a, f, None)
    assert lib.dll.enerf_forward_composite_cached_workspace_bytes(C.byref(a), C.byref(k)) == keep["call.ws"].numel() * 4
    lib._check(lib.dll.enerf_forward_composite_cached(C.byref(a), C.byref(k), idx.data_ptr(), None), "forward_composite_cached")
    # the indexed preparation's own refusals: a valid preparation whose index is missing, or whose tables are empty
    from enerf_amd.lib import CompositePrepArgs
    t = torch.zeros(4096, dtype=torch.float32, device=r.dev)
    p = CompositePrepArgs(L=1, S=2, num_levels=1, fg_planes=4, bg_planes=4, h=4, w=4, depth_inv=1)
    p.src_ixts = p.src_exts = p.tar_ixt = p.tar_ext = p.near_far = t.data_ptr()
    p.proj[0] = t.data_ptr()
    for c in range(2):
        p.dv[c] = p.nf[c] = t.data_ptr()
    with emu_trace(lib) as tr:
        assert lib.dll.enerf_composite_prep_indexed(C.byref(p), None, V, t.data_ptr(), t.data_ptr(), None) == EINVAL
        assert "view_idx / cam_exts / cam_ixts" in lib.dll.enerf_last_error().decode()
        assert lib.dll.enerf_composite_prep_indexed(C.byref(p), idx.data_ptr(), 0, t.data_ptr(), t.data_ptr(), None) == EINVAL
        assert "V=0" in lib.dll.enerf_last_error().decode()
        assert lib.dll.enerf_composite_prep_indexed(None, idx.data_ptr(), V, t.data_ptr(), t.data_ptr(), None) == EINVAL
    assert tr == []
    del keep


def frame_refusal_case(lib, dev, which):
    """Two of composite_driver_cases.REFUSALS sent through the cached entry: the frame's own refusals are the uncached frame's."""
    from emu_lib import emu_trace
    r = rig(lib, dev, "b")
    a, k, keep = _cached_args(r)
    mutate, code, names = DC.REFUSALS[which]
    mutate(a)
    idx = r.index(INDEX_ROWS[2][0])
    with emu_trace(lib) as tr:
        rc = lib.dll.enerf_forward_composite_cached(C.byref(a), C.byref(k), idx.data_ptr(), None)
    msg = lib.dll.enerf_last_error().decode()
    assert rc == code, (which, rc, msg)
    assert re.search(names, msg) and msg.startswith("forward_composite:"), (which, msg)
    assert tr == [], (which, tr)
    if code == EINVAL:
        assert lib.dll.enerf_forward_composite_cached_workspace_bytes(C.byref(a), C.byref(k)) == 0
    del keep


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. an index outside [0, V) (emulator only: never run this on a GPU)
def out_of_range_case(lib, dev, name="a"):
    """``[0, 7, 1]`` with V = 5: nothing faults, every output of every rendered level is NaN throughout — the views' own NaN reaches
    the colours only (the ReLUs upstream return 0 for NaN), the rest is the merge's, told by the preparation's flag —, and a good
    frame afterwards is the reference's: the flag is rewritten by every frame."""
    assert dev.type == "cpu", "an out-of-range index is an emulator test"
    r = rig(lib, dev, name)
    rows = {3: ([0, 7, 1], [0, 2, 1]), 2: ([7, 1], [2, 1])}[r.case["S"]]
    good = r.cached(rows[1])
    for options in (None, Options(single_stream=1)):
        out, inter = r.cached(rows[0], options)
        cas = DC.config(name).cas
        assert set(out) == {f"{k}_level{i}" for i in range(cas.num) if cas.render_if[i] for k in ("rgb", "depth", "weights", "net_output", "z_vals")}
        for k, v in sorted(out.items()):
            assert bool(v.isnan().all()), (k, int(v.isnan().sum()), v.numel())
        DC.assert_frames_equal(r.cached(rows[1]), good, "a good frame after the bad index")
    for bad in ([0, -1, 1], [5, 0, 1])[:1 if r.case["S"] == 2 else 2]:
        bad = bad[-r.case["S"]:]
        out, _ = r.cached(bad)
        assert all(bool(v.isnan().all()) for v in out.values()), bad
    DC.assert_frames_equal(r.cached(rows[1]), good, "a good frame after the bad indices")
    DC.assert_frames_equal(good, r.reference(rows[1]), "and it is the reference's")


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. GPU only
def _cameras(r):
    """Three target cameras (world-to-camera, camera-to-world) around the rig and the views' camera centres."""
    exts = r.views[2]
    cam_points = torch.linalg.inv(exts.double().cpu())[:, :3, 3].float().to(r.dev).contiguous()
    cams = []
    for c in ([0.0, 0.0, 0.0], [-120.0, -30.0, 10.0], [150.0, 90.0, -20.0]):
        ext = look_at_w2c(np.array(c))
        cams.append((torch.from_numpy(ext.astype(np.float32))[None].to(r.dev),
                     torch.from_numpy(np.linalg.inv(ext).astype(np.float32)).to(r.dev).contiguous()))
    return cam_points, cams


def graph_case(lib, dev, name):
    """select_views -> forward_cached captured once; replayed with three target cameras == eager, and eager == forward by hand."""
    from enerf_amd.graph import GraphedFrame
    r = rig(lib, dev, name)
    S = r.case["S"]
    cam_points, cams = _cameras(r)
    r.net.options = None

    def loop(b):
        idx = lib.select_views(cam_points, b["c2w"], S)
        out = dict(r.net.forward_cached(r.cache, idx, b))
        out["near_views"] = idx
        return out

    tar = {k: v for k, v in r.target().items() if not k.startswith("rays_")}          # full-image rays are generated on the device
    batches = [dict(tar, tar_ext=ext, c2w=c2w) for ext, c2w in cams]
    with torch.no_grad():
        eager = [{k: v.clone() for k, v in loop(b).items()} for b in batches]
    torch.cuda.synchronize()
    assert len({tuple(e["near_views"].tolist()) for e in eager}) >= 2, "the cameras select different view sets"
    for e, b in zip(eager, batches):
        hand = r.by_hand(e["near_views"].tolist())
        hand = {k: v for k, v in hand.items() if not k.startswith("rays_")}
        hand["tar_ext"] = b["tar_ext"]
        ref = DC.Pair.run(r.net, hand)[0]
        for k in ref:
            _same(e[k], ref[k], (name, "eager", k))
    frame = GraphedFrame(r.net, batches[0], fn=loop)
    for n, (b, e) in enumerate(list(zip(batches, eager)) + [(batches[0], eager[0])]):
        out = frame(b)
        torch.cuda.synchronize()
        for k in e:
            _same(out[k], e[k], (name, "replay", n, k))


def no_sync_case(lib, dev, name="b"):
    """Under ``torch.cuda.set_sync_debug_mode("error")`` an implicit synchronisation raises: the build, the selection and the cached
    frame (boxes on the host) have none."""
    r = rig(lib, dev, name)
    cam_points, cams = _cameras(r)
    b = dict(r.target(), tar_ext=cams[1][0], c2w=cams[1][1])
    r.net.options = None
    with torch.no_grad():
        warm = r.net.forward_cached(r.cache, lib.select_views(cam_points, b["c2w"], r.case["S"]), b)        # sizes the workspace
        ref = {k: v.clone() for k, v in warm.items()}
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            fresh = r.net.cache_sources(*r.views)
            idx = lib.select_views(cam_points, b["c2w"], r.case["S"])
            out = r.net.forward_cached(fresh, idx, b)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    for k in ref:
        _same(out[k], ref[k], ("no sync", k))


def uint8_case(lib, dev, name="b"):
    """(V,H,W,3) uint8 images: the build equals the float build of ingest_views_u8's output, buffer for buffer."""
    r = rig(lib, dev, name)
    g = torch.Generator().manual_seed(11)
    u8 = torch.randint(0, 256, (V, H, W, 3), dtype=torch.uint8, generator=g).to(dev)
    bg8 = torch.randint(0, 256, (V, H, W, 3), dtype=torch.uint8, generator=g).to(dev)
    got = r.net.cache_sources(u8, bg8, r.views[2], r.views[3])
    want = r.net.cache_sources(lib.ingest_views_u8(u8), lib.ingest_views_u8(bg8), r.views[2], r.views[3])
    for k, b in want.named_buffers().items():
        _same(got.named_buffers()[k], b, ("uint8", k))
    mixed = r.net.cache_sources(u8, r.views[1], r.views[2], r.views[3])                 # a uint8 rig over a float background
    _same(mixed.named_buffers()["fg_feat0"], want.named_buffers()["fg_feat0"], "uint8 + float")
    with pytest.raises(ValueError, match="uint8"):
        r.net.cache_sources(u8.float(), bg8, r.views[2], r.views[3])
