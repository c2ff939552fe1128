"""The frame driver (csrc/frame.hip run_frame, csrc/side_lane.h) on the CPU lane emulator.  The emulator's lane hands out fake streams
and writes every event record / wait, and every kernel launch, to a trace (emu_lib.emu_trace), so the fork/join discipline of a
frame — which the GPU parity tests can pass by luck when a join is missing — is checked as properties of that trace; and, since
the emulator executes launches in enqueue order, the frame with the lane must equal the one-stream frame bit for bit.

Frames: the cascades of test_source_cache.py plus one human / masked frame, each plain (HIP FeatureNet), through a source cache
and through the NCHW maps of the torch FeatureNet."""
import pytest
import torch

import __graft_entry__ as G
from emu_lib import emu_lib
from enerf_amd.config import EnerfConfig
from enerf_amd.lib import EnerfError, Options
from enerf_amd.synth import make_batch
from test_source_cache import CFG_BOTH, CFG_DEFAULT, CFG_ONE

H, W, S = 32, 64, 3
CASES = {"default": (CFG_DEFAULT, False), "both": (CFG_BOTH, False), "one": (CFG_ONE, False), "human": (CFG_DEFAULT, True)}
WAYS = ("plain", "cached", "nchw")
LANE_STREAMS = ("side", "render")


class Frame:
    """One network + batch, run ``way``; ``run(options)`` -> (outputs, trace)."""

    def __init__(self, cfg, human, way, h=H, w=W):
        self.cfg, self.way = cfg, way
        self.net = G._seeded_network(cfg, "cpu", human=human, lib=emu_lib(), feature_backend="torch" if way == "nchw" else "hip")
        self.net.static_shapes = True
        self.net.prepare()                     # the weight packs' launches stay out of the traces
        self.batch = {k: torch.from_numpy(v) for k, v in make_batch(h, w, S, cfg, seed=3, textured=True, mask_box=human).items()}
        if way == "cached":
            b = self.batch
            self.cache = self.net.cache_sources(b["src_inps"][0].contiguous(), b["src_exts"][0].contiguous(), b["src_ixts"][0].contiguous())
            self.idx = torch.arange(S, dtype=torch.int32)
            self.tar = {k: v for k, v in b.items() if not k.startswith("src_")}

    def run(self, options=None):
        from emu_lib import emu_trace
        self.net.options = options
        with torch.no_grad(), emu_trace(emu_lib()) as tr:
            out = self.net.forward_cached(self.cache, self.idx, self.tar) if self.way == "cached" else self.net(self.batch)
        return out, tr


def _same(out, ref):
    assert sorted(out) == sorted(ref)
    counts = {k[len("num_rays_level"):]: int(v[0]) for k, v in ref.items() if k.startswith("num_rays_level")}
    for k in ref:
        lvl = k[-1]
        if lvl in counts and k.startswith(("depth_level", "weights_level")):      # masked level, static shapes: rows past the count
            m = counts[lvl]                                                         # are never written
            assert 1 < m < H * W and torch.equal(out[k][:, :m], ref[k][:, :m]), k
        else:
            assert torch.equal(out[k], ref[k]), k


# ---- trace helpers: a trace is a list of ("launch", kernel, grid, stream) | ("record", event, stream) | ("wait", event, stream) ----
def _launches(tr, prefix, stream=None):
    return [i for i, r in enumerate(tr) if r[0] == "launch" and r[1].lstrip("(").startswith(prefix) and stream in (None, r[3])]


def _source_of_wait(tr, w):
    """Index of the record a wait binds to: the last record of its event before it (None: never recorded in this call)."""
    for i in range(w - 1, -1, -1):
        if tr[i][0] == "record" and tr[i][1] == tr[w][1]:
            return i
    return None


def _waits(tr, stream, event=None):
    return [i for i, r in enumerate(tr) if r[0] == "wait" and r[2] == stream and event in (None, r[1])]


def check_fork_join(tr):
    """The rules every frame obeys, whatever its cascade: no wait on an event this call did not record; a lane stream starts behind
    the caller's stream; the caller's stream leaves behind every lane stream."""
    for w in _waits(tr, "main") + _waits(tr, "side") + _waits(tr, "render"):
        assert _source_of_wait(tr, w) is not None, ("wait on an event not recorded in this call", w, tr[w])
    for s in LANE_STREAMS:
        on_s = [i for i, r in enumerate(tr) if r[0] == "launch" and r[3] == s]
        if not on_s:
            continue
        forks = [w for w in _waits(tr, s) if w < on_s[0] and tr[_source_of_wait(tr, w)][2] == "main"]
        assert forks, (s, "launches before it waited on the caller's stream")
        joins = [w for w in _waits(tr, "main") if tr[_source_of_wait(tr, w)][2] == s and _source_of_wait(tr, w) > on_s[-1]]
        assert joins, (s, "the caller's stream returns without waiting for its last launch")
    assert all(r[3] in ("main",) + LANE_STREAMS for r in tr if r[0] == "launch"), "a launch on an unknown stream"


def check_consumers(tr, cfg, way):
    """Each join precedes its first consumer on the caller's stream."""
    num = cfg.cas.num
    vols = _launches(tr, "k_feature_volume")
    assert len(vols) == num and all(tr[v][3] == "main" for v in vols)
    renders = _launches(tr, "k_render_rays")
    assert len(renders) == sum(cfg.cas.render_if) and tr[renders[-1]][3] == "main"
    if way == "plain" and num >= 2:           # level 1's maps come from the side stream (a cached frame gathers them on the caller's)
        l1 = _waits(tr, "main", "l1")
        assert l1 and l1[0] < vols[1], "level 1's volume is launched before the caller's stream waited on l1"
    # level_2 — in these cascades always emitted as the texels of the render that reads it, so its first reader is that render, not
    # a texel pack (a cached frame gathers it on the side stream just the same)
    rendered = [i for i in range(num) if cfg.cas.render_if[i]]
    from_l2 = [k for k, i in enumerate(rendered) if cfg.cas.render_im_feat_level[i] == 2]
    assert from_l2 and not _launches(tr, "k_pack_texels_cl", "main") and not _launches(tr, "k_pack_img_feat_rgb", "main")
    reader = renders[from_l2[0]]
    l2 = _waits(tr, "main", "l2")
    assert l2 and l2[0] < reader, "level_2 is read before the caller's stream waited on l2"


@pytest.fixture(scope="module")
def frames():
    made = {}

    def get(case, way):
        if (case, way) not in made:
            cfg, human = CASES[case]
            fr = Frame(cfg, human, way)
            fr.one_stream, fr.one_trace = fr.run(Options(single_stream=1))      # (also packs the weights, outside the later traces)
            made[case, way] = fr
        return made[case, way]
    return get


@pytest.mark.parametrize("way", WAYS)
@pytest.mark.parametrize("case", list(CASES))
def test_lane_frame_equals_one_stream_frame_and_joins_what_it_forks(frames, case, way):
    fr = frames(case, way)
    cfg = fr.cfg
    assert not [r for r in fr.one_trace if r[0] != "launch"] and {r[3] for r in fr.one_trace} == {"main"}     # single_stream: one stream
    out, tr = fr.run(None)
    _same(out, fr.one_stream)
    check_fork_join(tr)
    if way == "nchw":                          # torch's maps: nothing to fork
        assert not [r for r in tr if r[0] != "launch"]
        return
    assert _launches(tr, "", "side"), "the emulator's lane is on by default"
    check_consumers(tr, cfg, way)
    # the lane changes where launches go and (a forked render: fewer persistent blocks) one grid, never which kernels run — but for
    # a cached frame's gather, which is split in two
    extra = ["k_gather_sources"] if way == "cached" else []
    assert sorted(r[1] for r in tr if r[0] == "launch") == sorted([r[1] for r in fr.one_trace] + extra)
    if case == "both":                         # level 0's render is a leaf: on the render stream, behind `fork`, `done` after it
        r0 = _launches(tr, "k_render_rays")[0]
        assert tr[r0][3] == "render"
        behind = [w for w in _waits(tr, "render", "fork") if w < r0 and tr[_source_of_wait(tr, w)][2] == "main"]
        assert behind
        assert [i for i, r in enumerate(tr) if r == ("record", "done", "render") and i > r0]
        assert all(tr[i][3] == "render" for i in range(behind[-1], r0) if tr[i][0] == "launch")      # its texel pack / rays too
    else:
        assert not _launches(tr, "", "render")


@pytest.mark.parametrize("way", WAYS)
@pytest.mark.parametrize("gate", [2, 3, 4])
def test_side_gate_moves_the_last_feature_net_stage_and_nothing_else(frames, gate, way):
    """enerf_options_t.side_gate: the FeatureNet's last stage (k_smooth0_cb) is enqueued on the side stream from inside level 1's
    cost regularisation — after its conv0 (2), before it (3), after its conv2 (4); every CostRegNet layer is one launch."""
    fr = frames("default", way)
    out, tr = fr.run(Options(side_gate=gate))
    _same(out, fr.one_stream)
    check_fork_join(tr)
    if way == "nchw":
        return
    check_consumers(tr, fr.cfg, way)
    if way == "cached":                        # no FeatureNet in the frame: the option has nothing to move
        assert tr == fr.run(None)[1]
        return
    s0 = _launches(tr, "k_smooth0_cb")
    assert len(s0) == 1 and tr[s0[0]][3] == "side"
    vol1 = _launches(tr, "k_feature_volume")[1]
    assert vol1 < s0[0]
    between = [r for r in tr[vol1 + 1:s0[0]] if r[0] == "launch"]
    assert all(r[3] == "main" and r[1].lstrip("(").startswith("k_conv3d") for r in between)
    assert len(between) == {2: 1, 3: 0, 4: 3}[gate]
    w = [i for i in _waits(tr, "side", "fork") if i < s0[0]]
    assert w and tr[_source_of_wait(tr, w[-1])][2] == "main" and _source_of_wait(tr, w[-1]) > vol1


def test_error_after_the_fork_still_joins_the_lane():
    """48x80 (test_emu_pipeline.test_frame_sizes_the_reference_cannot_run_fail_loudly): level 0's cost_reg refuses its volume
    after the FeatureNet's top-down half has been forked; the error exit joins it."""
    fr = Frame(CFG_BOTH, False, "plain", h=48, w=80)
    from emu_lib import emu_trace
    fr.net.options = None
    with pytest.raises(EnerfError, match="divisible by 4"):
        with torch.no_grad(), emu_trace(emu_lib()) as tr:
            fr.net(fr.batch)
    assert _launches(tr, "k_smooth0_cb", "side") and not _launches(tr, "k_conv3d<")
    check_fork_join(tr)
