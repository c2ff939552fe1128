"""The shipped binding modules (integration/lib/networks/enerf/network[_human]_amd.py) loaded through the reference's OWN
loader: ``lib.networks.make_network.make_network(cfg)`` (make_network.py:5-9) with the reference's yacs ``cfg``
(``EnerfConfig.from_yacs``), a reference-saved ``state_dict`` loaded with ``strict=True`` (net_utils.py:443), one forward
on the CPU lane emulator compared with the reference network's own forward on the same batch.

Where the reference tree is absent, its side comes from vectors it recorded (oracle/make_golden_integration.py).  One
subprocess per case and side because the reference's cfg is an import-time global."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAVE_REF = os.path.isdir("/root/reference/lib/networks/enerf")

_PRELUDE = r'''
import os, sys
ROOT, case = sys.argv[1], sys.argv[2]
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
human = case == "human"
module = "lib.networks.enerf.network_human_amd" if human else "lib.networks.enerf.network_amd"
'''

_REFERENCE = r'''
from oracle.ref_loader import load_reference
cfg_file = "configs/enerf/zjumocap_eval.yaml" if human else "configs/enerf/dtu_pretrain.yaml"
opts = ["network_module", module] + ([] if human else ["enerf.cas_config.volume_planes", "8,8"])
cfg, ref_network = load_reference(cfg_file, opts)
assert cfg.network_path == module.replace(".", "/") + ".py"          # config.py:166-168 derived it
cfg.network_path = os.path.join(ROOT, "integration", cfg.network_path)  # the file a maintainer copies into lib/networks/enerf/
os.chdir("/root/reference")
from lib.networks.make_network import make_network
net = make_network(cfg)                                                # imp.load_source(...).Network()
if human:
    from lib.networks.enerf import network_human as ref_network
torch.manual_seed(0)
ref = ref_network.Network().eval()
sd = ref.state_dict()                                                   # what net_utils.save_model stores under 'net'
g = torch.Generator().manual_seed(3)
for k, v in sd.items():
    if k.endswith("running_mean"): v.copy_(torch.randn(v.shape, generator=g) * 0.1)
    elif k.endswith("running_var"): v.copy_(torch.rand(v.shape, generator=g) + 0.5)
from enerf_amd.synth import make_batch, make_zju_batch
b = make_zju_batch(32, 32, 2, net.cfg, seed=1) if human else make_batch(32, 64, 3, net.cfg, seed=1, textured=True)
batch = {k: torch.from_numpy(v) for k, v in b.items()}
torch.set_num_threads(1)
with torch.no_grad():
    want = ref(batch)
'''

# the reference's side recorded by oracle/make_golden_integration.py: its yacs values stand in for ``lib.config.cfg``, the
# binding module is loaded from its file the way make_network.py:5-9 does (imp.load_source(module, path).Network()), and the
# reference's forward was taken with seeded_state_dict weights on the same seeded batch
_GOLDEN = r'''
import importlib.util, json, types
g = np.load(os.path.join(ROOT, "tests", "golden", f"integration_{case}.npz"))
ns = lambda d: types.SimpleNamespace(**{k: ns(v) if isinstance(v, dict) else v for k, v in d.items()})
cfg = ns(json.loads(str(g["cfg_json"])))
lib, lib_config = types.ModuleType("lib"), types.ModuleType("lib.config")
lib.__path__, lib_config.cfg, lib.config = [], cfg, lib_config
sys.modules.update({"lib": lib, "lib.config": lib_config})
assert cfg.network_module == module and cfg.network_path == module.replace(".", "/") + ".py"
spec = importlib.util.spec_from_file_location(module, os.path.join(ROOT, "integration", cfg.network_path))
mod = importlib.util.module_from_spec(spec)
spec.loader.exec_module(mod)
net = mod.Network()
from oracle.make_golden_integration import seeded_state_dict
sd = seeded_state_dict(json.loads(str(g["state_dict_spec"])))         # the reference's key set, with the recorded run's weights
from enerf_amd.synth import make_batch, make_zju_batch
b = make_zju_batch(32, 32, 2, net.cfg, seed=1) if human else make_batch(32, 64, 3, net.cfg, seed=1, textured=True)
batch = {k: torch.from_numpy(v) for k, v in b.items()}
want = {k[4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("out/")}
torch.set_num_threads(1)
'''

_CHECK = r'''
from enerf_amd.network import Network as Amd, NetworkHuman as AmdH
assert isinstance(net, AmdH if human else Amd) and net.human == human
assert tuple(net.cfg.cas.volume_planes) == tuple(cfg.enerf.cas_config.volume_planes)
missing = net.load_state_dict(sd, strict=True)                         # net_utils.py:443
net.eval()
from emu_lib import emu_lib
net._lib = emu_lib()
got = net(batch)
assert sorted(got) == sorted(want), (sorted(got), sorted(want))
worst = 0.0
for k in want:
    assert got[k].shape == want[k].shape, k
    err = float((got[k] - want[k]).abs().max() / (want[k].abs().max() + 1e-12))
    worst = max(worst, err)
    assert err < 1e-4, (k, err)
print("INTEGRATION_OK", case, len(sd), worst)
'''


@pytest.mark.parametrize("case", ["dtu", "human"])
def test_binding_module_through_reference_make_network(case, tmp_path):
    """Against the recorded reference (tests/golden/integration_<case>.npz) everywhere, and against the live reference tree
    through its own make_network where that tree exists."""
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    for side, code in [("golden", _GOLDEN)] + ([("reference", _REFERENCE)] if HAVE_REF else []):
        script = tmp_path / f"run_integration_{side}.py"
        script.write_text(_PRELUDE + code + _CHECK)
        r = subprocess.run([sys.executable, str(script), ROOT, case], capture_output=True, text=True, env=env, timeout=900)
        assert r.returncode == 0 and "INTEGRATION_OK" in r.stdout, side + ": " + r.stdout[-2000:] + r.stderr[-4000:]
