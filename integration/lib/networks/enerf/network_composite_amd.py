"""``lib/networks/enerf/network_composite_amd.py``: the ENeRF-Outdoor variant (replaces
``lib/networks/enerf/network_composite.py``; ``network_module lib.networks.enerf.network_composite_amd``).  Inference only, B == 1;
the output dict has the reference's keys except ``idx_level{i}`` (enerf_amd/network_composite.py)."""
from lib.config import cfg
from enerf_amd.config import EnerfConfig
from enerf_amd.network_composite import Network as _AmdNetwork


class Network(_AmdNetwork):
    def __init__(self):
        super().__init__(EnerfConfig.from_yacs(cfg), int(cfg.num_fg_layers))
