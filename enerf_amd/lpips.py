"""Weights of the device-side LPIPS (``EnerfLib.eval_lpips``, csrc/lpips_vgg.h): the VGG16 trunk's thirteen 3x3 convolutions and the
five ``lin`` vectors of ``lpips.LPIPS(net='vgg')`` (lib/evaluators/enerf.py:81-87, enerf_human.py:71-77).

No weights ship with this package: the network is fixed and public, the numbers are the user's to supply
(``LpipsWeights.from_state_dict``).  ``LpipsWeights.random`` exists for tests and benchmarks only.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch

from .lib import LPIPS_TAP_CHANNELS, VGG_CONVS, EnerfLib, get_lib

# torchvision VGG16 ``features`` index of every conv, and the lpips slice (1..5) that holds it
VGG_FEATURE_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
_SLICE_OF = (1, 1, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5)

# THE key table: canonical name -> (torchvision-style name, lpips-package name).  The lpips names were written from memory of lpips
# 0.1.4 and are NOT verified against the package (it is not a dependency of this project): confirm them against your checkpoint.
KEY_TABLE: Dict[str, Tuple[str, str]] = {}
for _i, (_idx, _s) in enumerate(zip(VGG_FEATURE_INDEX, _SLICE_OF)):
    for _p in ("weight", "bias"):
        KEY_TABLE[f"conv{_i}.{_p}"] = (f"features.{_idx}.{_p}", f"net.slice{_s}.{_idx}.{_p}")
for _l in range(5):
    KEY_TABLE[f"lin{_l}"] = (f"lin{_l}", f"lin{_l}.model.1.weight")


class LpipsWeights:
    """The thirteen (w, b) pairs and five lin vectors on one device, plus the packed image the kernels read (built on first use)."""

    def __init__(self, convs: List[Tuple[torch.Tensor, torch.Tensor]], lins: List[torch.Tensor]):
        if len(convs) != 13 or len(lins) != 5:
            raise ValueError("LpipsWeights needs 13 (w, b) pairs and 5 lin vectors")
        for i, ((w, b), (cin, cout)) in enumerate(zip(convs, VGG_CONVS)):
            if tuple(w.shape) != (cout, cin, 3, 3) or tuple(b.shape) != (cout,):
                raise ValueError(f"conv {i} (features.{VGG_FEATURE_INDEX[i]}): expected ({cout},{cin},3,3) + ({cout},), "
                                 f"got {tuple(w.shape)} + {tuple(b.shape)}")
        for l, (v, c) in enumerate(zip(lins, LPIPS_TAP_CHANNELS)):
            if tuple(v.shape) != (c,):
                raise ValueError(f"lin{l}: expected ({c},), got {tuple(v.shape)}")
        self.convs = [(w.detach().to(torch.float32).contiguous(), b.detach().to(torch.float32).contiguous()) for w, b in convs]
        self.lins = [v.detach().to(torch.float32).contiguous() for v in lins]
        self._packed: Optional[torch.Tensor] = None
        self._packed_by = None

    @property
    def device(self):
        return self.lins[0].device

    def packed(self, lib: Optional[EnerfLib] = None) -> torch.Tensor:
        lib = lib or get_lib()
        if self._packed is None or self._packed_by is not lib:
            self._packed, self._packed_by = lib.lpips_pack(self.convs, self.lins), lib
        return self._packed

    def state_dict(self, names: str = "torchvision") -> Dict[str, torch.Tensor]:
        """The weights under the ``torchvision`` (``features.N.weight``, ``lin{k}`` as (1,C,1,1)) or ``lpips`` key spelling."""
        col = {"torchvision": 0, "lpips": 1}[names]
        sd = {}
        for i, (w, b) in enumerate(self.convs):
            sd[KEY_TABLE[f"conv{i}.weight"][col]] = w
            sd[KEY_TABLE[f"conv{i}.bias"][col]] = b
        for l, v in enumerate(self.lins):
            sd[KEY_TABLE[f"lin{l}"][col]] = v.reshape(1, -1, 1, 1)
        return sd

    @classmethod
    def from_state_dict(cls, sd: Dict[str, torch.Tensor], device) -> "LpipsWeights":
        """Accepts exactly one of two spellings (``KEY_TABLE``): a torchvision VGG16 ``features.{0,2,5,...,28}.{weight,bias}`` dict
        plus ``lin{0..4}``, or the lpips package's ``net.slice{1..5}.{idx}.{weight,bias}`` and ``lin{k}.model.1.weight``.  The lpips
        spelling is UNVERIFIED against the package (written from memory of lpips 0.1.4): check it against your checkpoint, and
        pass only these 31 tensors (drop anything else the checkpoint holds).  A missing key, an extra key or a wrong shape raises;
        lin may be (C,) or (1,C,1,1)."""
        keys = set(sd)
        hits = [len(keys & {v[col] for v in KEY_TABLE.values()}) for col in (0, 1)]
        if max(hits) == 0:
            raise KeyError("LpipsWeights.from_state_dict: the keys are neither the torchvision spelling (features.0.weight ... lin4) nor "
                           f"the lpips spelling (net.slice1.0.weight ... lin4.model.1.weight); got {sorted(keys)[:4]} ...")
        col = 0 if hits[0] >= hits[1] else 1
        want = {v[col] for v in KEY_TABLE.values()}
        missing, extra = sorted(want - keys), sorted(keys - want)
        if missing or extra:
            raise KeyError(f"LpipsWeights.from_state_dict ({('torchvision', 'lpips')[col]} names): missing {missing}, unexpected {extra}")
        convs = [(sd[KEY_TABLE[f"conv{i}.weight"][col]].to(device), sd[KEY_TABLE[f"conv{i}.bias"][col]].to(device)) for i in range(13)]
        lins = []
        for l, c in enumerate(LPIPS_TAP_CHANNELS):
            v = sd[KEY_TABLE[f"lin{l}"][col]]
            if tuple(v.shape) not in ((c,), (1, c, 1, 1)):
                raise ValueError(f"lin{l}: expected ({c},) or (1,{c},1,1), got {tuple(v.shape)}")
            lins.append(v.reshape(c).to(device))
        return cls(convs, lins)

    @classmethod
    def random(cls, seed: int, device="cpu") -> "LpipsWeights":
        """Seeded random weights — TEST AND BENCHMARK MATERIAL, not a perceptual metric: He-normal convolutions (activations keep
        their scale through the thirteen layers), biases 0.05 * N(0,1), lin uniform in [0,1] / C."""
        g = torch.Generator().manual_seed(int(seed))
        convs, lins = [], []
        for cin, cout in VGG_CONVS:
            w = torch.randn((cout, cin, 3, 3), generator=g) * (2.0 / (9 * cin)) ** 0.5
            convs.append((w.to(device), (0.05 * torch.randn((cout,), generator=g)).to(device)))
        for c in LPIPS_TAP_CHANNELS:
            lins.append((torch.rand((c,), generator=g) / c).to(device))
        return cls(convs, lins)
