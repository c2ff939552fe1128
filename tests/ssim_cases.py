"""Inputs of the SSIM fixture (tests/golden/ssim_cases.npz), shared by the generator (tools/make_golden_ssim.py, which runs
under an interpreter that has scikit-image but no torch) and by tests/test_eval_ssim.py.

numpy only, integer arithmetic only: a counter-based 32-bit integer hash and integer ramps, turned into float32 by ONE division
of exactly representable integers — no transcendental function and no ``numpy.random`` stream, so every numpy produces the
same bytes.  The fixture stores the SHA-1 of every array; the tests assert them before comparing anything.

A case is a dict: ``pred`` / ``gt`` (B,h,w,3) float32, ``mask`` (B,h,w) uint8 / int32 or None, ``evaluator`` 'enerf' (mask on =
``>= 1``, optional ``center`` crop: lib/evaluators/enerf.py) or 'human' (mask on = ``== 1``, SSIM on the mask's bounding
rectangle: lib/evaluators/enerf_human.py)."""
from __future__ import annotations

import hashlib

import numpy as np

_U = np.uint64
_M32 = _U(0xFFFFFFFF)


def hash32(n: int, seed: int) -> np.ndarray:
    """n 32-bit values (as uint64) of a fixed integer mixing function of (index, seed)."""
    x = (np.arange(n, dtype=np.uint64) * _U(2654435761) + _U(seed) * _U(40503) + _U(12345)) & _M32
    for _ in range(2):
        x ^= x >> _U(16)
        x = (x * _U(0x45D9F3B)) & _M32
    x ^= x >> _U(16)
    return x


def noise(shape, seed: int) -> np.ndarray:
    """float32 in [0,1): 24 hash bits / 2^24."""
    v = (hash32(int(np.prod(shape)), seed) >> _U(8)).astype(np.float32)
    return (v / np.float32(16777216.0)).reshape(shape)


def ramp_u8(h: int, w: int, seed: int) -> np.ndarray:
    """(h,w,3) int64 in [0,255]: a smooth integer gradient, different per channel."""
    y, x, c = np.meshgrid(np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), np.arange(3, dtype=np.int64), indexing="ij")
    return (20 + (x * (3 + seed) + y * 2) // 4 + 30 * c) % 256


def _u8_to_f32(a: np.ndarray) -> np.ndarray:
    return a.astype(np.float32) / np.float32(255.0)


def smooth_pair(h: int, w: int, seed: int):
    """gt = ramp / 255, pred = (ramp + d) / 255 with d in {-1, 0, 1}: windows whose variance is a few 1e-6."""
    base = ramp_u8(h, w, seed)
    d = (hash32(h * w * 3, seed + 100) % _U(3)).astype(np.int64).reshape(h, w, 3) - 1
    return _u8_to_f32(np.clip(base + d, 0, 255)), _u8_to_f32(base)


def textured_pair(h: int, w: int, seed: int):
    """a ramp under 6 bits of noise (gt) and the same under different noise (pred)."""
    base = ramp_u8(h, w, seed)
    n0 = (hash32(h * w * 3, seed + 200) % _U(64)).astype(np.int64).reshape(h, w, 3)
    n1 = (hash32(h * w * 3, seed + 300) % _U(64)).astype(np.int64).reshape(h, w, 3)
    return _u8_to_f32((base + n1) % 256), _u8_to_f32((base + n0) % 256)


def mask012(h: int, w: int, seed: int) -> np.ndarray:
    """uint8 values 0 / 1 / 2, about 30 % zeros."""
    v = hash32(h * w, seed + 400)
    on = (v % _U(10)) >= _U(3)
    return (on.astype(np.uint8) * (1 + ((v >> _U(8)) % _U(2)).astype(np.uint8))).reshape(h, w)


def blob_mask(h: int, w: int, cx: int, cy: int, ax: int, ay: int, r2: int) -> np.ndarray:
    """int32 ellipse ax*(x-cx)^2 + ay*(y-cy)^2 <= r2, clipped by the image."""
    y, x = np.meshgrid(np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), indexing="ij")
    return (ax * (x - cx) ** 2 + ay * (y - cy) ** 2 <= r2).astype(np.int32)


CASE_NAMES = ("plain", "smooth", "identical", "min7_7x7", "min7_7x40", "mask012", "center", "human_box", "full_dtu", "full_zju")


def build(name: str) -> dict:
    c = dict(name=name, evaluator="enerf", center=False, mask=None)
    if name in ("plain", "identical"):
        gt = noise((1, 61, 83, 3), 1)
        pred = gt.copy() if name == "identical" else noise((1, 61, 83, 3), 2)
    elif name == "smooth":
        pred, gt = (a[None] for a in smooth_pair(96, 160, 3))
    elif name.startswith("min7_"):
        h, w = (7, 7) if name == "min7_7x7" else (7, 40)
        gt, pred = noise((1, h, w, 3), 4 + w), noise((1, h, w, 3), 5 + w)
    elif name in ("mask012", "center"):
        pred, gt = (a[None] for a in textured_pair(96, 160, 6))
        c.update(mask=mask012(96, 160, 6)[None], center=name == "center")
    elif name == "human_box":
        p0, g0 = textured_pair(128, 128, 7)
        p1, g1 = textured_pair(128, 128, 8)
        pred, gt = np.stack([p0, p1]), np.stack([g0, g1])
        m0 = blob_mask(128, 128, 20, 15, 1, 1, 40 * 40)           # touches the top and the left border: box (0,0)-(60,55)
        m0[100:110, 100:120] = 2                                  # not == 1: must not widen the box
        m1 = blob_mask(128, 128, 70, 60, 1, 4, 45 * 45)           # interior ellipse, a different box
        m1[3, 5] = 2
        c.update(mask=np.stack([m0, m1]).astype(np.int32), evaluator="human")
    elif name == "full_dtu":
        pred, gt = (a[None] for a in textured_pair(512, 640, 9))
    elif name == "full_zju":
        pred, gt = (a[None] for a in textured_pair(1024, 1024, 10))
        m = np.zeros((1, 1024, 1024), np.uint8)
        m[0, 150:901, 200:803] = 1
        m[0, 400:420, 300:340] = 0                                # a hole: zeroed inside the box
        c.update(mask=m, evaluator="human")
    else:
        raise KeyError(name)
    c.update(pred=np.ascontiguousarray(pred, dtype=np.float32), gt=np.ascontiguousarray(gt, dtype=np.float32))
    return c


def sha1s(case: dict) -> dict:
    """{array name: SHA-1 of dtype, shape and bytes} of the case's arrays."""
    out = {}
    for k in ("pred", "gt", "mask"):
        a = case[k]
        if a is not None:
            a = np.ascontiguousarray(a)
            out[k] = hashlib.sha1(f"{a.dtype.str}{a.shape}".encode() + a.tobytes()).hexdigest()
    return out
