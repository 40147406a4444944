"""Shared helpers for the tests: small deterministic scenes and cameras."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from unitygaussiansplatting_amd import camera, creator, scenes

PRESETS = ["VeryLow", "Low", "Medium", "High", "VeryHigh"]


def _p(a):
    """the address of an array's data for a ctypes call; None stays NULL"""
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def same_bits(a, b, dtype=np.float32) -> bool:
    """the same shape and the same bits, both read as `dtype`; dtype=None: as they are, and then of the same dtype too"""
    a, b = np.ascontiguousarray(a, dtype), np.ascontiguousarray(b, dtype)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@functools.lru_cache(maxsize=16)
def small_asset(n: int = 20000, seed: int = 5, quality: str = "Medium", extent: float = 3.0, **fmt):
    raw = scenes.make_splats(n, seed, extent)
    return creator.CreateAssetFromSplats(raw, quality, name=f"t{n}_{seed}_{quality}", **fmt)


def default_camera(W=320, H=200, az=25.0, elev=10.0, radius=6.0, fov=39.0965):
    return camera.Camera(position=scenes.orbit_eye(radius, elev, az), pixelWidth=W, pixelHeight=H, fieldOfView=fov)


def psnr8(a: np.ndarray, b: np.ndarray) -> float:
    """GaussianSplatValidator.cs:202-204: PSNR = 20 log10(255) - 10 log10(rmse^2) on 8-bit images."""
    d = a.astype(np.float64) - b.astype(np.float64)
    mse = float((d * d).mean())
    if mse == 0.0:
        return float("inf")
    return 20.0 * np.log10(255.0) - 10.0 * np.log10(mse)


def diff_pixels(a: np.ndarray, b: np.ndarray, thr: int = 3) -> int:
    """GaussianSplatValidator.cs:171-199: pixels whose abs diff x5 >= 15, i.e. any channel differing by >= 3/255."""
    d = np.abs(a.astype(np.int32) - b.astype(np.int32))[..., :3].max(axis=-1)
    return int((d >= thr).sum())


def views_equal(got: np.ndarray, want: np.ndarray) -> bool:
    """40-byte SplatViewData records equal bit for bit, except that any NaN equals any NaN (the sign/payload of a NaN
    produced by 0*inf differs between x86 and gfx950 and carries no meaning: a NaN axis only means 'not drawn')."""
    g, w = got.view(np.uint32).reshape(-1, 10), want.view(np.uint32).reshape(-1, 10)
    gf, wf = g[:, :8].view(np.float32), w[:, :8].view(np.float32)
    both_nan = np.isnan(gf) & np.isnan(wf)
    return bool(((g[:, :8] == w[:, :8]) | both_nan).all() and (g[:, 8:] == w[:, 8:]).all())


RT_TOL = 2.0 ** -9
RT_CAP = 2.0 ** -8               # with an opt-in outlier allowance (rt_err(..., rare=n)): no pixel beyond this, ever
RT_RARE_PER_PIXEL = 2.0e-6       # the measured outlier rate behind rare_allowance(): 2 + 2 per megapixel


def rt_diff(img: np.ndarray, ref: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(img, np.uint16).view(np.float16).astype(np.float32)
    b = np.ascontiguousarray(ref, np.uint16).view(np.float16).astype(np.float32)
    return np.abs(a - b) / np.maximum(1.0, np.abs(b))


def rt_abs(img: np.ndarray, ref: np.ndarray) -> float:
    """Plain max-abs difference of two RGBA16F targets (SURVEY.md section 8c's wording of the bar), reported next to rt_err."""
    a = np.ascontiguousarray(img, np.uint16).view(np.float16).astype(np.float32)
    b = np.ascontiguousarray(ref, np.uint16).view(np.float16).astype(np.float32)
    return float(np.abs(a - b).max()) if a.size else 0.0


def rare_allowance(img: np.ndarray) -> int:
    """The opt-in outlier count for a FULL-SIZE frame: 2 + 2 per megapixel (measured: ONE pixel of the 1920x1080 C3 frame at 1.125 * 2^-9)."""
    h, w = img.shape[:2]
    return 2 + int(RT_RARE_PER_PIXEL * h * w)


def rt_err(img: np.ndarray, ref: np.ndarray, tol: float = RT_TOL, rare: int = 0) -> float:
    """Parity metric of the RGBA16F target.  Per pixel and channel e = |a - b| / max(1, |b|): the accumulator
    is fp16, a value c in [2^k, 2^(k+1)) has an ulp of 2^(k-10) and premultiplied splat colours are not clamped to 1, so the bound
    scales with the value (2^-9 = two fp16 ulps of any c in [0.5, 1), at most two of every larger c); for |c| <= 1 -- every pixel of
    the test scenes but a few SH highlights -- it IS the plain max-abs of SURVEY.md section 8c (rt_abs reports that one too).

    Default (rare = 0): the largest e of the frame, no allowance.  The only operation of the frame that is not bit-identical on both
    sides is exp2 (<= 1 ulp of fp32 in a fragment's alpha; the DISCARD decision is identical: gs_device_math.h DecideAlpha); one such
    ulp moves a blend's fp16 result by one fp16 ulp with probability ~2^-13 and the offset then rides along: > 99.99 % of the pixels are
    bit-equal, some carry one or two such ulps (<= 2^-9), and about one pixel in a couple of million collects THREE in one channel.
    A test of a multi-megapixel frame where that was MEASURED opts in with rare = rare_allowance(img): at most that many pixels may lie
    in (tol, RT_CAP], none beyond -- then the value returned is the largest e among the pixels within tol."""
    e = rt_diff(img, ref).max(axis=-1).reshape(-1)
    if e.size == 0:
        return 0.0
    over = e > tol
    if rare <= 0 or tol >= RT_CAP or int(over.sum()) > rare or float(e.max()) > RT_CAP:
        return float(e.max())
    return float(e[~over].max()) if (~over).any() else 0.0
