"""Independent pure-NumPy oracle.

Kept deliberately separate from the C++ oracle (``csrc/src/cpu_stencil.cpp``)
so the two check each other (SURVEY §4 "keeps the C++ oracle honest").

Semantics (reference ``mpi/mpi_convolution.c:301-322``): per
channel, ``out[y][x] = trunc(sum_{k,l} w[k][l] * in[y+k-1][x+l-1])`` with zero
padding (``border="zero"``, the reference's rule) or with the indices clamped
to the image (``border="replicate"``, ``np.pad(mode="edge")``), float32 multiply-then-add in row-major tap order starting from 0.0f.
NumPy's float32 elementwise ops round each multiply and add separately (no FMA),
which reproduces the reference bit for bit; integer-exact filters use
``(sum tap*p) >> shift`` directly.

Depth 16: a ``uint16`` array stays ``uint16`` and runs the gaussian only, as
``(sum tap*p) >> 4`` clamped at 65535 — which is what the reference's float32
formula gives for 16-bit samples too (every product exact, every partial sum a
multiple of 1/16 below 2^16).  Any other dtype is coerced to ``uint8`` as before.
"""
from __future__ import annotations

import numpy as np

from ..models.filters import get_filter

BORDERS = ("zero", "replicate")


def check_border(border: str) -> str:
    if border not in BORDERS:
        raise ValueError(f"unknown border {border!r} (expected zero|replicate)")
    return border


def _as_hwc(img: np.ndarray) -> np.ndarray:
    if img.ndim == 2:
        return img[:, :, None]
    if img.ndim == 3:
        return img
    raise ValueError("image must be (H, W) or (H, W, C)")


def sample_dtype(img) -> np.dtype:
    """``uint16`` for a ``uint16`` array (depth 16), else ``uint8``."""
    return np.dtype(np.uint16) if getattr(img, "dtype", None) == np.uint16 else np.dtype(np.uint8)


def refuse_depth16(image, what: str) -> None:
    """The named error of everything that is not built for ``uint16`` images."""
    if sample_dtype(image) == np.uint16 or str(getattr(image, "dtype", "")) == "torch.uint16":
        raise ValueError(f"{what}: depth 16 (uint16 images) not supported")


def check_depth16_filter(f) -> None:
    """Depth 16 runs the gaussian only: every backend raises this error."""
    g = get_filter("gaussian")
    if (f.taps, f.divisor) != (g.taps, g.divisor):
        raise ValueError(f"depth 16 (uint16 images) runs the gaussian filter only, not {f.name!r}")


def numpy_step(img: np.ndarray, filt="gaussian", border: str = "zero") -> np.ndarray:
    f = get_filter(filt)
    dt = sample_dtype(img)
    if dt == np.uint16:
        check_depth16_filter(f)
    top = int(np.iinfo(dt).max)
    x = _as_hwc(np.asarray(img, dtype=dt))
    h, w, _ = x.shape
    p = np.pad(x, ((1, 1), (1, 1), (0, 0)), mode="edge" if check_border(border) == "replicate" else "constant")
    if f.int_exact or dt == np.uint16:
        acc = np.zeros(x.shape, dtype=np.int64)
        for k in range(3):
            for l in range(3):
                t = f.taps[3 * k + l]
                if t:
                    acc += t * p[k : k + h, l : l + w].astype(np.int64)
        out = np.minimum(acc >> f.shift, top).astype(dt)
    else:
        acc = np.zeros(x.shape, dtype=np.float32)
        w32 = f.weights32
        for k in range(3):
            for l in range(3):
                prod = p[k : k + h, l : l + w].astype(np.float32) * w32[k, l]
                acc = (acc + prod).astype(np.float32)
        acc = np.where(acc > 0, acc, 0).astype(np.float32)
        out = np.minimum(np.trunc(acc), 255).astype(np.uint8)
    return out.reshape(img.shape)


def numpy_convolve(img: np.ndarray, reps: int = 1, filt="gaussian", border: str = "zero") -> np.ndarray:
    check_border(border)
    out = np.asarray(img, dtype=sample_dtype(img)).copy()
    if out.dtype == np.uint16:
        check_depth16_filter(get_filter(filt))
    for _ in range(int(reps)):
        out = numpy_step(out, filt, border)
    return out


MAX_DECIMATE = 64


def check_decimate(decimate) -> int:
    """A decimation factor: an integer in [1, 64] (``ValueError`` otherwise)."""
    if isinstance(decimate, bool) or not isinstance(decimate, (int, np.integer)):
        raise ValueError(f"decimate must be an integer in [1, {MAX_DECIMATE}], got {decimate!r}")
    if not 1 <= int(decimate) <= MAX_DECIMATE:
        raise ValueError(f"decimate must be an integer in [1, {MAX_DECIMATE}], got {decimate!r}")
    return int(decimate)


def decimated_shape(shape, s: int) -> tuple:
    """Shape of an ``(H, W[, C])`` image decimated by ``s``: ceil of H and W."""
    return (-(-int(shape[0]) // s), -(-int(shape[1]) // s)) + tuple(int(d) for d in shape[2:])


def numpy_decimate(img: np.ndarray, s: int) -> np.ndarray:
    """Every ``s``-th pixel of every ``s``-th row, phase 0 (pixel (0, 0) is
    always kept): ``img[::s, ::s]`` as a contiguous array of
    ``ceil(H / s) x ceil(W / s)`` pixels.  ``decimate=s`` of every entry point
    returns ``numpy_decimate(<the undecimated result>, s)``."""
    s = check_decimate(s)
    return np.ascontiguousarray(np.asarray(img)[::s, ::s])


def check_unsharp_amount(amount) -> int:
    """``k = amount * 16`` of an unsharp mask: an exact integer in [1, 255]
    (``ValueError`` otherwise; a sequence of amounts is refused by name)."""
    if isinstance(amount, (list, tuple, dict, np.ndarray)) or hasattr(amount, "shape") and tuple(amount.shape):
        raise ValueError("unsharp: per-channel amounts are not supported (one amount applies to every channel)")
    bad = f"unsharp amount must be a multiple of 1/16 in [0.0625, 15.9375], got {amount!r}"
    if isinstance(amount, bool) or not isinstance(amount, (int, float, np.integer, np.floating)):
        raise ValueError(bad)
    k = float(amount) * 16.0
    if not (1.0 <= k <= 255.0) or k != int(k):
        raise ValueError(bad)
    return int(k)


def refuse_unsharp(what: str, unsharp=None, threshold=0) -> None:
    """The named error of everything the unsharp mask is not built for: raised
    when a caller passes ``unsharp`` (or a threshold for it) to ``what``."""
    if unsharp is not None or threshold not in (0, None):
        raise ValueError(f"{what}: unsharp is not supported (use pconv.unsharp, Engine.unsharp or "
                         f"BatchEngine.unsharp on the image itself)")


def check_unsharp_threshold(threshold, depth: int) -> int:
    """An unsharp threshold: an integer in [0, 255] (depth 16: [0, 65535])."""
    top = 65535 if depth == 16 else 255
    bad = f"unsharp threshold must be an integer in [0, {top}], got {threshold!r}"
    if isinstance(threshold, bool) or not isinstance(threshold, (int, np.integer)):
        raise ValueError(bad)
    if not 0 <= int(threshold) <= top:
        raise ValueError(bad)
    return int(threshold)


def numpy_unsharp(img: np.ndarray, reps: int, amount=1.0, threshold=0, filt="gaussian",
                  border: str = "zero") -> np.ndarray:
    """Unsharp mask, ``x + amount * (x - blur(x))`` in exact integers.  With
    ``b = numpy_convolve(img, reps, filt, border)``, ``k = amount * 16`` (an
    integer in [1, 255]), ``t = threshold`` and ``max`` = 255 or 65535, per
    sample (every channel alike)::

        d   = x - b
        out = x                                            if |d| < t
        out = clamp((x (16 + k) - b k + 8) >> 4, 0, max)   otherwise

    The shift is arithmetic (floor).  ``reps = 0`` returns the input."""
    x = np.asarray(img, dtype=sample_dtype(img))
    depth = 16 if x.dtype == np.uint16 else 8
    k = check_unsharp_amount(amount)
    t = check_unsharp_threshold(threshold, depth)
    top = int(np.iinfo(x.dtype).max)
    xs = x.astype(np.int64)
    bs = numpy_convolve(x, reps, filt, border).astype(np.int64)
    sharp = np.clip((xs * (16 + k) - bs * k + 8) >> 4, 0, top)
    return np.where(np.abs(xs - bs) < t, xs, sharp).astype(x.dtype)


def numpy_residual(img: np.ndarray, filt="gaussian", border: str = "zero") -> int:
    """Bytes of ``img`` that one more repetition would change; 0 means ``img``
    is a fixed point of the iterated map.  By definition
    ``count_nonzero(numpy_convolve(img, 1, filt, border) != img)``."""
    if sample_dtype(img) == np.uint16:
        raise ValueError("residual: depth 16 (uint16 images) not supported")
    x = np.asarray(img, dtype=np.uint8)
    return int(np.count_nonzero(numpy_convolve(x, 1, filt, border) != x))
