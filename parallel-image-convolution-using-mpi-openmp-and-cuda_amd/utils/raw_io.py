"""Raw 8-bit (or 16-bit little-endian, ``depth=16``) image files (headerless, row-major, interleaved channels).

Reference I/O: MPI-IO band reads/writes (``mpi/mpi_convolution.c:126-140,
244-262``) and POSIX ``read_info``/``write_info`` (``cuda/functions.c:31-45``).
The native layer does the real work (pread/pwrite at 64-bit offsets, size
validation, ``O_TRUNC``); these helpers return NumPy arrays shaped (H, W[, C]).
"""
from __future__ import annotations

import os

import numpy as np

from .._native import require_native

_CH = {"grey": 1, "rgb": 3, "rgba": 4}


def _shape(width: int, height: int, channels: str):
    c = _CH[channels]
    return (height, width) if c == 1 else (height, width, c)


def output_path_for(path: str, prefix: str = "blur_") -> str:
    """``dir/x.raw`` -> ``dir/blur_x.raw`` (reference: ``"blur_" + argv[1]``)."""
    d, b = os.path.split(path)
    return os.path.join(d, prefix + b) if d else prefix + b


_DTYPE = {8: np.uint8, 16: np.dtype("<u2")}


def _check_depth(depth: int) -> int:
    if depth not in _DTYPE:
        raise ValueError(f"depth must be 8 or 16, got {depth!r}")
    return depth


def read_raw(path: str, width: int, height: int, channels: str = "grey", depth: int = 8) -> np.ndarray:
    """The file as ``uint8``, or (``depth=16``: little-endian 16-bit samples) ``uint16``."""
    out = np.empty(_shape(width, height, channels), dtype=_DTYPE[_check_depth(depth)])
    require_native().read_raw(path, out.reshape(-1).view(np.uint8), width, height, channels, depth=depth)
    return out.astype(np.uint16, copy=False) if depth == 16 else out


def write_raw(path: str, img: np.ndarray, depth: int | None = None) -> None:
    """``depth=None``: 16 for a ``uint16`` array (written little-endian), else 8."""
    if depth is None:
        depth = 16 if getattr(img, "dtype", None) == np.uint16 else 8
    arr = np.ascontiguousarray(img, dtype=_DTYPE[_check_depth(depth)])
    h, w = arr.shape[:2]
    ch = {2: "grey"}.get(arr.ndim) or {1: "grey", 3: "rgb", 4: "rgba"}[arr.shape[2]]
    require_native().write_raw(path, arr.reshape(-1).view(np.uint8), w, h, ch, depth=depth)


def synthetic_image(width: int, height: int, channels: str = "grey", seed: int = 0, y0: int = 0,
                    rows: int | None = None, depth: int = 8) -> np.ndarray:
    """Deterministic random-byte image (or rows [y0, y0+rows) of it) — the
    same bytes the native ``--synthetic SEED`` generator produces.  ``depth=16``:
    the same byte generator over the twice-as-wide row, read as little-endian
    16-bit samples (so any band split still generates identical rows)."""
    rows = height - y0 if rows is None else rows
    out = np.empty(_shape(width, rows, channels), dtype=_DTYPE[_check_depth(depth)])
    require_native().synth_rows(out.reshape(-1).view(np.uint8), width, height, channels, int(seed), int(y0),
                                int(rows), depth=depth)
    return out.astype(np.uint16, copy=False) if depth == 16 else out
