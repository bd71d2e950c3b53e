"""Gaussian pyramids: blur, keep every second pixel, repeat.

Level 0 is the input itself and level k + 1 is ``convolve(level k, reps,
filter, border=border, decimate=2)`` — with the default two repetitions of the
``[1,2,1] x [1,2,1]`` gaussian, the classic 5x5 REDUCE step of Burt and
Adelson.  The reference programs have no such mode: a user of theirs downloads
every blurred level, slices it on the host and uploads the kept quarter again.

On the ``hip`` backend a :class:`Pyramid` keeps one :class:`Engine` per level
below the top.  The input is uploaded once; every further level's input is
written by the decimation kernel straight from the level above
(``BandEngine.upload_decimated_from``), and every level >= 1 is downloaded once,
already decimated.  A CUDA tensor never touches the host.

Out of scope: pyramids of batches, a phase other than 0, factors other than 2
between levels, any filtering other than the repetitions already run, and the
unsharp mask (``unsharp=`` is refused by name: sharpen a level afterwards).
"""
from __future__ import annotations

from collections import OrderedDict
from typing import List, Optional, Tuple

import numpy as np
import torch

from ..models.filters import get_filter
from .reference import check_border, refuse_unsharp
from .stencil import (_CH_COUNT, _NP_DTYPE, Engine, _bytes_of, _check_depth, _check_tensor_dtype, _host_samples,
                      _resolve_backend, convolve, image_depth, image_geometry)


def pyramid_sizes(width: int, height: int) -> List[Tuple[int, int]]:
    """``[(width, height)]`` of every level of a pyramid of a ``width`` x
    ``height`` image, up to and including the first 1x1 level."""
    w, h = int(width), int(height)
    if w < 1 or h < 1:
        raise ValueError("image sizes must be >= 1x1")
    sizes = [(w, h)]
    while (w, h) != (1, 1):
        w, h = -(-w // 2), -(-h // 2)
        sizes.append((w, h))
    return sizes


def _check_levels(width: int, height: int, levels) -> int:
    if isinstance(levels, bool) or not isinstance(levels, (int, np.integer)) or int(levels) < 1:
        raise ValueError(f"levels must be an integer >= 1, got {levels!r}")
    most = len(pyramid_sizes(width, height))
    if int(levels) > most:
        raise ValueError(f"levels {int(levels)} exceeds the {most} levels of a {width}x{height} image "
                         f"(up to and including its first 1x1 level)")
    return int(levels)


class Pyramid:
    """Persistent single-GPU pyramid builder for one image geometry.

    Owns one :class:`Engine` per level below the top (its own engines, outside
    the 8-entry cache of :func:`convolve`).  ``__call__(img)`` returns the list
    of ``levels`` images in the input's container and on its device.
    """

    def __init__(self, width: int, height: int, channels: str = "grey", levels: int = 1, reps: int = 2,
                 filter="gaussian", border: str = "zero", device: int = 0, depth: int = 8, unsharp=None):
        refuse_unsharp("Pyramid", unsharp)
        if reps < 0:
            raise ValueError("reps must be >= 0")
        if channels not in _CH_COUNT:
            raise ValueError(f"unknown channels {channels!r}")
        self.levels = _check_levels(width, height, levels)
        self.width, self.height, self.channels = int(width), int(height), channels
        self.reps = int(reps)
        self.filter = get_filter(filter)
        self.border = check_border(border)
        self.depth = _check_depth(int(depth), self.filter)
        self.device = int(device)
        self.sizes = pyramid_sizes(self.width, self.height)[:self.levels]
        self._engines = [Engine(w, h, channels, self.filter, device=self.device, border=self.border,
                                depth=self.depth) for w, h in self.sizes[:-1]]

    def _level_shape(self, shape, k: int) -> tuple:
        w, h = self.sizes[k]
        return (h, w) + tuple(int(d) for d in shape[2:])

    def __call__(self, img) -> list:
        is_tensor = isinstance(img, torch.Tensor)
        _check_tensor_dtype(img)
        if image_geometry(tuple(img.shape)) != (self.width, self.height, self.channels):
            raise ValueError(f"image of shape {tuple(img.shape)} is no {self.width}x{self.height} "
                             f"{self.channels} image")
        if image_depth(img) != self.depth:
            raise TypeError(f"pyramid of depth {self.depth} got a {img.dtype} image")
        on_gpu = is_tensor and img.device.type == "cuda"
        engs = [e._eng for e in self._engines]
        if on_gpu:
            src = img.contiguous()
            outs = [src]
            if not engs:
                return outs
            ts = torch.cuda.current_stream(src.device).cuda_stream
            engs[0].wait_stream(ts)
            engs[0].upload_ptr(src.data_ptr(), self._engines[0].row_bytes, 0, self.height, device=True)
        else:
            src = _host_samples(img, self.depth)
            outs = [torch.from_numpy(src) if is_tensor else src]
            if not engs:
                return outs
            engs[0].upload(_bytes_of(src), 0, self.height)
        for k, e in enumerate(engs):
            e.run(self.reps)
            shape = self._level_shape(src.shape, k + 1)
            if on_gpu:
                out = torch.empty(shape, dtype=src.dtype, device=src.device)
                e.download_decimated_ptr(out.data_ptr(), e.decimated_row_bytes(2), 2, device=True)
            else:
                out = np.empty(shape, dtype=_NP_DTYPE[self.depth])
                e.download_decimated(_bytes_of(out), 2)
            outs.append(out)
            if k + 1 < len(engs):
                # the next level's input never leaves the device; level k's frame
                # may be overwritten (by the next call) only after that read
                engs[k + 1].upload_decimated_from(e, 2)
                e.wait_stream(engs[k + 1].compute_stream)
        if on_gpu:
            for e in engs:
                e.signal_stream(ts)
            src.record_stream(torch.cuda.current_stream(src.device))
            return outs
        for e in engs:
            e.synchronize()
        return [torch.from_numpy(o) if is_tensor and isinstance(o, np.ndarray) else o for o in outs]


# pyramid()'s own cache: at most two Pyramid objects (each owns its engines).
_PYRAMIDS: "OrderedDict[tuple, Pyramid]" = OrderedDict()
_MAX_CACHED_PYRAMIDS = 2


def _cached_pyramid(w, h, ch, levels, reps, flt, border, device, depth) -> Pyramid:
    key = (w, h, ch, levels, reps, flt.taps, flt.divisor, border, device, depth)
    pyr = _PYRAMIDS.get(key)
    if pyr is None:
        while len(_PYRAMIDS) >= _MAX_CACHED_PYRAMIDS:  # make room first: device frames of every level
            _PYRAMIDS.popitem(last=False)
        pyr = Pyramid(w, h, ch, levels, reps, flt, border, device, depth)
        _PYRAMIDS[key] = pyr
    else:
        _PYRAMIDS.move_to_end(key)
    return pyr


def pyramid(image, levels: int, reps: int = 2, filter="gaussian", border: str = "zero", backend: str = "auto",
            device: Optional[int] = None, unsharp=None) -> list:
    """The ``levels`` levels of the pyramid of ``image``, a list: level 0 is the
    input itself, level k + 1 is ``convolve(level k, reps, filter,
    border=border, decimate=2)``.  ``levels`` may not exceed the number of
    levels up to and including the first 1x1 one (``ValueError``).

    Every backend returns the same bytes, in the input's container and on its
    device.  ``hip`` runs through a cached :class:`Pyramid` (at most two are
    kept): one upload, the levels handed down on the device, one decimated
    download per level.  The other backends chain :func:`convolve` calls.
    """
    refuse_unsharp("pyramid", unsharp)
    if reps < 0:
        raise ValueError("reps must be >= 0")
    flt = get_filter(filter)
    check_border(border)
    _check_tensor_dtype(image)
    w, h, ch = image_geometry(tuple(image.shape))
    levels = _check_levels(w, h, levels)
    depth = _check_depth(image_depth(image), flt)
    backend = _resolve_backend(image, backend)
    if backend == "hip":
        if device is None:
            is_cuda = isinstance(image, torch.Tensor) and image.is_cuda
            device = image.device.index if is_cuda else 0
        return _cached_pyramid(w, h, ch, levels, int(reps), flt, border, int(device or 0), depth)(image)
    outs = [image]
    for _ in range(levels - 1):
        outs.append(convolve(outs[-1], reps, flt, backend=backend, border=border, decimate=2))
    return outs
