"""Stencil operators: the user-facing ``convolve`` and the persistent ``Engine``.

``convolve`` is the library form of the reference programs (repeated 3x3
convolution of an 8-bit grey/RGB image, zero padded — or, with
``border="replicate"``, with the image's edge pixels repeated): it dispatches to

* ``hip``   — the native CDNA4 kernels through a cached single-GPU
  :class:`Engine` (device-resident ping-pong frames, ``cuda/cuda_convolution.cu``
  analogue);
* ``omp`` / ``cpu`` — the native OpenMP / serial oracle (``open-mp/``, ``mpi/``);
* ``numpy`` — the independent pure-NumPy oracle (tests).

Images are ``(H, W)`` grey, ``(H, W, 3)`` RGB or ``(H, W, 4)`` RGBA uint8
arrays or tensors; CUDA tensors stay on the device (D2D copies on the
engine's stream, ordered after/before torch's current stream).
"""
from __future__ import annotations

from collections import OrderedDict
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from .._native import require_native
from ..models.filters import get_filter
from .reference import (check_border, check_decimate, check_depth16_filter, check_unsharp_amount,
                        check_unsharp_threshold, decimated_shape, numpy_convolve, numpy_decimate, numpy_residual,
                        numpy_step, numpy_unsharp, refuse_unsharp)

_CHANNELS = {1: "grey", 3: "rgb", 4: "rgba"}
_CH_COUNT = {"grey": 1, "rgb": 3, "rgba": 4}
_NP_DTYPE = {8: np.uint8, 16: np.uint16}
_TORCH_DTYPE = {8: torch.uint8, 16: torch.uint16}


def image_depth(image) -> int:
    """Bits per sample an image selects: 16 for dtype ``uint16`` (NumPy or
    ``torch.uint16``), 8 for everything else."""
    return 16 if getattr(image, "dtype", None) in (np.uint16, torch.uint16) else 8


def _check_tensor_dtype(image) -> None:
    if isinstance(image, torch.Tensor) and image.dtype not in (torch.uint8, torch.uint16):
        raise TypeError("image tensor must be uint8 (or uint16 for depth 16)")


def _check_depth(depth: int, flt, variant: str = "auto", graph: bool = False) -> int:
    """What depth 16 runs: the gaussian on the auto / temporal kernel, no graph replay."""
    if depth not in (8, 16):
        raise ValueError(f"depth must be 8 or 16, got {depth!r}")
    if depth == 16:
        check_depth16_filter(flt)
        if variant not in ("auto", "temporal"):
            raise ValueError(f"depth 16 (uint16 images) not supported by kernel {variant!r} (auto|temporal only)")
        if graph:
            raise ValueError("depth 16 (uint16 images) not supported with graph=True")
    return depth


def _refuse_depth16(image, what: str) -> None:
    if image_depth(image) == 16:
        raise ValueError(f"{what}: depth 16 (uint16 images) not supported")


def _host_samples(image, depth: int) -> np.ndarray:
    """``image`` (array or tensor) as a C-contiguous host array of the depth's dtype."""
    if isinstance(image, torch.Tensor):
        image = image.cpu().numpy()
    return np.ascontiguousarray(image, dtype=_NP_DTYPE[depth])


def _bytes_of(arr: np.ndarray) -> np.ndarray:
    """The flat byte view the native bindings take."""
    return arr.reshape(-1).view(np.uint8)


def image_geometry(shape) -> Tuple[int, int, str]:
    """(width, height, channels-name) of an (H, W[, C]) image."""
    if len(shape) == 2:
        return int(shape[1]), int(shape[0]), "grey"
    if len(shape) == 3 and int(shape[2]) in _CHANNELS:
        return int(shape[1]), int(shape[0]), _CHANNELS[int(shape[2])]
    raise ValueError(f"unsupported image shape {tuple(shape)}: expected (H, W) or (H, W, 1|3|4)")


@dataclass(frozen=True)
class StableInfo:
    """Outcome of a run to the fixed point: repetitions actually run, whether
    the returned image is a fixed point, the last check's count of bytes one
    more repetition would change (it describes the returned image), and the
    number of checks made."""

    reps_done: int
    converged: bool
    residual: int
    checks: int


# Default check intervals.  CPU backends: a check costs about one repetition,
# so one per 32 adds ~3 %.  GPU: 16 fused launches per check.  A check is the
# residual launch (about half a fused launch, as its traffic says) plus ~20 us
# of read-back and kernel boundaries; at 4 launches per check that measured
# +28 % on a 1920x2520 RGB loop, at 16 +8.5 % (docs/PERFORMANCE.md 3.2), and
# the up to 16 x fuse - 1 repetitions run past the fixed point are few against
# the hundreds to thousands it takes to reach one.
_CPU_CHECK_EVERY = 32
_GPU_CHECK_LAUNCHES = 16


def _check_stable_args(max_reps, check_every):
    """The argument checks every run to the fixed point shares:
    ``(int(max_reps), int(check_every) or None for the caller's default)``."""
    if max_reps < 0:
        raise ValueError("max_reps must be >= 0")
    if check_every is not None and int(check_every) < 1:
        raise ValueError("check_every must be >= 1")
    return int(max_reps), None if check_every is None else int(check_every)


def _stable_info(st) -> StableInfo:
    """The native engines' (reps_done, converged, residual, checks)."""
    return StableInfo(int(st[0]), bool(st[1]), int(st[2]), int(st[3]))


class Engine:
    """Persistent single-GPU convolution engine for one image geometry.

    Device frames are allocated once; every call uploads, runs ``reps``
    repetitions with the fused kernels and downloads the newest buffer.
    """

    def __init__(self, width: int, height: int, channels: str = "grey", filter="gaussian", device: int = 0,
                 fuse: Optional[int] = None, graph: bool = False, variant: str = "auto", border: str = "zero",
                 depth: int = 8):
        n = require_native()
        self.border = check_border(border)
        self.filter = get_filter(filter)
        self.depth = _check_depth(int(depth), self.filter, variant, graph)
        nf = self.filter.to_native()
        if fuse is None:
            ch = _CH_COUNT[channels]
            fuse = n.auto_fuse(nf, variant, int(width) * int(height) * ch * (self.depth // 8), ch, depth=self.depth)
        self.width, self.height, self.channels = int(width), int(height), channels
        self.device = int(device)
        self.graph = bool(graph)
        self._eng = n.BandEngine(self.width, self.height, channels, nf, 0, 1, self.device, halo=int(fuse),
                                 fuse=int(fuse), overlap=True, graph=bool(graph), variant=variant,
                                 border=self.border, depth=self.depth)
        self.row_bytes = self._eng.row_bytes

    @property
    def fuse(self) -> int:
        return self._eng.fuse

    @property
    def stats(self):
        return self._eng.stats

    def plan(self, reps: int):
        return self._eng.plan(reps)

    def _check_samples(self, img) -> None:
        """A uint16 image on a depth-8 engine would be wrapped modulo 256, a
        device tensor of the other width misread: both are errors."""
        if image_depth(img) != self.depth and (self.depth == 8 or isinstance(img, torch.Tensor)):
            raise TypeError(f"engine of depth {self.depth} got a {img.dtype} image")

    def run_numpy(self, img: np.ndarray, reps: int, decimate: int = 1) -> np.ndarray:
        """``decimate=s``: every s-th pixel of every s-th row of the result
        (``numpy_decimate``) — one decimation launch on the device, and only the
        kept bytes are downloaded."""
        s = check_decimate(decimate)
        self._check_samples(img)
        src = _host_samples(img, self.depth)
        out = np.empty_like(src) if s == 1 else np.empty(decimated_shape(src.shape, s), dtype=src.dtype)
        self._eng.upload(_bytes_of(src), 0, self.height)
        self._eng.run(int(reps))
        if s == 1:
            self._eng.download(_bytes_of(out), 0, self.height)
        else:
            self._eng.download_decimated(_bytes_of(out), s)
        self._eng.synchronize()
        return out

    def run_tensor(self, t: torch.Tensor, reps: int, decimate: int = 1) -> torch.Tensor:
        s = check_decimate(decimate)
        self._check_samples(t)
        if t.device.type != "cuda":
            return torch.from_numpy(self.run_numpy(t.numpy(), reps, s))
        src = t.contiguous()
        out = (torch.empty_like(src) if s == 1 else
               torch.empty(decimated_shape(src.shape, s), dtype=src.dtype, device=src.device))
        ts = torch.cuda.current_stream(src.device).cuda_stream
        self._eng.wait_stream(ts)
        self._eng.upload_ptr(src.data_ptr(), self.row_bytes, 0, self.height, device=True)
        self._eng.run(int(reps))
        if s == 1:
            self._eng.download_ptr(out.data_ptr(), self.row_bytes, 0, self.height, device=True)
        else:  # the kernel writes the result tensor itself
            self._eng.download_decimated_ptr(out.data_ptr(), self._eng.decimated_row_bytes(s), s, device=True)
        self._eng.signal_stream(ts)
        src.record_stream(torch.cuda.current_stream(src.device))
        return out

    def __call__(self, img, reps: int, decimate: int = 1):
        if isinstance(img, torch.Tensor):
            return self.run_tensor(img, reps, decimate)
        return self.run_numpy(np.asarray(img), reps, decimate)

    # ---- unsharp mask --------------------------------------------------
    def unsharp(self, img, reps: int, amount=1.0, threshold=0):
        """``numpy_unsharp(img, reps, amount, threshold, ...)``: ``x + amount *
        (x - blur(x))`` per sample, in exact integers.  The image is uploaded
        once; one device copy keeps the original beside the frames, ``reps``
        repetitions run as in ``__call__``, one pointwise launch combines the
        two in place, and the sharpened frame is downloaded.  Same container
        and device as ``img`` (a CUDA tensor never leaves the device)."""
        k = check_unsharp_amount(amount)
        t = check_unsharp_threshold(threshold, self.depth)
        if int(reps) < 0:
            raise ValueError("reps must be >= 0")
        if self.graph:
            raise ValueError("unsharp: hipGraph capture (graph=True) is not supported")
        self._check_samples(img)
        e = self._eng
        if isinstance(img, torch.Tensor) and img.device.type == "cuda":
            src = img.contiguous()
            out = torch.empty_like(src)
            ts = torch.cuda.current_stream(src.device).cuda_stream
            e.wait_stream(ts)
            e.upload_ptr(src.data_ptr(), self.row_bytes, 0, self.height, device=True)
            e.snapshot_original()
            e.run(int(reps))
            e.apply_unsharp(k, t)
            e.download_ptr(out.data_ptr(), self.row_bytes, 0, self.height, device=True)
            e.signal_stream(ts)
            src.record_stream(torch.cuda.current_stream(src.device))
            return out
        is_tensor = isinstance(img, torch.Tensor)
        src = _host_samples(img, self.depth)
        out = np.empty_like(src)
        e.upload(_bytes_of(src), 0, self.height)
        e.snapshot_original()
        e.run(int(reps))
        e.apply_unsharp(k, t)
        e.download(_bytes_of(out), 0, self.height)
        e.synchronize()
        return torch.from_numpy(out) if is_tensor else out

    # ---- fixed point -------------------------------------------------
    def _with_frame(self, img, work):
        """Upload ``img`` (array or tensor), ``work()`` on the resident frame,
        download the newest frame into the input's container type."""
        _refuse_depth16(img, "residual / run_until_stable")
        if self.depth == 16:
            raise ValueError("residual / run_until_stable: depth 16 not supported")
        if isinstance(img, torch.Tensor) and img.device.type == "cuda":
            src = img.contiguous()
            out = torch.empty_like(src)
            ts = torch.cuda.current_stream(src.device).cuda_stream
            self._eng.wait_stream(ts)
            self._eng.upload_ptr(src.data_ptr(), self.row_bytes, 0, self.height, device=True)
            res = work()
            self._eng.download_ptr(out.data_ptr(), self.row_bytes, 0, self.height, device=True)
            self._eng.signal_stream(ts)
            src.record_stream(torch.cuda.current_stream(src.device))
            return out, res
        is_tensor = isinstance(img, torch.Tensor)
        src = np.ascontiguousarray(img.numpy() if is_tensor else img, dtype=np.uint8)
        out = np.empty_like(src)
        self._eng.upload(src.reshape(-1), 0, self.height)
        res = work()
        self._eng.download(out.reshape(-1), 0, self.height)
        self._eng.synchronize()
        return (torch.from_numpy(out) if is_tensor else out), res

    def residual(self, img=None) -> int:
        """Bytes one more repetition would change: of ``img``, or (``None``) of
        the frame the engine holds after its last run."""
        if img is None:
            if self.depth == 16:
                raise ValueError("residual: depth 16 not supported")
            return int(self._eng.residual())
        return int(self._with_frame(img, self._eng.residual)[1])

    def run_until_stable(self, img, max_reps: int, check_every: Optional[int] = None):
        """Repetitions in chunks of ``check_every`` (default 16 x fuse) with a
        residual check after each, stopping at the first fixed point or at
        ``max_reps``; returns ``(image, StableInfo)``."""
        max_reps, k = _check_stable_args(max_reps, check_every)
        if k is None:
            k = _GPU_CHECK_LAUNCHES * self.fuse
        out, st = self._with_frame(img, lambda: self._eng.run_until_stable(max_reps, k))
        return out, _stable_info(st)


_ENGINES: "OrderedDict[tuple, Engine]" = OrderedDict()
_MAX_CACHED = 8


def _cached_engine(w, h, ch, flt, device, fuse, graph, variant, border="zero", depth=8) -> Engine:
    key = (w, h, ch, flt.taps, flt.divisor, device, fuse, graph, variant, border, depth)
    eng = _ENGINES.get(key)
    if eng is None:
        eng = Engine(w, h, ch, flt, device=device, fuse=fuse, graph=graph, variant=variant, border=border,
                     depth=depth)
        _ENGINES[key] = eng
        while len(_ENGINES) > _MAX_CACHED:
            _ENGINES.popitem(last=False)
    else:
        _ENGINES.move_to_end(key)
    return eng


def _default_backend() -> str:
    try:
        require_native()
    except ImportError:
        return "numpy"
    return "hip" if torch.cuda.is_available() else "omp"


def convolve(image, reps: int = 1, filter="gaussian", backend: str = "auto", device: Optional[int] = None,
             fuse: Optional[int] = None, graph: bool = False, variant: str = "auto", threads: int = 0,
             border: str = "zero", decimate: int = 1):
    """Apply ``reps`` 3x3 convolutions to an 8-bit image, or (dtype ``uint16``,
    NumPy or ``torch.uint16``: depth 16, the gaussian only) to a 16-bit one.

    ``border``: what a tap reads outside the image — ``"zero"`` (default, the
    reference's zero padding) or ``"replicate"`` (the nearest image pixel: no
    dark frame after many repetitions), on every backend.

    ``decimate=s`` (an integer in 1..64): return every s-th pixel of every s-th
    row of the result, ``out[Y, X] = blurred[Y * s, X * s]`` with
    ``ceil(H / s) x ceil(W / s)`` pixels (pixel (0, 0) is always kept) —
    ``numpy_decimate(convolve(image, reps, ...), s)`` on every backend.  On
    ``hip`` the slicing is one kernel launch and only the kept bytes are
    copied back; ``s = 1`` is the plain call, launch for launch.

    Returns the same container type as the input (NumPy array or torch tensor
    on the same device).
    """
    if reps < 0:
        raise ValueError("reps must be >= 0")
    s = check_decimate(decimate)
    flt = get_filter(filter)
    check_border(border)
    is_tensor = isinstance(image, torch.Tensor)
    _check_tensor_dtype(image)
    depth = image_depth(image)
    w, h, ch = image_geometry(tuple(image.shape))
    if backend == "auto":
        backend = "hip" if (is_tensor and image.is_cuda) else _default_backend()
    if backend not in ("numpy", "cpu", "omp", "hip"):
        raise ValueError(f"unknown backend {backend!r} (hip|omp|cpu|numpy|auto)")
    _check_depth(depth, flt, variant if backend == "hip" else "auto", graph and backend == "hip")

    if backend == "numpy":
        arr = image.cpu().numpy() if is_tensor else np.asarray(image)
        out = numpy_convolve(arr, reps, flt, border)
        if s > 1:
            out = numpy_decimate(out, s)
        return torch.from_numpy(out).to(image.device) if is_tensor else out

    if backend in ("cpu", "omp"):
        n = require_native()
        arr = _host_samples(image, depth)
        if s == 1:
            out = np.empty_like(arr)
            n.cpu_convolve(_bytes_of(arr), _bytes_of(out), w, h, ch, int(reps), flt.to_native(), backend == "omp",
                           int(threads), border=border, depth=depth)
        else:
            out = np.empty(decimated_shape(arr.shape, s), dtype=arr.dtype)
            n.cpu_convolve(_bytes_of(arr), _bytes_of(out), w, h, ch, int(reps), flt.to_native(), backend == "omp",
                           int(threads), border=border, depth=depth, decimate=s)
        return torch.from_numpy(out).to(image.device) if is_tensor else out

    if backend == "hip":
        if device is None:
            device = image.device.index if (is_tensor and image.is_cuda) else 0
        eng = _cached_engine(w, h, ch, flt, int(device or 0), fuse, graph, variant, border, depth)
        return eng(image, reps) if s == 1 else eng(image, reps, s)

    raise ValueError(f"unknown backend {backend!r} (hip|omp|cpu|numpy|auto)")


def _resolve_backend(image, backend: str) -> str:
    if backend == "auto":
        is_cuda = isinstance(image, torch.Tensor) and image.is_cuda
        return "hip" if is_cuda else _default_backend()
    if backend not in ("hip", "omp", "cpu", "numpy"):
        raise ValueError(f"unknown backend {backend!r} (hip|omp|cpu|numpy|auto)")
    return backend


def _refuse_unsharp_decimate(decimate) -> None:
    if decimate != 1:
        raise ValueError("unsharp: decimate is not supported (thumbnail pipelines sharpen after downscaling, not "
                         "before: decimate first, then sharpen the small image)")


def unsharp(image, reps: int = 1, amount=1.0, threshold=0, filter="gaussian", backend: str = "auto",
            device: Optional[int] = None, threads: int = 0, border: str = "zero", fuse: Optional[int] = None,
            variant: str = "auto", decimate: int = 1):
    """Unsharp mask: ``x + amount * (x - convolve(x, reps, filter, border))``
    per sample, rounded to nearest and clamped, in exact integers — the
    "sharpen" that goes with :func:`convolve`'s "blur".

    ``amount``: a multiple of 1/16 in [0.0625, 15.9375] (one amount for every
    channel, an RGBA image's fourth included).  ``threshold`` (an integer in
    [0, 255], depth 16: [0, 65535]): samples whose difference to the blurred
    image is below it keep their value.  The result is
    ``numpy_unsharp(image, reps, amount, threshold, filter, border)`` on every
    backend (``hip | omp | cpu | numpy | auto``), in the input's container and
    on its device.  On ``hip`` the image is uploaded once, the original stays
    on the device beside the frames, and one pointwise launch combines the two
    before the download; a CUDA tensor never leaves the device.

    Out of scope, refused by name: ``decimate`` above 1, per-channel amounts,
    hipGraph capture, differences of two blurs.
    """
    if reps < 0:
        raise ValueError("reps must be >= 0")
    _refuse_unsharp_decimate(decimate)
    flt = get_filter(filter)
    check_border(border)
    is_tensor = isinstance(image, torch.Tensor)
    _check_tensor_dtype(image)
    depth = image_depth(image)
    k = check_unsharp_amount(amount)
    t = check_unsharp_threshold(threshold, depth)
    w, h, ch = image_geometry(tuple(image.shape))
    backend = _resolve_backend(image, backend)
    _check_depth(depth, flt, variant if backend == "hip" else "auto")

    if backend == "numpy":
        arr = image.cpu().numpy() if is_tensor else np.asarray(image)
        out = numpy_unsharp(arr, reps, amount, t, flt, border)
        return torch.from_numpy(out).to(image.device) if is_tensor else out

    if backend in ("cpu", "omp"):
        arr = _host_samples(image, depth)
        out = np.empty_like(arr)
        require_native().cpu_unsharp_convolve(_bytes_of(arr), _bytes_of(out), w, h, ch, int(reps), k, t,
                                              flt.to_native(), backend == "omp", int(threads), border=border,
                                              depth=depth)
        return torch.from_numpy(out).to(image.device) if is_tensor else out

    if device is None:
        device = image.device.index if (is_tensor and image.is_cuda) else 0
    eng = _cached_engine(w, h, ch, flt, int(device or 0), fuse, False, variant, border, depth)
    return eng.unsharp(image, reps, amount, t)


_unsharp = unsharp  # (convolve_file's keyword of the same name shadows the function there)


def residual(image, filter="gaussian", backend: str = "auto", device: Optional[int] = None, threads: int = 0,
             border: str = "zero") -> int:
    """Bytes of ``image`` that one more repetition of ``filter`` would change
    (0: the image is a fixed point of the iterated map), on any backend."""
    flt = get_filter(filter)
    check_border(border)
    is_tensor = isinstance(image, torch.Tensor)
    _refuse_depth16(image, "residual")
    if is_tensor and image.dtype != torch.uint8:
        raise TypeError("image tensor must be uint8")
    w, h, ch = image_geometry(tuple(image.shape))
    backend = _resolve_backend(image, backend)
    if backend == "hip":
        if device is None:
            device = image.device.index if (is_tensor and image.is_cuda) else 0
        return _cached_engine(w, h, ch, flt, int(device or 0), None, False, "auto", border).residual(image)
    arr = np.ascontiguousarray(image.cpu().numpy() if is_tensor else image, dtype=np.uint8)
    if backend == "numpy":
        return numpy_residual(arr, flt, border)
    return int(require_native().cpu_residual(arr.reshape(-1), w, h, ch, flt.to_native(), backend == "omp",
                                             int(threads), border=border))


def convolve_until_stable(image, max_reps: int, filter="gaussian", check_every: Optional[int] = None,
                          backend: str = "auto", device: Optional[int] = None, fuse: Optional[int] = None,
                          graph: bool = False, variant: str = "auto", threads: int = 0, border: str = "zero",
                          unsharp=None):
    """``convolve`` that stops at the fixed point of the iterated map.

    Runs chunks of ``check_every`` repetitions (the last one shorter; default
    16 x the engine's fuse on the GPU, 32 on the CPU backends), counts after
    each chunk the bytes one more repetition would change, and stops at the
    first zero or at ``max_reps``.  From a fixed point on every further
    repetition returns the same bytes, so a converged result equals
    ``convolve(image, max_reps, ...)``.  Returns ``(out, StableInfo)``.
    """
    refuse_unsharp("convolve_until_stable", unsharp)
    _check_stable_args(max_reps, check_every)
    flt = get_filter(filter)
    check_border(border)
    is_tensor = isinstance(image, torch.Tensor)
    _refuse_depth16(image, "convolve_until_stable")
    if is_tensor and image.dtype != torch.uint8:
        raise TypeError("image tensor must be uint8")
    w, h, ch = image_geometry(tuple(image.shape))
    backend = _resolve_backend(image, backend)

    if backend == "hip":
        if device is None:
            device = image.device.index if (is_tensor and image.is_cuda) else 0
        eng = _cached_engine(w, h, ch, flt, int(device or 0), fuse, graph, variant, border)
        return eng.run_until_stable(image, int(max_reps), check_every)

    k = _CPU_CHECK_EVERY if check_every is None else int(check_every)
    arr = np.ascontiguousarray(image.cpu().numpy() if is_tensor else image, dtype=np.uint8)
    if backend == "numpy":
        out, done, checks = arr.copy(), 0, 0
        while True:
            for _ in range(min(k, int(max_reps) - done)):
                out = numpy_step(out, flt, border)
                done += 1
            res = numpy_residual(out, flt, border)
            checks += 1
            if res == 0 or done >= max_reps:
                break
        info = StableInfo(done, res == 0, res, checks)
    else:
        out = np.empty_like(arr)
        st = require_native().cpu_convolve_until_stable(arr.reshape(-1), out.reshape(-1), w, h, ch, int(max_reps), k,
                                                        flt.to_native(), backend == "omp", int(threads),
                                                        border=border)
        info = StableInfo(int(st[0]), bool(st[1]), int(st[2]), int(st[3]))
    return (torch.from_numpy(out).to(image.device) if is_tensor else out), info


# ---- image batches ----------------------------------------------------------


class BatchEngine:
    """Persistent single-GPU engine for up to ``capacity`` images of ONE
    geometry: all of a call's images advance in the same fused launches
    (``ceil(reps / fuse)`` launches whatever their number), so small images
    fill the chip together instead of paying a launch's latency each.

    ``run_numpy`` / ``run_tensor`` / ``__call__`` take a stack of
    ``n <= capacity`` images, ``(n, H, W)`` or ``(n, H, W, C)``, and return the
    same container type; a CUDA tensor never leaves the device.

    Mixed sizes: ``run_images`` / ``residual_images`` /
    ``run_images_until_stable`` take a sequence of ``n <= capacity`` images of
    ANY sizes within ``width`` x ``height`` (the engine's geometry is then an
    envelope).  Each is convolved as a lone image of its own size, in the same
    ``ceil(reps / fuse)`` launches; the results come back as a list.
    """

    def __init__(self, width: int, height: int, channels: str = "grey", capacity: int = 1, filter="gaussian",
                 device: int = 0, fuse: Optional[int] = None, variant: str = "auto", border: str = "zero",
                 depth: int = 8):
        n = require_native()
        self.border = check_border(border)
        self.filter = get_filter(filter)
        self.depth = _check_depth(int(depth), self.filter, variant)
        nf = self.filter.to_native()
        if fuse is None:
            ch = _CH_COUNT[channels]
            fuse = n.auto_fuse(nf, variant, int(width) * int(height) * ch * (self.depth // 8), ch, depth=self.depth)
        self.width, self.height, self.channels = int(width), int(height), channels
        self.device = int(device)
        self._eng = n.BatchEngine(self.width, self.height, channels, int(capacity), nf, self.device, fuse=int(fuse),
                                  variant=variant, border=self.border, depth=self.depth)
        self.capacity = self._eng.capacity
        self.row_bytes = self._eng.row_bytes
        self._n = 0  # images of the last call (residual(None) counts those)

    @property
    def fuse(self) -> int:
        return self._eng.fuse

    @property
    def stats(self):
        return self._eng.stats

    def _check_stack(self, shape) -> int:
        shape = tuple(int(s) for s in shape)
        if len(shape) not in (3, 4) or image_geometry(shape[1:]) != (self.width, self.height, self.channels):
            raise ValueError(f"stack of shape {shape} does not hold {self.width}x{self.height} {self.channels} images")
        if shape[0] > self.capacity:
            raise ValueError(f"{shape[0]} images exceed the engine's capacity {self.capacity}")
        return shape[0]

    def _transfer(self, flat, n: int, work, sizes=None, decimate: int = 1):
        """The bracket every call shares.  ``flat``: the packed samples of ``n``
        images, a 1-D NumPy array or CUDA tensor (which never leaves the
        device); ``sizes``: their ``[(width, height)]``, or ``None`` for images
        of the engine's geometry.  Waits for the caller's stream, uploads,
        ``work(n)`` on the resident frames, downloads the newest frames in the
        same packing, signals the caller's stream (host memory: synchronises):
        ``(out, work's result)``, ``(out, None)`` for no images.  ``decimate``
        above 1: the download is the decimated one (one launch for all images)
        and ``out`` holds the decimated images in the same packing."""
        e = self._eng
        self._n = n
        s = decimate
        device = isinstance(flat, torch.Tensor)
        if s == 1:
            out = torch.empty_like(flat) if device else np.empty_like(flat)
        else:
            c = _CH_COUNT[self.channels]
            dims = sizes if sizes is not None else [(self.width, self.height)] * n
            count = sum(-(-w // s) * -(-h // s) * c for w, h in dims)
            out = (torch.empty(count, dtype=flat.dtype, device=flat.device) if device
                   else np.empty(count, dtype=flat.dtype))
        if n == 0:
            return out, None
        form = ("" if sizes is None else "_sized") + ("_ptr" if device else "")
        kw = {"device": True} if device else {}
        if device:
            ts = torch.cuda.current_stream(flat.device).cuda_stream
            e.wait_stream(ts)
        getattr(e, "upload" + form)(flat.data_ptr() if device else _bytes_of(flat), n if sizes is None else sizes, **kw)
        res = work(n)
        name = ("download" + form) if s == 1 else (
            "download" + ("" if sizes is None else "_sized") + "_decimated" + ("_ptr" if device else ""))
        getattr(e, name)(out.data_ptr() if device else _bytes_of(out), *([n] if sizes is None else []),
                         *([] if s == 1 else [s]), **kw)
        if device:
            e.signal_stream(ts)
            flat.record_stream(torch.cuda.current_stream(flat.device))
        else:
            e.synchronize()
        return out, res

    def _with_frames(self, stack, work, decimate: int = 1):
        """:meth:`_transfer` of a stack: ``(out stack in the input's container,
        work's result)``."""
        is_tensor = isinstance(stack, torch.Tensor)
        on_gpu = is_tensor and stack.device.type == "cuda"
        self._check_samples(stack)
        src = stack.contiguous() if on_gpu else _host_samples(stack, self.depth)
        out, res = self._transfer(src.reshape(-1), self._check_stack(src.shape), work, None, decimate)
        out = out.reshape((int(src.shape[0]),) + decimated_shape(src.shape[1:], decimate))
        return (torch.from_numpy(out) if is_tensor and not on_gpu else out), res

    _check_samples = Engine._check_samples

    def _refuse_depth16(self, what: str) -> None:
        if self.depth == 16:
            raise ValueError(f"{what}: depth 16 not supported")

    def run_numpy(self, stack: np.ndarray, reps: int, decimate: int = 1) -> np.ndarray:
        """``decimate=s``: every image comes back as ``numpy_decimate(result,
        s)`` — ONE decimation launch for the whole stack."""
        s = check_decimate(decimate)
        return self._with_frames(np.asarray(stack), lambda n: self._eng.run(int(reps), n), s)[0]

    def run_tensor(self, stack: torch.Tensor, reps: int, decimate: int = 1) -> torch.Tensor:
        s = check_decimate(decimate)
        return self._with_frames(stack, lambda n: self._eng.run(int(reps), n), s)[0]

    def __call__(self, stack, reps: int, decimate: int = 1):
        if isinstance(stack, torch.Tensor):
            return self.run_tensor(stack, reps, decimate)
        return self.run_numpy(stack, reps, decimate)

    # ---- fixed points ------------------------------------------------
    def _residual(self, images, bracket) -> np.ndarray:
        self._refuse_depth16("residual")
        if images is None:
            res = self._eng.residual(self._n) if self._n else []
        else:
            res = bracket(images, self._eng.residual)[1] or []
        return np.asarray(res, dtype=np.int64).reshape(-1)

    def _until_stable(self, images, bracket, max_reps, check_every, compact):
        self._refuse_depth16("run_until_stable")
        max_reps, k = _check_stable_args(max_reps, check_every)
        if k is None:
            k = _GPU_CHECK_LAUNCHES * self.fuse
        out, st = bracket(images, lambda n: self._eng.run_until_stable(max_reps, k, n, bool(compact)))
        return out, [_stable_info(s) for s in (st or [])]

    def residual(self, stack=None) -> np.ndarray:
        """Per image, the bytes one more repetition would change, ``(n,)``
        int64 from one launch: of the images of ``stack``, or (``None``) of the
        frames the engine holds after its last call, for that call's ``n``."""
        return self._residual(stack, self._with_frames)

    def run_until_stable(self, stack, max_reps: int, check_every: Optional[int] = None, compact: bool = False):
        """All images of ``stack`` in chunks of ``check_every`` repetitions
        (default 16 x fuse) with a per-image residual check after each, until
        every image is at its fixed point or at ``max_reps``.  Returns ``(out,
        [StableInfo] * n)``: ``out[b]`` and entry b are what a single-image run
        of image b returns (an image that converged at an earlier check than
        the rest went on rewriting the same bytes).

        ``compact``: an image found fixed at a check is retired from the
        launches that follow the chunk already in flight; the return values are
        identical, ``stats.image_launches`` shows the work saved.  Retired
        launches run the latency model's tile (no first-use tuning)."""
        return self._until_stable(stack, self._with_frames, max_reps, check_every, compact)

    # ---- mixed sizes ---------------------------------------------------
    def _check_images(self, images):
        """The images as a list and their (width, height) list."""
        seq = list(images)
        if len(seq) > self.capacity:
            raise ValueError(f"{len(seq)} images exceed the engine's capacity {self.capacity}")
        sizes = []
        for im in seq:
            w, h, ch = image_geometry(tuple(im.shape))
            if ch != self.channels or not (1 <= w <= self.width and 1 <= h <= self.height):
                raise ValueError(f"image of shape {tuple(im.shape)} does not lie within the engine's "
                                 f"{self.width}x{self.height} {self.channels} envelope")
            sizes.append((w, h))
        return seq, sizes

    def _with_images(self, images, work, decimate: int = 1):
        """:meth:`_transfer` of a sequence of images of any sizes within the
        envelope, each top-left in its frame: ``([out], work's result)``, every
        output in its input's container."""
        seq, sizes = self._check_images(images)
        tensors = [isinstance(im, torch.Tensor) for im in seq]
        on_gpu = bool(seq) and all(tensors) and all(im.device.type == "cuda" for im in seq)
        for im in seq:
            self._check_samples(im)
        if on_gpu:
            flat = torch.cat([im.contiguous().reshape(-1) for im in seq])
        else:
            flat = np.concatenate([_host_samples(im, self.depth).reshape(-1) for im in seq]
                                  or [np.empty(0, _NP_DTYPE[self.depth])])
        out, res = self._transfer(flat, len(seq), work, sizes, decimate)
        outs, at = [], 0
        for im, t in zip(seq, tensors):
            shape = decimated_shape(tuple(im.shape), decimate)
            k = int(np.prod(shape))
            piece = out[at:at + k].reshape(shape)
            at += k
            if not on_gpu:
                piece = torch.from_numpy(piece.copy()) if t else piece.copy()
            outs.append(piece)
        return outs, res

    def run_images(self, images, reps: int, decimate: int = 1) -> list:
        """``reps`` repetitions of every image of the sequence, each as a lone
        image of its own size; a list in input order, in the input's container
        type (CUDA tensors stay on the device).  ``decimate=s``: entry b is
        ``numpy_decimate`` of image b's result, all from one launch."""
        s = check_decimate(decimate)
        return self._with_images(images, lambda n: self._eng.run(int(reps), n), s)[0]

    # ---- unsharp mask --------------------------------------------------
    def _unsharp_work(self, reps, amount, threshold):
        """The work between a call's upload and download: one copy launch keeps
        all originals on the device, the repetitions, one unsharp launch."""
        k = check_unsharp_amount(amount)
        t = check_unsharp_threshold(threshold, self.depth)
        if int(reps) < 0:
            raise ValueError("reps must be >= 0")
        e = self._eng

        def work(n):
            e.snapshot_original(n)
            e.run(int(reps), n)
            e.apply_unsharp(k, t, n)

        return work

    def unsharp(self, stack, reps: int, amount=1.0, threshold=0):
        """:meth:`Engine.unsharp` of every image of a stack: entry b equals
        ``numpy_unsharp(stack[b], reps, amount, threshold, ...)``.  One upload,
        ONE copy launch for all originals, the fused launches of ``__call__``,
        ONE unsharp launch, one download."""
        work = self._unsharp_work(reps, amount, threshold)
        return self._with_frames(stack if isinstance(stack, torch.Tensor) else np.asarray(stack), work)[0]

    def unsharp_images(self, images, reps: int, amount=1.0, threshold=0) -> list:
        """:meth:`unsharp` for a sequence of images of any sizes within the
        envelope (:meth:`run_images`' inputs): the unsharp launch reads the
        upload's extents table, so every image is sharpened as a lone one."""
        return self._with_images(images, self._unsharp_work(reps, amount, threshold))[0]

    def residual_images(self, images=None) -> np.ndarray:
        """:meth:`residual` for mixed sizes: of ``images``, or (``None``) of the
        frames the engine holds after its last mixed-size call."""
        return self._residual(images, self._with_images)

    def run_images_until_stable(self, images, max_reps: int, check_every: Optional[int] = None,
                                compact: bool = False):
        """:meth:`run_until_stable` for mixed sizes: ``([out], [StableInfo])``,
        entry b what a single-image run of image b returns (``compact`` as
        there: same return values, converged images leave the launches)."""
        return self._until_stable(images, self._with_images, max_reps, check_every, compact)


# convolve_batch's own engine cache (the single-image engines keep theirs).
_BATCH_ENGINES: "OrderedDict[tuple, BatchEngine]" = OrderedDict()
_MAX_CACHED_BATCH = 2
# Memory policy of batch_size=None, not a tuned number: the two ping-pong
# allocations of a BatchEngine together stay within this many bytes.
_BATCH_BYTES = 1 << 30


def _cached_batch_engine(w, h, ch, capacity, flt, device, fuse, variant, border, depth=8) -> BatchEngine:
    key = (w, h, ch, capacity, flt.taps, flt.divisor, device, fuse, variant, border, depth)
    eng = _BATCH_ENGINES.get(key)
    if eng is None:
        # make room first: two engines of the memory bound are the cache's most
        while len(_BATCH_ENGINES) >= _MAX_CACHED_BATCH:
            _BATCH_ENGINES.popitem(last=False)
        eng = BatchEngine(w, h, ch, capacity, flt, device=device, fuse=fuse, variant=variant, border=border,
                          depth=depth)
        _BATCH_ENGINES[key] = eng
    else:
        _BATCH_ENGINES.move_to_end(key)
    return eng


def _frame_bytes(w: int, h: int, ch: str, fuse: int, depth: int = 8) -> int:
    """Bytes of one device frame (csrc/include/pconv/image.hpp, FrameLayout):
    16 pad bytes, the row, at least 32 more, rounded to 128; ``fuse`` ghost
    rows above and below."""
    row_bytes = w * _CH_COUNT[ch] * (depth // 8)
    pitch = -(-(16 + -(-row_bytes // 16) * 16 + 32) // 128) * 128
    return pitch * (h + 2 * fuse)


def _as_stack(images):
    """``images`` as one uint8 (or uint16: depth 16) stack ``(N, H, W[, C])``;
    (stack, is_tensor)."""
    if isinstance(images, torch.Tensor):
        if images.dtype not in (torch.uint8, torch.uint16):
            raise TypeError("image tensor must be uint8")
        return images, True
    if isinstance(images, np.ndarray):
        if images.dtype not in (np.uint8, np.uint16):
            raise TypeError("image array must be uint8")
        return images, False
    seq = list(images)
    if not seq:
        raise ValueError("an empty sequence of images has no geometry: pass an array or tensor of shape (0, H, W[, C])")
    shapes = {tuple(im.shape) for im in seq}
    if len(shapes) != 1:
        raise ValueError(f"images of a batch must have one shape, got {sorted(shapes)}")
    if all(isinstance(im, torch.Tensor) for im in seq):
        if any(im.dtype != seq[0].dtype or im.dtype not in (torch.uint8, torch.uint16) for im in seq):
            raise TypeError("image tensor must be uint8")
        return torch.stack(seq), True
    arrs = [im.cpu().numpy() if isinstance(im, torch.Tensor) else np.asarray(im) for im in seq]
    if any(a.dtype != arrs[0].dtype or a.dtype not in (np.uint8, np.uint16) for a in arrs):
        raise TypeError("image array must be uint8")
    return np.stack(arrs), False


def _prepare_batch(images, filter, backend, border, batch_size):
    """The argument checks the batch entry points share: (filter, stack,
    is_tensor, (width, height, channels), resolved backend)."""
    if batch_size is not None and int(batch_size) < 1:
        raise ValueError("batch_size must be >= 1")
    flt = get_filter(filter)
    check_border(border)
    stack, is_tensor = _as_stack(images)
    shape = tuple(int(s) for s in stack.shape)
    if len(shape) not in (3, 4):
        raise ValueError(f"unsupported batch shape {shape}: expected (N, H, W) or (N, H, W, 1|3|4)")
    geo = image_geometry(shape[1:])
    if backend == "auto":
        backend = "hip" if (is_tensor and stack.is_cuda) else _default_backend()
    if backend not in ("hip", "omp", "cpu", "numpy"):
        raise ValueError(f"unknown backend {backend!r} (hip|omp|cpu|numpy|auto)")
    return flt, stack, is_tensor, geo, backend


def _empty_like_stack(stack, is_tensor):
    return torch.empty_like(stack) if is_tensor else np.empty(tuple(stack.shape), dtype=stack.dtype)


def _hip_batch_engine(stack, is_tensor, geo, flt, device, fuse, variant, border, batch_size):
    """The cached BatchEngine for a stack and its capacity (the chunk size)."""
    n = require_native()
    w, h, ch = geo
    n_img = int(stack.shape[0])
    if device is None:
        device = stack.device.index if (is_tensor and stack.is_cuda) else 0
    device = int(device or 0)
    depth = _check_depth(image_depth(stack), flt, variant)
    if fuse is None:
        c = _CH_COUNT[ch]
        fuse = n.auto_fuse(flt.to_native(), variant, w * h * c * (depth // 8), c, depth=depth)
    fuse = int(fuse)
    if batch_size is None:
        cap = max(1, min(n_img, _BATCH_BYTES // (2 * _frame_bytes(w, h, ch, fuse, depth))))
    else:
        cap = min(n_img, int(batch_size))
    return _cached_batch_engine(w, h, ch, cap, flt, device, fuse, variant, border, depth), cap


def convolve_batch(images, reps: int = 1, filter="gaussian", backend: str = "auto", device: Optional[int] = None,
                   fuse: Optional[int] = None, variant: str = "auto", threads: int = 0, border: str = "zero",
                   batch_size: Optional[int] = None, decimate: int = 1):
    """``convolve`` for N same-size 8-bit images at once.

    ``images``: an ``(N, H, W)`` array or tensor (grey), an ``(N, H, W, C)``
    one with ``C`` in {1, 3, 4}, or a sequence of N same-shape images (stacked).
    The result equals ``np.stack([convolve(img, reps, ...) for img in images])``
    on every backend, in the input's container type and on its device (a
    sequence returns a stack).

    On the ``hip`` backend the images advance together through one cached
    :class:`BatchEngine`, ``batch_size`` at a time (the last chunk shorter).
    ``batch_size=None``: the largest n <= N whose two device allocations stay
    within 1 GiB (at least 1) — a memory policy, not a tuned number.  The
    other backends loop over the images.  ``decimate=s``: every image of the
    result is decimated as by :func:`convolve` (``hip``: one decimation launch
    per chunk).
    """
    if reps < 0:
        raise ValueError("reps must be >= 0")
    s = check_decimate(decimate)
    flt, stack, is_tensor, geo, backend = _prepare_batch(images, filter, backend, border, batch_size)
    _check_depth(image_depth(stack), flt, variant if backend == "hip" else "auto")
    n_img = int(stack.shape[0])
    if n_img == 0:
        empty = _empty_like_stack(stack, is_tensor)
        return empty if s == 1 else empty[:, ::s, ::s]

    if backend != "hip":
        outs = [convolve(stack[i], reps, flt, backend=backend, threads=threads, border=border, decimate=s)
                for i in range(n_img)]
        return torch.stack(outs) if is_tensor else np.stack(outs)

    eng, cap = _hip_batch_engine(stack, is_tensor, geo, flt, device, fuse, variant, border, batch_size)
    if n_img <= cap:
        return eng(stack, reps, s)
    outs = [eng(stack[i:i + cap], reps, s) for i in range(0, n_img, cap)]
    return torch.cat(outs) if is_tensor else np.concatenate(outs)


def unsharp_batch(images, reps: int = 1, amount=1.0, threshold=0, filter="gaussian", backend: str = "auto",
                  device: Optional[int] = None, fuse: Optional[int] = None, variant: str = "auto", threads: int = 0,
                  border: str = "zero", batch_size: Optional[int] = None, decimate: int = 1):
    """:func:`unsharp` for N same-size images at once (:func:`convolve_batch`'s
    inputs, engine cache, chunking and ``batch_size``): the result equals
    ``np.stack([unsharp(img, reps, amount, threshold, ...) for img in
    images])`` on every backend.  ``hip``: per chunk one copy launch for the
    originals and one unsharp launch beside the fused launches; the other
    backends loop over the images."""
    if reps < 0:
        raise ValueError("reps must be >= 0")
    _refuse_unsharp_decimate(decimate)
    flt, stack, is_tensor, geo, backend = _prepare_batch(images, filter, backend, border, batch_size)
    depth = image_depth(stack)
    check_unsharp_amount(amount)
    t = check_unsharp_threshold(threshold, depth)
    _check_depth(depth, flt, variant if backend == "hip" else "auto")
    n_img = int(stack.shape[0])
    if n_img == 0:
        return _empty_like_stack(stack, is_tensor)

    if backend != "hip":
        outs = [unsharp(stack[i], reps, amount, t, flt, backend=backend, threads=threads, border=border)
                for i in range(n_img)]
        return torch.stack(outs) if is_tensor else np.stack(outs)

    eng, cap = _hip_batch_engine(stack, is_tensor, geo, flt, device, fuse, variant, border, batch_size)
    if n_img <= cap:
        return eng.unsharp(stack, reps, amount, t)
    outs = [eng.unsharp(stack[i:i + cap], reps, amount, t) for i in range(0, n_img, cap)]
    return torch.cat(outs) if is_tensor else np.concatenate(outs)


def convolve_batch_until_stable(images, max_reps: int, filter="gaussian", check_every: Optional[int] = None,
                                backend: str = "auto", device: Optional[int] = None, fuse: Optional[int] = None,
                                variant: str = "auto", threads: int = 0, border: str = "zero",
                                batch_size: Optional[int] = None, compact: bool = False, unsharp=None):
    """``convolve_until_stable`` for N same-size 8-bit images at once.

    Inputs, backends, the engine cache and ``batch_size`` are
    :func:`convolve_batch`'s.  Returns ``(stack, [StableInfo] * N)`` where, on
    every backend and for every b, ``stack[b]`` and entry b equal what
    ``convolve_until_stable(images[b], max_reps, filter, check_every, ...)``
    returns.  On the ``hip`` backend the images of a chunk advance together and
    every check counts all of them in one launch of the residual kernel; a
    chunk's loop ends when its last image has converged (the others rewrite
    their fixed point's bytes meanwhile) or at ``max_reps``.  The other
    backends loop over the images.

    ``compact`` (``hip`` backend): images found fixed are retired from the
    launches after the chunk in flight (:meth:`BatchEngine.run_until_stable`).
    The ``cpu`` and ``numpy`` backends accept and ignore it: they loop per
    image and already stop each image at its own fixed point.  The return
    values are identical for both settings on every backend.
    """
    refuse_unsharp("convolve_batch_until_stable", unsharp)
    _check_stable_args(max_reps, check_every)
    flt, stack, is_tensor, geo, backend = _prepare_batch(images, filter, backend, border, batch_size)
    _refuse_depth16(stack, "convolve_batch_until_stable")
    n_img = int(stack.shape[0])
    if n_img == 0:
        return _empty_like_stack(stack, is_tensor), []

    if backend != "hip":
        res = [convolve_until_stable(stack[i], max_reps, flt, check_every=check_every, backend=backend,
                                     threads=threads, border=border) for i in range(n_img)]
        outs = [r[0] for r in res]
        return (torch.stack(outs) if is_tensor else np.stack(outs)), [r[1] for r in res]

    eng, cap = _hip_batch_engine(stack, is_tensor, geo, flt, device, fuse, variant, border, batch_size)
    if n_img <= cap:
        return eng.run_until_stable(stack, int(max_reps), check_every, compact)
    res = [eng.run_until_stable(stack[i:i + cap], int(max_reps), check_every, compact)
           for i in range(0, n_img, cap)]
    outs = [r[0] for r in res]
    return (torch.cat(outs) if is_tensor else np.concatenate(outs)), [info for r in res for info in r[1]]


def residual_batch(images, filter="gaussian", backend: str = "auto", device: Optional[int] = None, threads: int = 0,
                   border: str = "zero") -> np.ndarray:
    """:func:`residual` of N same-size images, ``(N,)`` int64: equals
    ``[residual(img, ...) for img in images]``; on the ``hip`` backend one
    launch of the residual kernel per chunk of the batch engine."""
    flt, stack, is_tensor, geo, backend = _prepare_batch(images, filter, backend, border, None)
    _refuse_depth16(stack, "residual_batch")
    n_img = int(stack.shape[0])
    if n_img == 0:
        return np.zeros((0,), dtype=np.int64)
    if backend != "hip":
        return np.asarray([residual(stack[i], flt, backend=backend, threads=threads, border=border)
                           for i in range(n_img)], dtype=np.int64)
    eng, cap = _hip_batch_engine(stack, is_tensor, geo, flt, device, None, "auto", border, None)
    return np.concatenate([eng.residual(stack[i:i + cap]) for i in range(0, n_img, cap)])


# ---- images of different sizes ------------------------------------------------

def size_buckets(sizes, channels, fuse, min_fill: float = 0.5, batch_size: Optional[int] = None,
                 max_bytes: int = _BATCH_BYTES, depth: int = 8):
    """Group images of different sizes into envelopes for :class:`BatchEngine`.

    ``sizes``: ``[(width, height)]``; ``channels``: ``"grey" | "rgb" | "rgba"``
    or the count; ``fuse``: the ghost rows of a frame, an int or a callable
    ``(width, height) -> int`` asked with a bucket's envelope.  Returns
    ``[((W, H), [indices])]``: every index once, ``(W, H)`` the members' maximum
    width and maximum height.

    Pure Python and deterministic: the indices are sorted by (height, width)
    descending (stable) and buckets are filled greedily — an image joins the
    open bucket while its fill ``sum(w_i * h_i) / (n * W * H)`` stays
    ``>= min_fill``, ``n <= batch_size`` and the engine's two allocations,
    ``2 * n * frame bytes of the envelope``, stay within ``max_bytes``; a
    bucket always takes at least one image.

    ``min_fill = 0.5`` is a waste policy (at most half of a bucket's tile work
    and frame memory goes to area outside its images), like the 1 GiB of
    ``max_bytes``: neither is a tuned number.  ``depth``: bits per sample
    (8 | 16) of the frames the bytes are counted for.
    """
    ch = _CHANNELS[channels] if channels in _CHANNELS else channels
    if ch not in _CH_COUNT:
        raise ValueError(f"unknown channels {channels!r}")
    if not 0.0 <= float(min_fill) <= 1.0:
        raise ValueError("min_fill must lie in [0, 1]")
    if batch_size is not None and int(batch_size) < 1:
        raise ValueError("batch_size must be >= 1")
    sizes = [(int(w), int(h)) for w, h in sizes]
    if any(w < 1 or h < 1 for w, h in sizes):
        raise ValueError("image sizes must be >= 1x1")
    fuse_of = fuse if callable(fuse) else (lambda w, h: int(fuse))
    order = sorted(range(len(sizes)), key=lambda i: (-sizes[i][1], -sizes[i][0]))
    buckets = []
    members, env, area = [], (0, 0), 0
    for i in order:
        w, h = sizes[i]
        if members:
            n = len(members) + 1
            e = (max(env[0], w), max(env[1], h))
            fits = ((area + w * h) >= float(min_fill) * n * e[0] * e[1]
                    and (batch_size is None or n <= int(batch_size))
                    and 2 * n * _frame_bytes(e[0], e[1], ch, fuse_of(*e), depth) <= max_bytes)
            if fits:
                members.append(i)
                env, area = e, area + w * h
                continue
            buckets.append((env, members))
        members, env, area = [i], (w, h), w * h
    if members:
        buckets.append((env, members))
    return buckets


def _prepare_many(images, filter, backend, border, batch_size, min_fill):
    """The argument checks the mixed-size entry points share: (filter, images
    as a list, is_tensor, channels name, resolved backend)."""
    if batch_size is not None and int(batch_size) < 1:
        raise ValueError("batch_size must be >= 1")
    if not 0.0 <= float(min_fill) <= 1.0:
        raise ValueError("min_fill must lie in [0, 1]")
    flt = get_filter(filter)
    check_border(border)
    if isinstance(images, (np.ndarray, torch.Tensor)):
        raise TypeError("images must be a sequence of images (a stack of same-size images goes to convolve_batch)")
    seq = list(images)
    if backend not in ("auto", "hip", "omp", "cpu", "numpy"):
        raise ValueError(f"unknown backend {backend!r} (hip|omp|cpu|numpy|auto)")
    if not seq:
        return flt, seq, False, None, backend
    kinds = {isinstance(im, torch.Tensor) for im in seq}
    if len(kinds) != 1 or not all(isinstance(im, (torch.Tensor, np.ndarray)) for im in seq):
        raise TypeError("images must be all NumPy arrays or all torch tensors")
    is_tensor = kinds.pop()
    ok = (torch.uint8, torch.uint16) if is_tensor else (np.uint8, np.uint16)
    if any(im.dtype != seq[0].dtype or im.dtype not in ok for im in seq):
        raise TypeError("image tensor must be uint8" if is_tensor else "image array must be uint8")
    chans = {image_geometry(tuple(im.shape))[2] for im in seq}
    if len(chans) != 1:
        raise ValueError(f"images must share one channel count, got {sorted(chans)}")
    if any(int(s) < 1 for im in seq for s in im.shape):
        raise ValueError("images must be at least 1x1")
    if is_tensor and len({im.device for im in seq}) != 1:
        raise ValueError("image tensors must share one device")
    if backend == "auto":
        backend = "hip" if (is_tensor and seq[0].is_cuda) else _default_backend()
    return flt, seq, is_tensor, chans.pop(), backend


def _hip_buckets(seq, is_tensor, ch, flt, device, fuse, variant, border, batch_size, min_fill):
    """(cached BatchEngine, indices) per size bucket of the images."""
    n = require_native()
    if device is None:
        device = seq[0].device.index if (is_tensor and seq[0].is_cuda) else 0
    device = int(device or 0)
    c = _CH_COUNT[ch]
    nf = flt.to_native()
    depth = _check_depth(image_depth(seq[0]), flt, variant)
    fuse_of = ((lambda w, h: int(n.auto_fuse(nf, variant, w * h * c * (depth // 8), c, depth=depth)))
               if fuse is None else (lambda w, h: int(fuse)))
    sizes = [image_geometry(tuple(im.shape))[:2] for im in seq]
    for (w, h), idx in size_buckets(sizes, ch, fuse_of, min_fill, batch_size, depth=depth):
        yield _cached_batch_engine(w, h, ch, len(idx), flt, device, fuse_of(w, h), variant, border, depth), idx


def convolve_many(images, reps: int = 1, filter="gaussian", backend: str = "auto", device: Optional[int] = None,
                  fuse: Optional[int] = None, variant: str = "auto", threads: int = 0, border: str = "zero",
                  batch_size: Optional[int] = None, min_fill: float = 0.5, decimate: int = 1) -> list:
    """``convolve`` for a sequence of 8-bit images of ANY sizes.

    ``images``: uint8 ``(H, W)`` / ``(H, W, C)`` arrays or tensors that share
    one channel count and one container kind (tensors one device).  Entry i of
    the returned list equals ``convolve(images[i], reps, ...)``, in the input's
    container and on its device; ``[]`` gives ``[]``.

    On the ``hip`` backend the images are grouped by :func:`size_buckets`
    (``min_fill``, ``batch_size``, 1 GiB of frames) and every bucket advances
    in the fused launches of one cached :class:`BatchEngine` whose geometry is
    the bucket's envelope: ``ceil(reps / fuse)`` launches per bucket whatever
    its images' number and sizes.  The other backends loop over the images.
    ``decimate=s``: entry i is decimated as by :func:`convolve` (``hip``: one
    decimation launch per bucket).
    """
    if reps < 0:
        raise ValueError("reps must be >= 0")
    s = check_decimate(decimate)
    flt, seq, is_tensor, ch, backend = _prepare_many(images, filter, backend, border, batch_size, min_fill)
    if not seq:
        return []
    _check_depth(image_depth(seq[0]), flt, variant if backend == "hip" else "auto")
    if backend != "hip":
        return [convolve(im, reps, flt, backend=backend, threads=threads, border=border, decimate=s) for im in seq]
    outs = [None] * len(seq)
    for eng, idx in _hip_buckets(seq, is_tensor, ch, flt, device, fuse, variant, border, batch_size, min_fill):
        for i, o in zip(idx, eng.run_images([seq[i] for i in idx], reps, s)):
            outs[i] = o
    return outs


def unsharp_many(images, reps: int = 1, amount=1.0, threshold=0, filter="gaussian", backend: str = "auto",
                 device: Optional[int] = None, fuse: Optional[int] = None, variant: str = "auto", threads: int = 0,
                 border: str = "zero", batch_size: Optional[int] = None, min_fill: float = 0.5,
                 decimate: int = 1) -> list:
    """:func:`unsharp` for a sequence of images of ANY sizes
    (:func:`convolve_many`'s inputs and size buckets): entry i equals
    ``unsharp(images[i], reps, amount, threshold, ...)``; ``[]`` gives ``[]``.
    ``hip``: per bucket one copy launch for the originals and one unsharp
    launch, which reads the bucket's extents table."""
    if reps < 0:
        raise ValueError("reps must be >= 0")
    _refuse_unsharp_decimate(decimate)
    flt, seq, is_tensor, ch, backend = _prepare_many(images, filter, backend, border, batch_size, min_fill)
    check_unsharp_amount(amount)
    if not seq:
        check_unsharp_threshold(threshold, 16)
        return []
    depth = image_depth(seq[0])
    t = check_unsharp_threshold(threshold, depth)
    _check_depth(depth, flt, variant if backend == "hip" else "auto")
    if backend != "hip":
        return [unsharp(im, reps, amount, t, flt, backend=backend, threads=threads, border=border) for im in seq]
    outs = [None] * len(seq)
    for eng, idx in _hip_buckets(seq, is_tensor, ch, flt, device, fuse, variant, border, batch_size, min_fill):
        for i, o in zip(idx, eng.unsharp_images([seq[i] for i in idx], reps, amount, t)):
            outs[i] = o
    return outs


def convolve_many_until_stable(images, max_reps: int, filter="gaussian", check_every: Optional[int] = None,
                               backend: str = "auto", device: Optional[int] = None, fuse: Optional[int] = None,
                               variant: str = "auto", threads: int = 0, border: str = "zero",
                               batch_size: Optional[int] = None, min_fill: float = 0.5, compact: bool = False,
                               unsharp=None):
    """``convolve_until_stable`` for a sequence of images of any sizes
    (:func:`convolve_many`'s inputs and buckets).  Returns ``([out],
    [StableInfo])``: entry i of both is what ``convolve_until_stable(images[i],
    max_reps, filter, check_every, ...)`` returns.  On the ``hip`` backend every
    check counts a bucket's images in one launch of the residual kernel.
    ``compact`` is :func:`convolve_batch_until_stable`'s, per bucket: same
    return values; the ``cpu`` and ``numpy`` backends accept and ignore it
    (they already stop each image at its own fixed point)."""
    refuse_unsharp("convolve_many_until_stable", unsharp)
    _check_stable_args(max_reps, check_every)
    flt, seq, is_tensor, ch, backend = _prepare_many(images, filter, backend, border, batch_size, min_fill)
    if not seq:
        return [], []
    _refuse_depth16(seq[0], "convolve_many_until_stable")
    if backend != "hip":
        res = [convolve_until_stable(im, max_reps, flt, check_every=check_every, backend=backend, threads=threads,
                                     border=border) for im in seq]
        return [r[0] for r in res], [r[1] for r in res]
    outs, infos = [None] * len(seq), [None] * len(seq)
    for eng, idx in _hip_buckets(seq, is_tensor, ch, flt, device, fuse, variant, border, batch_size, min_fill):
        got, st = eng.run_images_until_stable([seq[i] for i in idx], int(max_reps), check_every, compact)
        for i, o, info in zip(idx, got, st):
            outs[i], infos[i] = o, info
    return outs, infos


def residual_many(images, filter="gaussian", backend: str = "auto", device: Optional[int] = None, threads: int = 0,
                  border: str = "zero", batch_size: Optional[int] = None, min_fill: float = 0.5) -> np.ndarray:
    """:func:`residual` of a sequence of images of any sizes, ``(N,)`` int64:
    equals ``[residual(img, ...) for img in images]``; on the ``hip`` backend
    one launch of the residual kernel per size bucket."""
    flt, seq, is_tensor, ch, backend = _prepare_many(images, filter, backend, border, batch_size, min_fill)
    if not seq:
        return np.zeros((0,), dtype=np.int64)
    _refuse_depth16(seq[0], "residual_many")
    if backend != "hip":
        return np.asarray([residual(im, flt, backend=backend, threads=threads, border=border) for im in seq],
                          dtype=np.int64)
    out = np.zeros((len(seq),), dtype=np.int64)
    for eng, idx in _hip_buckets(seq, is_tensor, ch, flt, device, None, "auto", border, batch_size, min_fill):
        out[idx] = eng.residual_images([seq[i] for i in idx])
    return out


def convolve_file(path: str, width: int, height: int, reps: int, channels: str = "grey", filter="gaussian",
                  out: Optional[str] = None, backend: str = "auto", device: Optional[int] = None,
                  border: str = "zero", depth: int = 8, decimate: int = 1, unsharp=None,
                  unsharp_threshold=0) -> str:
    """The reference program in one call (``cuda/main.c:10-53``): read the raw
    image, ``reps`` repetitions, write ``blur_<name>`` (or ``out``); returns the
    output path.  ``decimate=s``: the file holds the decimated result,
    ``ceil(height / s) x ceil(width / s)`` pixels.  ``unsharp=amount`` (with
    ``unsharp_threshold``): the file holds :func:`unsharp` of the image
    instead of its blur (not together with ``decimate`` above 1)."""
    from ..utils.raw_io import output_path_for, read_raw, write_raw

    if unsharp is None and unsharp_threshold not in (0, None):
        raise ValueError("unsharp_threshold needs unsharp (an amount)")
    img = read_raw(path, width, height, channels, depth=depth)
    if unsharp is not None:
        res = _unsharp(img, reps, unsharp, unsharp_threshold, filter, backend=backend, device=device, border=border,
                       decimate=check_decimate(decimate))
    else:
        res = convolve(img, reps, filter, backend=backend, device=device, border=border, decimate=decimate)
    dst = out or output_path_for(path)
    write_raw(dst, res)
    return dst
