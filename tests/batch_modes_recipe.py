"""One BatchEngine taken through its modes in a row — mixed sizes, a plain
stack, mixed sizes again, every run compacting — for test_gpu_batch_compact.py
(the engine) and test_batch_compact_cpu.py (the recipe itself, without a GPU).

Envelope 67 x 33, capacity 4, gaussian, fuse 2: 67 RGB pixels are 201 bytes, no
whole dwords, while the 64-pixel image's rows are; 33 rows straddle the residual
kernel's 32-row workgroup.  Every step holds an image that is at its fixed
point by the first check (a single pixel, a constant image) and noise that is
still moving at MAX_REPS, so each step retires work (``retires`` says so from
the oracle's results alone).  The oracle is the per-image ``convolve_until_stable(..., backend="cpu")``."""
import numpy as np

from batch_compact_formula import chunk_launches, converged_at

W, H, CAPACITY, FUSE, FILTER = 67, 33, 4, 2, "gaussian"
MAX_REPS, CHECK_EVERY = 48, 4
CHANNELS = [1, 3]

_STEPS = {}
_ORACLE = {}


def _noise(rng, w, h, c):
    return rng.integers(0, 256, size=(h, w, c) if c > 1 else (h, w), dtype=np.uint8)


def steps(c, border):
    """[("images" | "stack", [image])]: what the engine is given, in order."""
    key = (c, border)
    if key not in _STEPS:
        rng = np.random.default_rng(6733 + c)
        # a constant image is a fixed point under the replicate border, zeros under both
        flat = 200 if border == "replicate" else 0
        first = [_noise(rng, w, h, c) for w, h in [(67, 33), (5, 31), (64, 32), (1, 1)]]
        stack = [_noise(rng, W, H, c), np.full_like(first[0], flat), _noise(rng, W, H, c)]
        last = [_noise(rng, w, h, c) for w, h in [(4, 3), (66, 17), (67, 2)]]
        last[0][...] = flat
        _STEPS[key] = [("images", first), ("stack", stack), ("images", last)]
        for _, imgs in _STEPS[key]:
            for im in imgs:
                im.setflags(write=False)
    return _STEPS[key]


def oracle(pconv_mod, c, border):
    """Per step ([out_b], [StableInfo_b]) of the single-image CPU runs, computed once."""
    key = (c, border)
    if key not in _ORACLE:
        _ORACLE[key] = []
        for _, imgs in steps(c, border):
            res = [pconv_mod.convolve_until_stable(im, MAX_REPS, FILTER, check_every=CHECK_EVERY, backend="cpu",
                                                   border=border) for im in imgs]
            _ORACLE[key].append(([r[0] for r in res], [r[1] for r in res]))
    return _ORACLE[key]


def retires(infos):
    """Whether a compacting loop with these results launches without some
    image: one converged at a check that two more chunks follow (the first of
    them is in flight with it)."""
    chunks = len(chunk_launches(MAX_REPS, CHECK_EVERY, FUSE, converged_at(infos)))
    return any(i.converged and i.checks + 1 < chunks for i in infos)
