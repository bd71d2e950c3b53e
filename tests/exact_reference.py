"""Exact integer reference of the gaussian, independent of both oracles the
package ships: it shares no code with ``pconv.numpy_convolve`` (the float32
formula) or with ``cpu_fused_launch`` (the native twin of a fused launch)."""
import numpy as np

WEIGHTS = ((1, 2, 1), (2, 4, 2), (1, 2, 1))  # sum 16


def exact_gaussian(img, steps, border):
    """``steps`` repetitions of out = (sum w p) >> 4 per channel in int64;
    ``border`` "zero" pads with zeros, "replicate" with the edge samples.
    ``img`` is (H, W) or (H, W, C), uint8 or uint16; the result has its dtype."""
    if img.dtype not in (np.uint8, np.uint16):
        raise TypeError(f"exact_gaussian: uint8 or uint16, not {img.dtype}")
    if border not in ("zero", "replicate"):
        raise ValueError(f"exact_gaussian: unknown border {border!r}")
    cur = img.astype(np.int64)
    cur = cur[:, :, None] if img.ndim == 2 else cur
    h, w, _ = cur.shape
    for _ in range(int(steps)):
        p = np.pad(cur, ((1, 1), (1, 1), (0, 0)), mode="edge" if border == "replicate" else "constant")
        s = np.zeros_like(cur)
        for dy in range(3):
            for dx in range(3):
                s += WEIGHTS[dy][dx] * p[dy:dy + h, dx:dx + w]
        cur = s >> 4  # the weights sum to 16: never above the input's maximum
    return cur.reshape(img.shape).astype(img.dtype)


def adversarial(rng, h, n, c, dtype):
    """(h, n) samples of `dtype` (n = width x c): uniform random over the full
    range with a block of the maximum, a 0 / max checkerboard and alternating
    0 / max column groups of `c` samples planted in it.  The 8-bit paired step
    form fills its 16-bit fields up to 65280 only at such values."""
    top = int(np.iinfo(dtype).max)
    a = rng.integers(0, top + 1, size=(h, n), dtype=dtype)
    yy, xx = np.mgrid[0:h, 0:n]
    r, q = h // 5, n // 7
    a[r:r + 4, q:q + 9] = top
    cb = (((yy + xx) & 1) * top).astype(dtype)
    r = h // 2
    a[r:r + 3, :max(1, n // 2)] = cb[r:r + 3, :max(1, n // 2)]
    cg = ((((xx // c) & 1) ^ 1) * top).astype(dtype)
    r = (3 * h) // 4
    a[r:r + 3, n // 3:] = cg[r:r + 3, n // 3:]
    return a
