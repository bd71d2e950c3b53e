"""Harness of tests/test_gpu_tile_edges.py: tile geometry of the fused 8-bit
kernels, sizes derived from it, test images, dirty canary-guarded frames and
the byte-for-byte comparison of a launch's whole destination allocation.

Imports NumPy only; torch is imported inside launch()."""
import math

import numpy as np

GUARD = 4096
CANARY = 0xA5
PAD = 16  # pad bytes left of a frame row's first data byte
NAME = {1: "grey", 3: "rgb", 4: "rgba"}
CH = {"grey": 1, "rgb": 3, "rgba": 4}
BORDERS = ("zero", "replicate")
NEG_TAPS = ([3, 1, 0, 2, 5, 1, -1, 2, 4], 17)  # the negative-tap custom filter of test_gpu_kernels.py


def module_shapes(name):
    """A shape list of the native module as tuples, for parametrize ids; []
    when the extension is not there (test_shape_lists_were_read then fails)."""
    try:
        import pconv

        return [tuple(s) for s in getattr(pconv.native, name)()]
    except Exception:
        return []


def geom(lw, m, nw, c, steps):
    """(hl, vs, vrows) of a tile: halo lanes per side, valid bytes per column
    strip, valid rows per tile.  The float kernel: lw = 8."""
    hl = -(-steps * c // lw)
    return hl, (64 - 2 * hl) * lw, m * nw - 2 * steps


def runs(lw, m, nw, c, steps):
    """The only reason a (shape, steps) pair is left out."""
    _, vs, vrows = geom(lw, m, nw, c, steps)
    return vs > 0 and vrows > 0 and lw >= c


def strips(rb, vs):
    """(nstrips, pair_stride) of a row of rb bytes."""
    n = -(-rb // vs)
    return n, (n + 1) // 2


def tile_sizes(lw, m, nw, c, steps, chunk_valid=()):
    """[(h, w, small)] in pixels for the tile kernel, paired and not multiplied
    out: one pixel; small x small; thin images at the edges; each side of the
    tile edge in x with each side in y; two tiles and a rest both ways (3
    strips: the last tile has no B strip); the 4-strip width at one height;
    (c > 1) the width whose last pixel straddles two strips and a width whose
    last chunk is partial; one width per entry of chunk_valid (valid bytes of
    the row's last lw-byte chunk).  `small`: halved across border and form at
    steps >= 8."""
    _, vs, vrows = geom(lw, m, nw, c, steps)
    wpx = -(-vs // c)
    out = [(1, 1, True), (2, 2, True), (3, 1, True), (1, 2, True),
           (1, wpx + 1, True), (3, wpx, True), (vrows + 1, 1, True), (vrows - 1, 2, True),
           (vrows - 1, wpx - 1, False), (vrows - 1, wpx + 1, False), (vrows + 1, wpx - 1, False),
           (vrows + 1, wpx + 1, False), (vrows, wpx, False),
           (2 * vrows + 3, 2 * wpx + 3, False), (vrows + 1, 3 * wpx + 1, False)]
    if c > 1:
        # last pixel across two strips: row bytes rb with rb - c < k vs < rb
        out += [(vrows, k * vs // c + 1, False) for k in (1, 2) if (k * vs) % c][:1]
        out += [(2, w, True) for w in range(wpx + 2, wpx + 2 + 2 * lw) if (w * c) % lw][:1]
    for valid in chunk_valid:
        out += [(3, w, True) for w in range(1, 40) if (w * c) % lw == valid % lw][:1]
    seen, uniq = set(), []
    for h, w, small in out:
        if h >= 1 and w >= 1 and (h, w) not in seen:
            seen.add((h, w))
            uniq.append((h, w, small))
    return uniq


def bufop_sizes(m, nw, c, steps):
    """tile_sizes() for the buffer-op kernel (4-byte lanes, rows of whole
    dwords): every byte target rounded to the nearest multiple of lcm(c, 4) on
    its side of the strip edge.  [(h, w, small, two_tile)]."""
    _, vs, vrows = geom(4, m, nw, c, steps)
    q = c * 4 // math.gcd(c, 4)
    below = lambda b: (b - 1) // q * q  # noqa: E731  largest multiple of q < b
    above = lambda b: b // q * q + q    # noqa: E731  smallest multiple of q > b
    rbs = [(1, q, True), (2, 2 * q, True), (3, q, True), (1, above(vs), True), (vrows + 1, q, True),
           (vrows - 1, 2 * q, True),
           (vrows - 1, below(vs), False), (vrows - 1, above(vs), False), (vrows + 1, below(vs), False),
           (vrows + 1, above(vs), False), (2 * vrows + 3, above(2 * vs + 3 * c), False),
           (vrows + 1, above(3 * vs), False)]
    if vs % q == 0:
        rbs.append((vrows, vs, False))  # the last pixel ends the strip
    seen, out = set(), []
    for h, rb, small in rbs:
        if h >= 1 and rb >= q and (h, rb) not in seen:
            seen.add((h, rb))
            out.append((h, rb // c, small, h == 2 * vrows + 3))
    return out


# ---- images (h, rb) uint8 -----------------------------------------------------


def values8(rng, h, rb):
    """Uniform random bytes with a block of 255, a 0 / 255 checkerboard band
    and a band of 254 / 1 columns planted in them."""
    a = rng.integers(0, 256, size=(h, rb), dtype=np.uint8)
    a[h // 5:h // 5 + 4, rb // 7:rb // 7 + 9] = 255
    yy, xx = np.mgrid[0:h, 0:rb]
    cb = (((yy + xx) & 1) * 255).astype(np.uint8)
    a[h // 2:h // 2 + 3, :(rb + 1) // 2] = cb[h // 2:h // 2 + 3, :(rb + 1) // 2]
    cols = np.where(xx & 1, 1, 254).astype(np.uint8)
    a[(3 * h) // 4:(3 * h) // 4 + 2, rb // 3:] = cols[(3 * h) // 4:(3 * h) // 4 + 2, rb // 3:]
    return a


def checkerboard(h, rb):
    yy, xx = np.mgrid[0:h, 0:rb]
    return (((yy + xx) & 1) * 255).astype(np.uint8)


def strip_image(h, rb, vs, lit):
    """255 in the bytes of every column strip k = x // vs with lit(k), else 0."""
    k = np.arange(rb) // vs
    row = np.where(np.vectorize(lit, otypes=[bool])(k), 255, 0).astype(np.uint8)
    return np.repeat(row[None], h, axis=0)


def deep_zero_columns(rb, vs, c, steps, lit):
    """Byte columns of unlit strips further than `steps` pixels from both strip
    boundaries: under the zero border nothing lit reaches them."""
    x = np.arange(rb)
    k = x // vs
    unlit = ~np.vectorize(lit, otypes=[bool])(k)
    return unlit & (x - k * vs >= steps * c) & ((k + 1) * vs - 1 - x >= steps * c)


# ---- frames ---------------------------------------------------------------------


def frames(lay, halo, rows_img, top_ghosts=0, bottom_ghosts=0):
    """(clean, dirty) frames ((h + 2 halo, pitch) uint8) of rows_img ((h + 2
    halo, rb): ghost rows included).  Frame rows [0, top_ghosts) and the last
    bottom_ghosts ones lie outside the global image.  clean: zeros there and in
    every pad; dirty: 0xFF there, in the 16 left pad bytes and right of rb."""
    n, rb = rows_img.shape
    clean = np.zeros((n, lay["pitch"]), np.uint8)
    clean[:, PAD:PAD + rb] = rows_img
    clean[:top_ghosts] = 0
    clean[n - bottom_ghosts:] = 0
    dirty = clean.copy()
    dirty[:top_ghosts] = 0xFF
    dirty[n - bottom_ghosts:] = 0xFF
    dirty[:, :PAD] = 0xFF
    dirty[:, PAD + rb:] = 0xFF
    assert n == 2 * halo + lay["rows"] and dirty.size == lay["bytes"]
    return clean, dirty


def _alloc(torch, frame):
    buf = torch.full((frame.size + 2 * GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    buf[GUARD:GUARD + frame.size] = torch.from_numpy(np.ascontiguousarray(frame).reshape(-1)).cuda()
    return buf


def launch(native, dirty, lay, halo, filt, c, r0, r1, steps, g_row0, height, border, variant):
    """One launch of a (h + 2 halo, pitch) source frame into an all-canary
    destination.  Returns the destination ALLOCATION (guard bands included,
    uint8, flat); the source must come back unmodified."""
    import torch

    src = _alloc(torch, dirty)
    dst = torch.full((dirty.size + 2 * GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    base = GUARD + lay["pitch"] * halo + PAD
    rows = dirty.shape[0] - 2 * halo
    native.launch_stencil(filt, NAME[c], src.data_ptr() + base, dst.data_ptr() + base, lay["pitch"], lay["row_bytes"],
                          r0, r1, -halo, rows + halo, steps, g_row0, height,
                          torch.cuda.current_stream().cuda_stream, variant, border=border)
    torch.cuda.synchronize()
    s = src.cpu().numpy()
    assert (s[:GUARD] == CANARY).all() and (s[-GUARD:] == CANARY).all() and \
        np.array_equal(s[GUARD:-GUARD], dirty.reshape(-1)), "the source allocation was modified"
    return dst.cpu().numpy()


def expected(shape, lay, halo, ref_rows, lo, hi):
    """The destination allocation a launch must leave: canary everywhere but
    frame rows [lo, hi) x bytes [0, rb), which hold ref_rows ((hi - lo, rb))."""
    want = np.full(shape[0] * shape[1] + 2 * GUARD, CANARY, np.uint8)
    fr = want[GUARD:-GUARD].reshape(shape)
    if lo < hi:
        fr[halo + lo:halo + hi, PAD:PAD + lay["row_bytes"]] = ref_rows
    return want


def mismatch(got, want, shape):
    """None, or (count, first three (frame row, frame byte) | 'guard band')."""
    if np.array_equal(got, want):
        return None
    bad = np.flatnonzero(got != want)
    where = ["guard band" if i < GUARD or i >= got.size - GUARD else divmod(int(i) - GUARD, shape[1]) for i in bad[:3]]
    return len(bad), where
