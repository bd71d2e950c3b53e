"""Harness of tests/test_gpu_tile_edges.py and tests/test_gpu_single_step.py:
tile geometry of the fused 8-bit kernels and lane / workgroup geometry of the
single-step ones, sizes derived from them, test images, dirty canary-guarded
frames and the byte-for-byte comparison of a launch's whole destination
allocation.

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


# ---- the single-step kernels (k_binomial, k_generic9) ------------------------------
# A lane owns 16 row bytes, a workgroup is 64 lanes (1024 row bytes) x 4 row
# groups; a lane of k_binomial marches down RPT = 4 rows, one of k_generic9
# makes one row.

LANE = 16
WG_BYTES = 64 * LANE
RPT = 4
WG_ROWS = {"binomial": 4 * RPT, "generic9": 4}
SINGLE_STEP_HEIGHTS = {"binomial": (1, 2, 3, RPT, RPT + 1, 4 * RPT - 1, 4 * RPT, 4 * RPT + 1, 2 * 4 * RPT + 1),
                       "generic9": (1, 2, 3, 4, 5, 2 * 4 + 1)}


def partial_valids(c):
    """The smallest and the largest count of valid bytes (1..15) a row of whole
    c-byte pixels can leave in its last lane: 1 and 15 for grey and RGB; an
    RGBA row ends on a multiple of 4 bytes, so 4 and 12."""
    g = math.gcd(c, LANE)
    return g, LANE - g


def single_step_widths(c):
    """Pixel widths of c-byte pixels: one and two pixels; the whole-pixel
    widths nearest below, at (where c divides it) and above one lane, two
    lanes, one workgroup and two workgroups (the last: three workgroups in x);
    the smallest rows that end on each of partial_valids(c) bytes of a lane
    and on a full lane."""
    ws = [1, 2]
    for edge in (LANE, 2 * LANE, WG_BYTES, 2 * WG_BYTES):
        ws += [(edge - 1) // c] + ([edge // c] if edge % c == 0 else []) + [edge // c + 1]
    for valid in partial_valids(c) + (0,):  # 0: the row's last lane is full (RGB: 48 bytes)
        ws += [w for w in range(1, 2 * LANE + 1) if (w * c) % LANE == valid][:1]
    return sorted({w for w in ws if w >= 1})


def seam_widths(c):
    """The widths of single_step_widths(c) either side of (and at) the 1024-byte seam."""
    return [w for w in single_step_widths(c) if abs(w * c - WG_BYTES) <= c]


def single_step_sizes(kernel, c):
    """[(h, w)] in pixels for `kernel` ("binomial" | "generic9"), paired and not
    multiplied out: the seam widths at every height up to one row group and a
    row; the taller heights at a width just past the seam, at the narrowest
    partial last lane and at three workgroups; every other width once, the
    heights taken in turn."""
    hs = SINGLE_STEP_HEIGHTS[kernel]
    ws = single_step_widths(c)
    small = [h for h in hs if h <= 5]
    tall = [h for h in hs if h > 5]
    seam = seam_widths(c)
    few = [max(seam), min(w for w in ws if (w * c) % LANE == partial_valids(c)[0]), max(ws)]
    out = [(h, w) for w in seam for h in small] + [(h, w) for h in tall for w in few]
    out += [(hs[i % len(hs)], w) for i, w in enumerate(w for w in ws if w not in seam)]
    seen, uniq = set(), []
    for s in out:
        if s not in seen:
            seen.add(s)
            uniq.append(s)
    return uniq


# ---- images (h, rb) uint8 -----------------------------------------------------


def half_lane_stripes(h, rb, low):
    """255 in the low (bytes x % 16 < 8) or the high half of every 16-byte lane,
    0 in the other: the two 16-bit halves of k_binomial's pairs (b_k, b_k+8)
    hold the maximum beside zero."""
    lit = (np.arange(rb) % LANE < LANE // 2) == bool(low)
    return np.repeat(np.where(lit, 255, 0).astype(np.uint8)[None], h, axis=0)


def untouched_zero_columns(img, c):
    """Byte columns of img that are zero and whose neighbours c bytes to the
    left and to the right are zero (or outside the row) in every row: a 3 x 3
    step under the zero border leaves them zero whatever its taps."""
    z = ~img.any(axis=0)
    left = np.concatenate([np.ones(c, bool), z[:-c]]) if img.shape[1] > c else np.ones_like(z)
    right = np.concatenate([z[c:], np.ones(c, bool)]) if img.shape[1] > c else np.ones_like(z)
    return z & left & right


def impulses(h, rb, c, flip=False):
    """Single 255 pixels on black, at least 3 pixels apart in x or in y, so
    that every tap of a 3 x 3 filter shows alone: on the pixels that hold the
    bytes either side of the 1024-byte seam, the row's first and last byte and
    a lane's last and the next lane's first byte, tried in the first and then
    in the last row.  Neighbouring targets cannot share a row; `flip` gives the
    other one of each pair the first pick.  Returns (image, impulse count)."""
    pairs = [(WG_BYTES - 1, WG_BYTES), (0, rb - 1), (LANE - 1, LANE), (WG_BYTES - LANE, WG_BYTES + LANE - 1)]
    targets = [b for p in pairs for b in (p[::-1] if flip else p) if 0 <= b < rb]
    img = np.zeros((h, rb), np.uint8)
    placed = []
    for y in dict.fromkeys((0, h - 1)):
        for b in targets:
            px = b // c
            if all(max(abs(y - py), abs(px - qx)) >= 3 for py, qx in placed) and (y, px) not in placed:
                placed.append((y, px))
                img[y, px * c:(px + 1) * c] = 255
    return img, len(placed)


def exact_sums(img, c, taps):
    """sum tap x sample of one 3 x 3 step under the zero border, in int64: what
    the clamps at 0 and at 255 are applied to, before the division."""
    h, rb = img.shape
    p = np.pad(img.astype(np.int64).reshape(h, rb // c, c), ((1, 1), (1, 1), (0, 0)))
    s = np.zeros((h, rb // c, c), np.int64)
    for k in range(3):
        for l in range(3):
            s += int(taps[3 * k + l]) * p[k:k + h, l:l + rb // c]
    return s.reshape(h, rb)



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


def frames(lay, halo, rows_img, top_ghosts=0, bottom_ghosts=0, pads="dirty"):
    """(clean, dirty) frames ((h + 2 halo, pitch) uint8) of rows_img ((h + 2
    halo, rb): ghost rows included).  Frame rows [0, top_ghosts) and the last
    bottom_ghosts ones lie outside the global image.  clean: zeros there and in
    every pad; dirty: 0xFF there, in the 16 left pad bytes and right of rb.
    pads="zero" is the single-step kernels' contract (they take the left and
    right boundary from the frame's pad): the pads of every row inside the
    global image stay zero, the rows outside it are 0xFF from end to end."""
    assert pads in ("dirty", "zero")
    n, rb = rows_img.shape
    clean = np.zeros((n, lay["pitch"]), np.uint8)
    clean[:, PAD:PAD + rb] = rows_img
    clean[:top_ghosts] = 0
    clean[n - bottom_ghosts:] = 0
    dirty = clean.copy()
    dirty[:top_ghosts] = 0xFF
    dirty[n - bottom_ghosts:] = 0xFF
    if pads == "dirty":
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


def expected(shape, lay, halo, ref_rows, lo, hi, tail_zeros=False):
    """The destination allocation a launch must leave: canary everywhere but
    frame rows [lo, hi) x bytes [0, rb), which hold ref_rows ((hi - lo, rb)).
    tail_zeros: the vector-store contract of the single-step kernels, whose
    lanes store whole 16-byte vectors — bytes [rb, round_up(rb, 16)) of those
    rows hold 0, and everything else is canary all the same."""
    want = np.full(shape[0] * shape[1] + 2 * GUARD, CANARY, np.uint8)
    fr = want[GUARD:-GUARD].reshape(shape)
    if lo < hi:
        rb = lay["row_bytes"]
        fr[halo + lo:halo + hi, PAD:PAD + rb] = ref_rows
        if tail_zeros:
            fr[halo + lo:halo + hi, PAD + rb:PAD + -(-rb // LANE) * LANE] = 0
    return want


def mismatch(got, want, shape):
    """None, or (count, first three (frame row, frame byte) | 'guard band')."""
    if np.array_equal(got, want):
        return None
    bad = np.flatnonzero(got != want)
    where = ["guard band" if i < GUARD or i >= got.size - GUARD else divmod(int(i) - GUARD, shape[1]) for i in bad[:3]]
    return len(bad), where
