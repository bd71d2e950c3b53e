"""The three fused 8-bit kernels (k_swar, k_swar_pf, k_float_temporal) on a real
MI355X, held to the standard of tests/test_gpu_depth16.py: every row of
swar_shapes(), swar_prefetch_shapes() and float_shapes() forced, on sizes
derived from that row's own tile (one pixel, either side of a strip edge and of
a tile edge, two tiles plus a rest, 3 and 4 column strips), both step forms,
both borders, steps up to 16.

Frames are dirty: 0xFF in the 16 left pad bytes, in everything right of
row_bytes and in every ghost row outside the global image, which every kernel
must read as zeros.  Images carry saturated content (blocks of 255,
checkerboards, whole strips of 255 beside strips of 0), where a slip between
the two 16-bit fields of a SWAR register would show.  The destination
ALLOCATION is compared byte for byte with "reference where the launch may write,
canary everywhere else", and after every launch last_swar_launch() /
last_float_launch() must name the kernel, shape and form that were forced (a
forced choice that cannot run falls back silently).

Reference: pconv.numpy_convolve for whole images, cpu_fused_launch on the clean
frame (zeros where the dirty one holds 0xFF) for band frames.  Bit-exact.
Harness: tests/tile_edges.py."""
import math

import numpy as np
import pytest

import tile_edges as te
from tile_edges import BORDERS, CH, NEG_TAPS

pytestmark = pytest.mark.gpu

SWAR_SHAPES = te.module_shapes("swar_shapes")
BUFOP_SHAPES = te.module_shapes("swar_prefetch_shapes")
FLOAT_SHAPES = te.module_shapes("float_shapes")
SWAR_STEPS = (1, 2, 3, 8, 16)
FLOAT_STEPS = (1, 3, 4, 8)

_REF = {}  # (filter, c, image key, steps, border) -> NumPy result; emptied after every test
_IMG = {}


def _sid(s):
    return "x".join(str(v) for v in s)


@pytest.fixture(autouse=True)
def forced(native):
    import torch

    prev = native.set_autotune(False)
    yield
    torch.cuda.synchronize()
    native.set_prefetch_mode(-1)
    native.set_xcd_swizzle(True)
    native.set_swar_shape(0, 0, 0)
    native.set_swar_alt(-1)
    native.set_float_shape(0, 0)
    native.set_autotune(prev)
    _REF.clear()
    _IMG.clear()


def _image(kind, c, h, w, vs=0):
    """(h, w c) uint8, one per key: `values` (random + planted), `full` (255),
    `checker`, and the strip images of vs-byte strips — even / odd: strips of
    that parity hold 255, the others 0; low / high: the strips left / right of
    the middle, so that a register's A and B strips differ."""
    key = (kind, c, h, w, vs if kind in ("even", "odd", "low", "high") else 0)
    if key not in _IMG:
        rb = w * c
        if kind == "values":
            img = te.values8(np.random.default_rng(1000003 * c + 1009 * h + w), h, rb)
        elif kind == "full":
            img = np.full((h, rb), 255, np.uint8)
        elif kind == "checker":
            img = te.checkerboard(h, rb)
        else:
            img = te.strip_image(h, rb, vs, _lit(kind, rb, vs))
        _IMG[key] = img
    return key, _IMG[key]


def _lit(kind, rb, vs):
    ps = te.strips(rb, vs)[1]
    return {"even": lambda k: k % 2 == 0, "odd": lambda k: k % 2 == 1, "low": lambda k: k < ps,
            "high": lambda k: k >= ps}[kind]


def _oracle(pconv_mod, fkey, filt, c, key, img, steps, border):
    k = (fkey, key, steps, border)
    if k not in _REF:
        h, rb = img.shape
        x = img.reshape(h, rb // c, c) if c > 1 else img
        _REF[k] = pconv_mod.numpy_convolve(x, steps, filt, border).reshape(h, rb)
    return _REF[k]


def _whole(native, pconv_mod, c, key, img, steps, border, variant, fkey="gaussian", filt="gaussian", nfilt=None):
    """The whole image in one launch on a dirty frame; (got rows, mismatch)."""
    h, rb = img.shape
    lay = native.frame_layout(rb, h, steps)
    rows = np.zeros((h + 2 * steps, rb), np.uint8)
    rows[steps:steps + h] = img
    _, dirty = te.frames(lay, steps, rows, steps, steps)
    got = te.launch(native, dirty, lay, steps, filt if nfilt is None else nfilt, c, 0, h, steps, 0, h, border, variant)
    want = te.expected(dirty.shape, lay, steps, _oracle(pconv_mod, fkey, filt, c, key, img, steps, border), 0, h)
    bad = te.mismatch(got, want, dirty.shape)
    out = got[te.GUARD:-te.GUARD].reshape(dirty.shape)[steps:steps + h, te.PAD:te.PAD + rb]
    return out, (bad and (key[0], h, key[3], steps, border) + bad)


def _assert_swar_ran(native, kern, shape, form):
    assert tuple(native.last_swar_launch()) == (kern,) + tuple(shape) + (form,), "another kernel, shape or form ran"


def test_shape_lists_were_read(native):
    """The parametrize lists above are the module's, row for row."""
    assert SWAR_SHAPES == [tuple(s) for s in native.swar_shapes()] and len(SWAR_SHAPES) >= 19
    assert BUFOP_SHAPES == [tuple(s) for s in native.swar_prefetch_shapes()] and len(BUFOP_SHAPES) >= 6
    assert FLOAT_SHAPES == [tuple(s) for s in native.float_shapes()] and len(FLOAT_SHAPES) >= 5
    assert set(BUFOP_SHAPES) <= set(SWAR_SHAPES)


def _swar_sweep(native, pconv_mod, kern, shape, c):
    """Every planned (steps, size, form, border[, swizzle]) of one shape;
    returns (launches, planned launches, mismatches, step counts run)."""
    lw, m, nw = shape
    native.set_swar_shape(lw, m, nw)
    native.set_prefetch_mode(kern)
    ran, planned, bad, steps_run = 0, 0, [], []
    for steps in SWAR_STEPS:
        if not te.runs(lw, m, nw, c, steps):
            continue
        steps_run.append(steps)
        sizes = [s + (False,) for s in te.tile_sizes(lw, m, nw, c, steps)] if kern == 0 else \
            te.bufop_sizes(m, nw, c, steps)
        for h, w, small, both_orders in sizes:
            halve = small and steps >= 8  # a small size at deep fusion: one border per form
            planned += (2 if halve else 4) * (2 if both_orders else 1)
            assert kern == 0 or (w * c) % 4 == 0
            key, img = _image("values", c, h, w)
            for form in (0, 1):
                native.set_swar_alt(form)
                for border in BORDERS:
                    if halve and border == BORDERS[form]:
                        continue
                    for swz in ((True, False) if both_orders else (True,)):
                        native.set_xcd_swizzle(swz)
                        _, r = _whole(native, pconv_mod, c, key, img, steps, border, "temporal")
                        _assert_swar_ran(native, kern, shape, form)
                        ran += 1
                        if r:
                            bad.append((form, swz) + r)
    return ran, planned, bad, steps_run


def _check_sweep(ran, planned, bad, steps_run, lw, m, nw, c, all_steps):
    assert steps_run == [s for s in all_steps if te.runs(lw, m, nw, c, s)], "a step count left out for another reason"
    if lw < c:  # a lane holds no whole pixel (no such row today): nothing to run
        assert ran == planned == 0
        return
    assert len(steps_run) >= 3 and set(all_steps[:3]) <= set(steps_run)  # every row allows 1, 2 and 3 steps
    assert ran == planned and ran > 0
    assert not bad, (len(bad), ran, bad[:8])


@pytest.mark.parametrize("channels", ["grey", "rgb", "rgba"])
@pytest.mark.parametrize("shape", SWAR_SHAPES, ids=_sid)
def test_swar_tile_kernel_every_shape(native, pconv_mod, shape, channels):
    """k_swar in every row of swar_shapes() x forms x borders x steps 1-16 at
    the shape's own strip and tile edges."""
    c = CH[channels]
    ran, planned, bad, steps_run = _swar_sweep(native, pconv_mod, 0, shape, c)
    _check_sweep(ran, planned, bad, steps_run, *shape, c, SWAR_STEPS)


@pytest.mark.parametrize("channels", ["grey", "rgb", "rgba"])
@pytest.mark.parametrize("shape", BUFOP_SHAPES, ids=_sid)
def test_swar_bufop_kernel_every_shape(native, pconv_mod, shape, channels):
    """k_swar_pf in every row of swar_prefetch_shapes(), rows of whole dwords
    only; both tile orders on the two-tile size."""
    c = CH[channels]
    assert shape[0] == 4
    ran, planned, bad, steps_run = _swar_sweep(native, pconv_mod, 1, shape, c)
    _check_sweep(ran, planned, bad, steps_run, *shape, c, SWAR_STEPS)


@pytest.mark.parametrize("filt", ["box", "neg"])
@pytest.mark.parametrize("channels", ["grey", "rgb", "rgba"])
@pytest.mark.parametrize("shape", FLOAT_SHAPES, ids=_sid)
def test_float_temporal_every_shape_zero_border(native, pconv_mod, shape, channels, filt):
    """k_float_temporal in every row of float_shapes() under the zero border:
    the uniform path (box) and the non-uniform one with the clamp at 0 (a
    negative tap), the tile-edge sizes with 8-byte lanes, rows whose last chunk
    holds 1, 4, 5 and 8 bytes, and all-255 / checkerboard images (box takes 255
    to 254: the truncation is exercised)."""
    c = CH[channels]
    m, nw = shape
    native.set_float_shape(m, nw)
    nf = native.Filter.custom(NEG_TAPS[0], NEG_TAPS[1], "custom") if filt == "neg" else filt
    pf = pconv_mod.get_filter(NEG_TAPS) if filt == "neg" else filt
    ran, planned, bad, steps_run = 0, 0, [], []
    for steps in FLOAT_STEPS:
        if not te.runs(8, m, nw, c, steps):
            continue
        steps_run.append(steps)
        _, vs, vrows = te.geom(8, m, nw, c, steps)
        wpx = -(-vs // c)
        for h, w, _small in te.tile_sizes(8, m, nw, c, steps, chunk_valid=(1, 4, 5, 8)):
            kinds = ["values"] + (["full", "checker"] if (h, w) in ((vrows + 1, wpx + 1), (3, wpx)) else [])
            planned += len(kinds)
            for kind in kinds:
                key, img = _image(kind, c, h, w)
                _, r = _whole(native, pconv_mod, c, key, img, steps, "zero", "float_temporal", fkey=filt, filt=pf,
                              nfilt=nf)
                assert tuple(native.last_float_launch()) == shape, "another float shape ran"
                ran += 1
                if r:
                    bad.append(r)
    _check_sweep(ran, planned, bad, steps_run, 8, m, nw, c, FLOAT_STEPS)


def _isolation_shape(kernel):
    """The first table row of the kind that runs 16 steps."""
    rows = BUFOP_SHAPES if kernel == "bufop" else [s for s in SWAR_SHAPES if s[0] == (8 if kernel == "tile8" else 4)]
    return next(s for s in rows if s[1] * s[2] > 32)


@pytest.mark.parametrize("channels", ["grey", "rgb", "rgba"])
@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("kernel", ["tile8", "tile4", "bufop"])
def test_field_isolation(native, pconv_mod, kernel, form, channels):
    """Whole column strips of 255 beside whole strips of 0 (by strip parity,
    and by register field: the A strips against the B strips) and the all-255
    image, on 2, 3 and 4 strips.  Besides equality with NumPy: under the zero
    border the bytes deep inside a zero strip, further than `steps` pixels from
    its boundaries, are 0 — a leak between a register's fields would land there."""
    c = CH[channels]
    shape = _isolation_shape(kernel)
    lw, m, nw = shape
    kern = 1 if kernel == "bufop" else 0
    native.set_swar_shape(lw, m, nw)
    native.set_prefetch_mode(kern)
    native.set_swar_alt(form)
    px = 4 // math.gcd(c, 4) if kern else 1  # rows of whole dwords: a multiple of px pixels
    ran, deep, bad = 0, 0, []
    for steps in (2, 3, 16):
        assert te.runs(lw, m, nw, c, steps)
        _, vs, vrows = te.geom(lw, m, nw, c, steps)
        wpx = -(-vs // c)
        for n in (2, 3, 4):
            w = -(-((n - 1) * wpx + 1) // px) * px
            rb = w * c
            assert te.strips(rb, vs)[0] == n
            for kind in ("even", "odd", "low", "high", "full"):
                key, img = _image(kind, c, vrows + 1, w, vs)
                for border in BORDERS:
                    out, r = _whole(native, pconv_mod, c, key, img, steps, border, "temporal")
                    _assert_swar_ran(native, kern, shape, form)
                    ran += 1
                    if r:
                        bad.append(r)
                    if border == "zero" and kind != "full":
                        cols = te.deep_zero_columns(rb, vs, c, steps, _lit(kind, rb, vs))
                        deep += int(cols.sum())
                        assert not out[:, cols].any(), (kind, n, steps, "non-zero bytes deep inside a zero strip")
    assert ran == 3 * 3 * 5 * 2 and deep > 0
    assert not bad, (len(bad), bad[:8])


BAND_RANGES = lambda h, halo, steps: [  # noqa: E731  the list of test_band_frames_against_cpu_fused_launch
    (0, h), (-(halo - steps), h + (halo - steps)), (steps, h - steps), (-3, 5), (h - 2, h + 1), (7, 8)]


@pytest.mark.parametrize("kernel", ["k_swar", "k_swar_pf", "k_float_temporal"])
def test_band_frames_zero_border_dirty_ghosts(native, kernel):
    """Band frames of a taller image under the zero border: g_row0 != 0, frames
    whose owned rows reach past the image, partial [r0, r1); the ghost rows
    outside the image and every pad hold 0xFF.  Reference: cpu_fused_launch on
    the clean frame."""
    H, h, c, halo = 100, 30, 3, 8
    w = 44 if kernel == "k_swar_pf" else 45
    rb = w * c
    filt, variant = ("box", "float_temporal") if kernel == "k_float_temporal" else ("gaussian", "temporal")
    if kernel == "k_float_temporal":
        settings = [(s, None) for s in (FLOAT_SHAPES[0], FLOAT_SHAPES[-1])]
    else:
        rows = BUFOP_SHAPES[:2] if kernel == "k_swar_pf" else [_isolation_shape("tile8"), _isolation_shape("tile4")]
        settings = [(s, f) for s in rows for f in (0, 1)]
        native.set_prefetch_mode(1 if kernel == "k_swar_pf" else 0)
    lay = native.frame_layout(rb, h, halo)
    rng = np.random.default_rng(97)
    ran, planned = 0, 0
    for g_row0 in (0, 35, H - h, -3, H - h + 4):
        top = min(max(-g_row0 + halo, 0), h + 2 * halo)         # frame rows above the image
        bottom = min(max(g_row0 + h + halo - H, 0), h + 2 * halo)  # and below it
        clean, dirty = te.frames(lay, halo, te.values8(rng, h + 2 * halo, rb), top, bottom)
        for steps in (1, 3, 8):
            for (r0, r1) in BAND_RANGES(h, halo, steps):
                if r0 - steps < -halo or r1 + steps > h + halo or r0 >= r1:
                    continue
                planned += len(settings)
                cpu = np.zeros_like(clean)
                native.cpu_fused_launch(filt, "rgb", rb, h, halo, clean.reshape(-1), cpu.reshape(-1), r0, r1, steps,
                                        g_row0, H)
                lo, hi = max(r0, -g_row0), min(r1, H - g_row0)
                want = te.expected(dirty.shape, lay, halo, cpu[halo + lo:halo + hi, te.PAD:te.PAD + rb], lo, hi)
                for shape, form in settings:
                    if form is None:
                        native.set_float_shape(*shape)
                    else:
                        native.set_swar_shape(*shape)
                        native.set_swar_alt(form)
                    got = te.launch(native, dirty, lay, halo, filt, c, r0, r1, steps, g_row0, H, "zero", variant)
                    if lo >= hi:
                        pass  # no owned row inside the image: nothing is launched, `want` is all canary
                    elif form is None:
                        assert tuple(native.last_float_launch()) == shape
                    else:
                        _assert_swar_ran(native, 1 if kernel == "k_swar_pf" else 0, shape, form)
                    ran += 1
                    assert te.mismatch(got, want, dirty.shape) is None, \
                        (shape, form, g_row0, r0, r1, steps, te.mismatch(got, want, dirty.shape))
    # 5 frames x (6 + 6 + 4 ranges at 1, 3 and 8 steps: the range filter drops (-3, 5) and (h - 2, h + 1) at 8)
    assert ran == planned == 5 * 16 * len(settings)


def test_grid_sizes_around_the_xcd_count(native, pconv_mod):
    """Grids of exactly 1, 7, 8, 9, 15, 16 and 17 workgroups (pair_stride x
    row_tiles) of k_swar, XCD-aware tile order on and off: the remap's q = 0
    and rem != 0 branches.  Odd strip counts, too: the last tile has no B strip."""
    # workgroups: (pair_stride, row_tiles)
    grids = {1: (1, 1), 7: (1, 7), 8: (2, 4), 9: (3, 3), 15: (3, 5), 16: (4, 4), 17: (17, 1)}
    steps, ran = 1, 0
    native.set_prefetch_mode(0)
    native.set_swar_alt(1)
    for shape in ((4, 2, 16), (8, 2, 16)):
        assert shape in SWAR_SHAPES
        native.set_swar_shape(*shape)
        for c in (1, 3):
            _, vs, vrows = te.geom(*shape, c, steps)
            for wgs, (ps, rt) in grids.items():
                for nstrips in (2 * ps - 1, 2 * ps):
                    w = -(-((nstrips - 1) * vs + 5) // c)
                    h = rt * vrows - (wgs & 1)
                    assert te.strips(w * c, vs) == (nstrips, ps) and -(-h // vrows) == rt and ps * rt == wgs
                    key, img = _image("values", c, h, w)
                    for swz in (True, False):
                        native.set_xcd_swizzle(swz)
                        _, r = _whole(native, pconv_mod, c, key, img, steps, "zero", "temporal")
                        _assert_swar_ran(native, 0, shape, 1)
                        ran += 1
                        assert r is None, (shape, c, wgs, nstrips, swz, r)
    assert ran == 2 * 2 * 7 * 2 * 2
