"""The three single-step kernels of csrc/kernels/stencil.hip — k_binomial,
k_generic9<CH, false> ("int9") and k_generic9<CH, true> ("float9") — on a real
MI355X, held to the standard of tests/test_gpu_tile_edges.py.  `auto` sends
every one-step, zero-border launch of a single plain image to them: an engine
with fuse=1, the last launch of a run whose repetition count leaves a rest of
1, every phase of a band whose halo is 1.

Every variant is forced by name (a forced single-step variant runs or raises:
there is no fallback).  Sizes come from the kernels' own constants (a lane's
16 bytes, a workgroup's 1024 row bytes, 16 rows of k_binomial's row march and 4
of k_generic9): either side of a lane, of two lanes, of the workgroup seam and
of two workgroups, rows whose last lane holds 1 and 15 bytes, pixels across a
lane and across the seam, three workgroups in x, more than one in y.

Source frames follow the kernels' contract: they take the left / right
boundary from the frame's zero pad, so the pads of rows inside the global image
are zero, and the rows outside it — which the kernels must not load at all —
are 0xFF from end to end.  The destination ALLOCATION is compared byte for
byte: the reference in bytes [0, row_bytes) of the launched rows, zeros in
[row_bytes, round_up(row_bytes, 16)) (the lanes store whole 16-byte vectors),
canary everywhere else.  Images are saturated (255 blocks, checkerboards, half
lanes of 255 beside half lanes of 0 for k_binomial's packed pairs) and, for
the tap order, asymmetric filters on single-pixel impulses.

Reference: pconv.numpy_convolve for whole images, cpu_fused_launch on the clean
frame for band frames.  Bit-exact.  Harness: tests/tile_edges.py."""
import numpy as np
import pytest

import tile_edges as te
from tile_edges import CH, NEG_TAPS

pytestmark = pytest.mark.gpu

SWAR_SHAPES = te.module_shapes("swar_shapes")
FLOAT_SHAPES = te.module_shapes("float_shapes")

ASYM = [1, 0, 3, 2, 4, 0, 1, 3, 2]  # asymmetric in both axes, sum 16
# key -> what get_filter() / Filter.custom() take; int-exact: gaussian, asym16 (gain 1), asym8 (gain 2: saturates)
FILTERS = {"gaussian": "gaussian", "box": "box", "edge": "edge", "asym16": (ASYM, 16), "asym8": (ASYM, 8),
           "neg17": NEG_TAPS, "neg7": (NEG_TAPS[0], 7)}

_REF = {}  # (filter key, image key) -> NumPy result; emptied after every test
_IMG = {}


@pytest.fixture(autouse=True)
def forced(native):
    import torch

    prev = native.set_autotune(False)
    yield
    torch.cuda.synchronize()
    native.set_prefetch_mode(-1)
    native.set_swar_shape(0, 0, 0)
    native.set_swar_alt(-1)
    native.set_float_shape(0, 0)
    native.set_autotune(prev)
    _REF.clear()
    _IMG.clear()


def _native_filter(native, fkey):
    f = FILTERS[fkey]
    return native.Filter.by_name(f) if isinstance(f, str) else native.Filter.custom(list(f[0]), f[1], "custom")


def _taps(pconv_mod, fkey):
    f = pconv_mod.get_filter(FILTERS[fkey])
    return f.taps, f.divisor


def _image(kind, c, h, w):
    """(h, w c) uint8, one per key: `values` (random + planted), `full` (255),
    `checker`, `stripes_lo` / `stripes_hi` (half lanes of 255 and of 0),
    `impulse_a` / `impulse_b` (single 255 pixels at the lane and seam edges)."""
    key = (kind, c, h, w)
    if key not in _IMG:
        rb = w * c
        if kind == "values":
            img = te.values8(np.random.default_rng(1000003 * c + 1009 * h + w), h, rb)
        elif kind == "full":
            img = np.full((h, rb), 255, np.uint8)
        elif kind == "checker":
            img = te.checkerboard(h, rb)
        elif kind in ("stripes_lo", "stripes_hi"):
            img = te.half_lane_stripes(h, rb, kind == "stripes_lo")
        else:
            img, n = te.impulses(h, rb, c, flip=kind == "impulse_b")
            assert n >= 1
        _IMG[key] = img
    return key, _IMG[key]


def _oracle(pconv_mod, fkey, c, key, img):
    if (fkey, key) not in _REF:
        h, rb = img.shape
        x = img.reshape(h, rb // c, c) if c > 1 else img
        _REF[(fkey, key)] = pconv_mod.numpy_convolve(x, 1, FILTERS[fkey]).reshape(h, rb)
    return _REF[(fkey, key)]


def _whole(native, pconv_mod, c, key, img, fkey, variant):
    """The whole image in one launch: ghost rows of 0xFF, zero pads, an
    all-canary destination; (output rows, mismatch | None)."""
    h, rb = img.shape
    lay = native.frame_layout(rb, h, 1)
    rows = np.zeros((h + 2, rb), np.uint8)
    rows[1:1 + h] = img
    _, dirty = te.frames(lay, 1, rows, 1, 1, pads="zero")
    got = te.launch(native, dirty, lay, 1, _native_filter(native, fkey), c, 0, h, 1, 0, h, "zero", variant)
    want = te.expected(dirty.shape, lay, 1, _oracle(pconv_mod, fkey, c, key, img), 0, h, tail_zeros=True)
    bad = te.mismatch(got, want, dirty.shape)
    out = got[te.GUARD:-te.GUARD].reshape(dirty.shape)[1:1 + h, te.PAD:te.PAD + rb]
    return out, (bad and (variant, fkey, key[0], h, key[3]) + bad)


def _check(ran, planned, bad):
    assert ran == planned and ran > 0
    assert not bad, (len(bad), ran, bad[:8])


def test_shape_lists_were_read(native):
    assert SWAR_SHAPES == [tuple(s) for s in native.swar_shapes()] and len(SWAR_SHAPES) >= 2
    assert FLOAT_SHAPES == [tuple(s) for s in native.float_shapes()] and len(FLOAT_SHAPES) >= 2


@pytest.mark.parametrize("channels", ["grey", "rgb", "rgba"])
def test_binomial_every_edge(native, pconv_mod, channels):
    """k_binomial at every lane, seam and row-march edge.  All-255: the packed
    sums' maximum 16 x 255 must come back as 255 in the interior.  Half-lane
    stripes: the halves of every pair (b_k, b_k+8) hold 255 beside 0, and the
    bytes of a zero half whose +-c neighbours are zero stay 0 — a carry or a
    selector slip between the halves would land there."""
    c = CH[channels]
    kinds = ("values", "full", "checker", "stripes_lo", "stripes_hi")
    sizes = te.single_step_sizes("binomial", c)
    planned = len(sizes) * len(kinds)
    ran, deep, bad = 0, 0, []
    for h, w in sizes:
        for kind in kinds:
            key, img = _image(kind, c, h, w)
            out, r = _whole(native, pconv_mod, c, key, img, "gaussian", "binomial")
            ran += 1
            if r:
                bad.append(r)
            if kind == "full" and h >= 3 and w >= 3:
                assert (out[1:-1, c:-c] == 255).all(), (h, w, "the interior of an all-255 image")
            if kind.startswith("stripes"):
                cols = te.untouched_zero_columns(img, c)
                deep += int(cols.sum()) if kind == "stripes_hi" else 0
                assert not out[:, cols].any(), (kind, h, w, "non-zero bytes deep inside a zero half-lane")
    assert deep > 0
    _check(ran, planned, bad)


@pytest.mark.parametrize("channels", ["grey", "rgb", "rgba"])
def test_generic9_int_every_edge(native, pconv_mod, channels):
    """k_generic9's integer form: the gaussian, a filter asymmetric in both
    axes (tap order) and its gain-2 twin, whose sums pass 255 << shift (the
    clamp at 255; without it a byte spills into its neighbours).  `auto` takes
    the two custom filters to the same kernel: the same bytes."""
    c = CH[channels]
    kinds = ("values", "full", "checker")
    sizes = te.single_step_sizes("generic9", c)
    planned = len(sizes) * (3 * len(kinds) + 2)
    ran, over, bad = 0, 0, []
    for h, w in sizes:
        for fkey in ("gaussian", "asym16", "asym8"):
            assert _native_filter(native, fkey).int_exact
            for kind in kinds:
                key, img = _image(kind, c, h, w)
                _, r = _whole(native, pconv_mod, c, key, img, fkey, "int9")
                ran += 1
                if r:
                    bad.append(r)
                if fkey == "asym8":
                    taps, div = _taps(pconv_mod, fkey)
                    sat = te.exact_sums(img, c, taps) > 255 * div
                    over += int(sat.sum())
                    assert (_oracle(pconv_mod, fkey, c, key, img)[sat] == 255).all()
                    if kind == "full" and h >= 2 and w >= 2:  # a corner's taps alone sum to 9 > 8
                        assert sat.any(), (h, w, "no sum above 255 << shift")
            if fkey != "gaussian":
                key, img = _image("values", c, h, w)
                _, r = _whole(native, pconv_mod, c, key, img, fkey, "auto")
                ran += 1
                if r:
                    bad.append(r)
    assert over > 0
    _check(ran, planned, bad)


@pytest.mark.parametrize("channels", ["grey", "rgb", "rgba"])
def test_generic9_float_every_edge(native, pconv_mod, channels):
    """k_generic9's float form: box, edge, the asymmetric negative-tap filter
    (/17) and its taps over 7 (gain 17/7: the clamp at 255).  The impulse
    images lay every tap out alone: beside an impulse the -1 tap's exact sum is
    -255, so the clamp at 0 is reached by construction."""
    c = CH[channels]
    kinds = ("values", "checker", "impulse_a", "impulse_b")
    fkeys = ("box", "edge", "neg17", "neg7")
    sizes = te.single_step_sizes("generic9", c)
    planned = len(sizes) * len(kinds) * len(fkeys)
    ran, alone, bad = 0, 0, []
    below = dict.fromkeys(("neg17", "neg7"), 0)
    above = {"neg7": 0}
    for h, w in sizes:
        for fkey in fkeys:
            taps, div = _taps(pconv_mod, fkey)
            for kind in kinds:
                key, img = _image(kind, c, h, w)
                _, r = _whole(native, pconv_mod, c, key, img, fkey, "float9")
                ran += 1
                if r:
                    bad.append(r)
                if fkey in below:
                    s, ref = te.exact_sums(img, c, taps), _oracle(pconv_mod, fkey, c, key, img)
                    assert (ref[s < 0] == 0).all() and (ref[s >= 256 * div] == 255).all()
                    below[fkey] += int((s < 0).sum())
                    if fkey in above:
                        above[fkey] += int((s >= 256 * div).sum())
                    if kind.startswith("impulse"):  # every sum is one tap of one impulse
                        assert set(np.unique(s).tolist()) <= {0} | {255 * t for t in taps}, (h, w)
                        alone += int((s == -255).sum())
    assert all(below.values()) and all(above.values()) and alone > 0, (below, above, alone)
    _check(ran, planned, bad)


# the list of test_band_frames_zero_border_dirty_ghosts at steps = 1 ...
BAND_RANGES = lambda h, halo: [  # noqa: E731
    (0, h), (-(halo - 1), h + (halo - 1)), (1, h - 1), (-3, 5), (h - 2, h + 1), (7, 8)]
# ... and, for k_binomial's march of 4 rows per lane and 16 per workgroup: r0 off a multiple of 4 with
# (r1 - r0) % 4 = 1, 2 and 3, below and above 16 rows
MARCH_RANGES = [(1, 6), (2, 8), (-5, 26), (3, 30), (-1, 17), (5, 22)]
BAND_FILTERS = {"binomial": ("gaussian",), "int9": ("asym16", "asym8"), "float9": ("neg17", "neg7")}


@pytest.mark.parametrize("channels", ["grey", "rgb", "rgba"])
@pytest.mark.parametrize("variant", ["binomial", "int9", "float9"])
def test_band_frames_dirty_ghosts(native, variant, channels):
    """Band frames of a taller image: g_row0 != 0, frames whose owned rows reach
    past the image, partial [r0, r1) on and off the row march's multiples of 4;
    every frame row outside the image holds 0xFF from end to end and must not
    be loaded.  One narrow width and one across the 1024-byte seam.  Reference:
    cpu_fused_launch on the clean frame."""
    c = CH[channels]
    H, h, halo = 100, 30, 8
    ranges = BAND_RANGES(h, halo) + MARCH_RANGES
    assert all(r0 % 4 and (r1 - r0) % 4 for r0, r1 in MARCH_RANGES)
    assert {(r1 - r0) % 4 for r0, r1 in MARCH_RANGES} == {1, 2, 3}
    filters = [(k, _native_filter(native, k)) for k in BAND_FILTERS[variant]]
    rng = np.random.default_rng(97)
    ran, planned, empty = 0, 0, 0
    for w in (45, te.WG_BYTES // c + 1):
        rb = w * c
        lay = native.frame_layout(rb, h, halo)
        for g_row0 in (0, 35, H - h, -3, H - h + 4):
            top = min(max(-g_row0 + halo, 0), h + 2 * halo)         # frame rows above the image
            bottom = min(max(g_row0 + h + halo - H, 0), h + 2 * halo)  # and below it
            clean, dirty = te.frames(lay, halo, te.values8(rng, h + 2 * halo, rb), top, bottom, pads="zero")
            for (r0, r1) in ranges:
                if r0 - 1 < -halo or r1 + 1 > h + halo or r0 >= r1:
                    continue
                planned += len(filters)
                lo, hi = max(r0, -g_row0), min(r1, H - g_row0)
                empty += lo >= hi  # no owned row inside the image: nothing is launched, `want` is all canary
                for fkey, nf in filters:
                    cpu = np.zeros_like(clean)
                    native.cpu_fused_launch(nf, channels, rb, h, halo, clean.reshape(-1), cpu.reshape(-1), r0, r1, 1,
                                            g_row0, H)
                    want = te.expected(dirty.shape, lay, halo, cpu[halo + lo:halo + hi, te.PAD:te.PAD + rb], lo, hi,
                                       tail_zeros=True)
                    got = te.launch(native, dirty, lay, halo, nf, c, r0, r1, 1, g_row0, H, "zero", variant)
                    ran += 1
                    assert te.mismatch(got, want, dirty.shape) is None, \
                        (variant, fkey, w, g_row0, r0, r1, te.mismatch(got, want, dirty.shape))
    # 2 widths x 5 frames x 12 ranges (none reaches past the frame at one step)
    assert ran == planned == 2 * 5 * 12 * len(filters) and empty > 0


def test_auto_runs_the_single_step_kernels(native, pconv_mod):
    """`auto`, one step, zero border, one plain image: k_binomial for the
    gaussian and k_generic9 for box — the last-launch records of the fused
    kernels still name the launch made before, under another forced shape."""
    native.set_prefetch_mode(0)
    native.set_swar_alt(0)
    for channels in ("grey", "rgb", "rgba"):
        c = CH[channels]
        # a forced fused shape that cannot run falls back silently: take shapes that can
        a = next(s for s in SWAR_SHAPES if te.runs(*s, c, 2))
        b = next(s for s in reversed(SWAR_SHAPES) if te.runs(*s, c, 1) and s != a)
        fa, fb = FLOAT_SHAPES[0], FLOAT_SHAPES[-1]
        assert fa != fb and te.runs(8, *fa, c, 2) and te.runs(8, *fb, c, 1)
        h, w = 9, te.WG_BYTES // c + 1
        key, img = _image("values", c, h, w)
        rb = w * c
        # a two-step launch of each fused kernel under shapes A
        lay = native.frame_layout(rb, h, 2)
        rows = np.zeros((h + 4, rb), np.uint8)
        rows[2:2 + h] = img
        _, dirty = te.frames(lay, 2, rows, 2, 2)
        native.set_swar_shape(*a)
        native.set_float_shape(*fa)
        te.launch(native, dirty, lay, 2, "gaussian", c, 0, h, 2, 0, h, "zero", "temporal")
        te.launch(native, dirty, lay, 2, "box", c, 0, h, 2, 0, h, "zero", "float_temporal")
        assert tuple(native.last_swar_launch()) == (0,) + a + (0,) and tuple(native.last_float_launch()) == fa
        # shapes B could run one step; `auto` does not go there
        native.set_swar_shape(*b)
        native.set_float_shape(*fb)
        for fkey, variant in (("gaussian", "binomial"), ("box", "float9")):
            out_auto, r = _whole(native, pconv_mod, c, key, img, fkey, "auto")
            assert r is None, r
            assert tuple(native.last_swar_launch()) == (0,) + a + (0,), "auto ran a fused SWAR kernel"
            assert tuple(native.last_float_launch()) == fa, "auto ran the fused float kernel"
            out_forced, r = _whole(native, pconv_mod, c, key, img, fkey, variant)
            assert r is None, r
            assert np.array_equal(out_auto, out_forced)
        # the controls: the forced fused variants do move the records
        te.launch(native, dirty, lay, 2, "gaussian", c, 0, h, 1, 0, h, "zero", "temporal")
        te.launch(native, dirty, lay, 2, "box", c, 0, h, 1, 0, h, "zero", "float_temporal")
        assert tuple(native.last_swar_launch()) == (0,) + b + (0,) and tuple(native.last_float_launch()) == fb


ENGINE_SIZES = {"grey": (1100, 21), "rgb": (350, 19), "rgba": (257, 18)}  # (w, h): 1100, 1050 and 1028 row bytes


def _engine_image(c, h, w):
    return _image("values", c, h, w)[1].reshape((h, w, c) if c > 1 else (h, w))


@pytest.mark.parametrize("fkey", ["gaussian", "box", "asym8"])
@pytest.mark.parametrize("channels", ["grey", "rgb", "rgba"])
def test_engine_single_step_launches_cross_the_seam(pconv_mod, channels, fkey):
    """Engines whose single-step launches span more than one workgroup in x:
    fuse=1 (every launch), and fuse=4 at 5 repetitions (a fused launch, then
    one single step on the frame it left: uploads and fused launches keep the
    pads the single-step kernels rely on at zero)."""
    w, h = ENGINE_SIZES[channels]
    img = _engine_image(CH[channels], h, w)
    ref = {reps: pconv_mod.numpy_convolve(img, reps, FILTERS[fkey]) for reps in (1, 3, 5)}
    eng = pconv_mod.Engine(w, h, channels, FILTERS[fkey], fuse=1)
    for reps in (1, 3, 1):
        assert np.array_equal(eng(img, reps), ref[reps]), (channels, fkey, "fuse 1", reps)
    eng = pconv_mod.Engine(w, h, channels, FILTERS[fkey], fuse=4)
    for _ in range(2):  # the second run starts on frames the first one left
        assert np.array_equal(eng(img, 5), ref[5]), (channels, fkey, "fuse 4", 5)


@pytest.mark.parametrize("fkey", ["gaussian", "box", "asym8"])
@pytest.mark.parametrize("bands", [2, 3])
def test_local_cluster_halo_one_crosses_the_seam(pconv_mod, bands, fkey):
    """Bands of halo 1: every phase is a single-step launch, on frames whose
    ghost rows the halo transport fills; 1100 grey bytes, two workgroups."""
    n = pconv_mod.native
    w, h, reps = 1100, 45, 3
    img = _engine_image(1, h, w)
    cl = n.LocalCluster(w, h, "grey", _native_filter(n, fkey), bands, 0, 1, 1)
    for preload in (False, True):
        cl.upload(img.reshape(-1), preload)
        cl.run(reps)
        out = np.empty_like(img)
        cl.download(out.reshape(-1))
        assert np.array_equal(out, pconv_mod.numpy_convolve(img, reps, FILTERS[fkey])), (bands, fkey, preload)
