"""Mixed-size image batches on a real MI355X: per-image extents
(StencilLaunch dims / dims_host) in the fused launches of the SWAR tile kernel,
the buffer-op tile kernel, the float temporal kernel and the residual kernel,
then ``BatchEngine.run_images`` and ``convolve_many(backend="hip")``.

Kernel level (test_gpu_batch.py's pattern): the frames of one ENVELOPE geometry
lie at a stride with a gap, between canaries.  Image b sits top-left in its
frame; every other source byte — the rest of the envelope, ghost rows, pad
columns, the gaps — is 0x77, which is what catches a missed mask.  The
destination is prefilled with a pattern and compared BYTE FOR BYTE with the
expected allocation: each image's rows and bytes are the NumPy oracle of that
image ALONE, everything else is the pattern.  The source must be unmodified.

The envelope is the smallest image with 3 strips and 2 row tiles of the forced
shape (4 tiles per image; five images make 20 workgroups, the XCD remap's
remainder path).  Shapes are forced and tuning is off."""
import math

import numpy as np
import pytest

import batch_converge_recipe as rcp

pytestmark = pytest.mark.gpu

GUARD = 4096
CANARY = 0xA5
JUNK = 0x77
NAME = {1: "grey", 3: "rgb", 4: "rgba"}
NEG_TAPS = ([3, 1, 0, 2, 5, 1, -1, 2, 4], 17)
BORDERS = ["zero", "replicate"]
STEPS = (1, 3, 8, 16)

# hard-coded copies of the shape tables (tests/test_shape_tables.py pins them)
SWAR_SHAPES = [(8, 8, 8), (8, 8, 4), (8, 16, 4), (8, 4, 8), (4, 8, 8), (4, 6, 8), (4, 5, 8), (4, 4, 8), (4, 3, 8),
               (4, 4, 16), (4, 2, 16), (4, 3, 16), (8, 2, 16), (8, 4, 16), (4, 16, 4), (4, 12, 4), (4, 16, 8),
               (4, 12, 8), (4, 20, 8)]
PF_SHAPES = [(4, 8, 8), (4, 16, 4), (4, 12, 4), (4, 16, 8), (4, 12, 8), (4, 20, 8)]
FLOAT_SHAPES = [(16, 8), (16, 4), (8, 8), (8, 4), (4, 8)]

_IMG = {}  # (c, h, w) -> image
_REF = {}  # (filter key, border, c, h, w, steps) -> oracle


@pytest.fixture(autouse=True)
def forced(native):
    prev = native.set_autotune(False)
    yield
    native.set_prefetch_mode(-1)
    native.set_swar_shape(0, 0, 0)
    native.set_swar_alt(-1)
    native.set_float_shape(0, 0)
    native.set_xcd_swizzle(True)
    native.set_autotune(prev)


def _image(c, h, w):
    key = (c, h, w)
    if key not in _IMG:
        rng = np.random.default_rng(613 * c + 104729 * h + w)
        img = rng.integers(0, 256, size=(h, w, c) if c > 1 else (h, w), dtype=np.uint8)
        img.setflags(write=False)
        _IMG[key] = img
    return _IMG[key]


def _oracle(pconv_mod, fkey, filt, border, c, h, w, steps):
    key = (fkey, border, c, h, w, steps)
    if key not in _REF:
        _REF[key] = pconv_mod.numpy_convolve(_image(c, h, w), steps, filt, border=border)
    return _REF[key]


def _dims_table(sizes, c):
    """(host list of (row_bytes, height), device int32 tensor of the same)."""
    import torch

    host = [(w * c, h) for w, h in sizes]
    return host, torch.tensor(host, dtype=torch.int32, device="cuda").contiguous()


def _launch_ragged(native, pconv_mod, fkey, filt, c, H, W, steps, variant, border, sizes, capacity=None, gap=48,
                   nfilt=None):
    """The images of `sizes` [(w, h)] in frames of the envelope (c, H, W), one
    launch; returns the list of mismatches (empty: all as expected)."""
    import torch

    batch = len(sizes)
    capacity = batch if capacity is None else capacity
    rb, halo = W * c, steps
    lay = native.frame_layout(rb, H, halo)
    pitch, fbytes = lay["pitch"], lay["bytes"]
    stride = fbytes + gap
    total = capacity * stride
    src_host = np.full((capacity, stride), JUNK, np.uint8)
    pattern = ((np.arange(total, dtype=np.int64) * 31 + 7) & 0xFF).astype(np.uint8).reshape(capacity, stride)
    exp_host = pattern.copy()
    for b, (w, h) in enumerate(sizes):
        fr = src_host[b, :fbytes].reshape(H + 2 * halo, pitch)
        fr[halo:halo + h, 16:16 + w * c] = _image(c, h, w).reshape(h, w * c)
        ex = exp_host[b, :fbytes].reshape(H + 2 * halo, pitch)
        ex[halo:halo + h, 16:16 + w * c] = _oracle(pconv_mod, fkey, filt, border, c, h, w, steps).reshape(h, w * c)
    src = torch.full((total + 2 * GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    dst = torch.full((total + 2 * GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    src[GUARD:GUARD + total] = torch.from_numpy(src_host.reshape(-1)).cuda()
    dst[GUARD:GUARD + total] = torch.from_numpy(pattern.reshape(-1)).cuda()
    host, dev = _dims_table(sizes, c)
    base = GUARD + pitch * halo + 16
    native.launch_stencil(filt if nfilt is None else nfilt, NAME[c], src.data_ptr() + base, dst.data_ptr() + base, pitch,
                          rb, 0, H, -halo, H + halo, steps, 0, H, torch.cuda.current_stream().cuda_stream, variant,
                          border=border, batch=batch, batch_stride=stride, dims=host, dims_ptr=dev.data_ptr())
    torch.cuda.synchronize()
    d = dst.cpu().numpy()
    case = (fkey, variant, border, c, H, W, steps, tuple(sizes), capacity)
    bad = []
    if not ((d[:GUARD] == CANARY).all() and (d[-GUARD:] == CANARY).all()):
        bad.append(case + ("write outside the allocation",))
    got = d[GUARD:-GUARD].reshape(capacity, stride)
    if not np.array_equal(got, exp_host):
        b = int(np.argwhere((got != exp_host).any(axis=1))[0][0])
        off = np.argwhere(got[b] != exp_host[b])[:3].reshape(-1).tolist()
        where = [(o // pitch - halo, o % pitch - 16) if o < fbytes else ("gap", o - fbytes) for o in off]
        bad.append(case + (f"image {b}: first differing (row, byte) {where}",))
    s = src.cpu().numpy()
    if not ((s[:GUARD] == CANARY).all() and (s[-GUARD:] == CANARY).all()
            and np.array_equal(s[GUARD:-GUARD], src_host.reshape(-1))):
        bad.append(case + ("the source was modified",))
    return bad


# ---- the geometry formulas of swar_geom / ft_geom (as in test_gpu_batch.py) ----


def _swar_geom(lw, m, nw, c, steps):
    hl = (steps * c + lw - 1) // lw
    vbytes, vrows = (64 - 2 * hl) * lw, m * nw - 2 * steps
    return vbytes, vrows, vbytes > 0 and vrows > 0 and lw >= c


def _swar_image(lw, m, nw, c, steps, dword_rows):
    vbytes, vrows, ok = _swar_geom(lw, m, nw, c, steps)
    assert ok
    w = 2 * vbytes // c + 1
    while (w * c) % 4 and dword_rows:
        w += 1
    h = vrows + 1
    strips, row_tiles = math.ceil(w * c / vbytes), math.ceil(h / vrows)
    assert strips == 3 and row_tiles == 2
    assert (5 * ((strips + 1) // 2) * row_tiles) % 8
    return h, w


def _float_image(m, nw, c, steps):
    hl = (steps * c + 7) // 8
    vlanes, vrows = 64 - 2 * hl, m * nw - 2 * steps
    assert vlanes > 0 and vrows > 0
    w = 8 * vlanes // c + 1
    h = vrows + 1
    assert math.ceil(math.ceil(w * c / 8) / vlanes) == 2 and math.ceil(h / vrows) == 2
    return h, w, 8 * vlanes, vrows


def _five(W, H, vb, vrows, c, dword_rows):
    """The envelope itself; one pixel (both edge masks on it, above_own and
    below_own on one row); the first tile exactly (every other tile leaves
    early); one pixel and one row into the second strip and row tile; one row."""
    sizes = [(W, H), (1, 1), (vb, vrows), (vb + 1, vrows + 1), (W - 1, 1)]
    if dword_rows:  # the buffer-op kernel takes rows of whole dwords, per image

        def up(w):
            while (w * c) % 4:
                w += 1
            return min(w, W)

        sizes = [(up(w), h) for w, h in sizes]
    for w, h in sizes:
        assert 1 <= w <= W and 1 <= h <= H
    return sizes


def test_example_images_of_the_rule():
    # shape {4, 8, 8} at 8 steps, RGB: vbytes 208, vrows 48 -> envelope 139 x 49
    assert _swar_image(4, 8, 8, 3, 8, False) == (49, 139)
    assert _five(139, 49, 208 // 3, 48, 3, False) == [(139, 49), (1, 1), (69, 48), (70, 49), (138, 1)]
    assert _five(481, 49, 240, 48, 1, True)[1] == (4, 1) and _five(140, 49, 69, 48, 3, True)[1] == (4, 1)
    assert _five(97, 49, 48, 48, 4, True)[1] == (1, 1)


def _swar_cases(native, pconv_mod, shape, kernel, border, channels, steps_list, forms):
    lw, m, nw = shape
    native.set_swar_shape(lw, m, nw)
    native.set_prefetch_mode(1 if kernel == "bufop" else 0)
    bad, ran = [], 0
    for c in channels:
        for steps in steps_list:
            vbytes, vrows, ok = _swar_geom(lw, m, nw, c, steps)
            if not ok:
                continue
            H, W = _swar_image(lw, m, nw, c, steps, kernel == "bufop")
            sizes = _five(W, H, vbytes // c, vrows, c, kernel == "bufop")
            for form in forms:
                native.set_swar_alt(form)
                got = _launch_ragged(native, pconv_mod, "gaussian", "gaussian", c, H, W, steps, "temporal", border, sizes)
                bad += [g + (f"form {form}",) for g in got]
                ran += 1
    return bad, ran


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("kernel", ["tile", "bufop"])
def test_swar_five_images(native, pconv_mod, kernel, border):
    bad, ran = _swar_cases(native, pconv_mod, (4, 8, 8), kernel, border, (1, 3, 4), STEPS, (0, 1))
    assert ran == 24
    assert not bad, bad[:6]


def _float_filters(native):
    return [("box", "box", None), ("neg", NEG_TAPS, native.Filter.custom(NEG_TAPS[0], NEG_TAPS[1], "custom"))]


@pytest.mark.parametrize("border", BORDERS)
def test_float_five_images(native, pconv_mod, border):
    native.set_float_shape(8, 8)
    bad = []
    for c in (1, 3, 4):
        for steps in STEPS:
            H, W, vbytes, vrows = _float_image(8, 8, c, steps)
            sizes = _five(W, H, vbytes // c, vrows, c, False)
            for fkey, filt, nfilt in _float_filters(native):
                bad += _launch_ragged(native, pconv_mod, fkey, filt, c, H, W, steps, "float_temporal", border, sizes,
                                      nfilt=nfilt)
    assert not bad, bad[:6]


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("shape", [s for s in SWAR_SHAPES if s != (4, 8, 8)], ids=lambda s: "x".join(map(str, s)))
def test_other_swar_shapes(native, pconv_mod, shape, border):
    bad, ran = _swar_cases(native, pconv_mod, shape, "tile", border, (1, 3, 4), (3,), (1,))
    assert ran >= 1
    assert not bad, bad[:6]


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("shape", [s for s in PF_SHAPES if s != (4, 8, 8)], ids=lambda s: "x".join(map(str, s)))
def test_other_bufop_shapes(native, pconv_mod, shape, border):
    bad, ran = _swar_cases(native, pconv_mod, shape, "bufop", border, (1, 3, 4), (3,), (1,))
    assert ran == 3
    assert not bad, bad[:6]


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("shape", [s for s in FLOAT_SHAPES if s != (8, 8)], ids=lambda s: "x".join(map(str, s)))
def test_other_float_shapes(native, pconv_mod, shape, border):
    m, nw = shape
    native.set_float_shape(m, nw)
    bad = []
    for c in (1, 3, 4):
        H, W, vbytes, vrows = _float_image(m, nw, c, 3)
        sizes = _five(W, H, vbytes // c, vrows, c, False)
        bad += _launch_ragged(native, pconv_mod, "box", "box", c, H, W, 3, "float_temporal", border, sizes)
    assert not bad, bad[:6]


@pytest.mark.parametrize("kernel", ["tile", "bufop", "float"])
def test_batch_of_one_and_partial_batch(native, pconv_mod, kernel):
    native.set_swar_shape(4, 8, 8)
    native.set_float_shape(8, 4)
    native.set_prefetch_mode(1 if kernel == "bufop" else 0)
    variant, fkey = ("float_temporal", "box") if kernel == "float" else ("temporal", "gaussian")
    c, steps = 4, 8
    H, W = _swar_image(4, 8, 8, c, steps, True)
    bad = []
    for border in BORDERS:
        # batch = 1 with dims: one image smaller than its frame
        bad += _launch_ragged(native, pconv_mod, fkey, fkey, c, H, W, steps, variant, border, [(W - 5, H - 3)])
        # a partial batch: the frames beyond it keep the pattern
        bad += _launch_ragged(native, pconv_mod, fkey, fkey, c, H, W, steps, variant, border,
                              [(W, H), (7, 2)], capacity=4)
    assert not bad, bad[:6]


def test_auto_routes_a_one_step_dims_launch_to_the_temporal_kernels(native, pconv_mod):
    native.set_swar_shape(4, 8, 8)
    native.set_float_shape(8, 4)
    for fkey in ("gaussian", "box"):
        assert not _launch_ragged(native, pconv_mod, fkey, fkey, 3, 9, 21, 1, "auto", "zero", [(20, 9)])
        assert not _launch_ragged(native, pconv_mod, fkey, fkey, 3, 9, 21, 1, "auto", "zero", [(21, 9), (2, 3), (5, 1)])


# ---- the residual kernel ------------------------------------------------------


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("filt", ["gaussian", "box"])  # the int form and the float form
def test_residual_five_images(native, pconv_mod, filt, border):
    import torch

    R = native.RESIDUAL_BLOCK_ROWS
    for c in (1, 3, 4):
        W, H, halo = 1024 // c + 30, R + 8, 1  # 2 x 2 workgroups per image
        rb = W * c
        sizes = _five(W, H, 1024 // c, R, c, False)
        lay = native.frame_layout(rb, H, halo)
        pitch, fbytes = lay["pitch"], lay["bytes"]
        stride = fbytes + 48
        src_host = np.full((len(sizes), stride), JUNK, np.uint8)
        want = []
        for b, (w, h) in enumerate(sizes):
            img = _image(c, h, w)
            fr = src_host[b, :fbytes].reshape(H + 2 * halo, pitch)
            fr[halo:halo + h, 16:16 + w * c] = img.reshape(h, w * c)
            want.append(int(pconv_mod.numpy_residual(img, filt, border)))
        src = torch.from_numpy(src_host.reshape(-1)).cuda()
        counters = torch.tensor([5, 0, 7, 0, 11, 0xDEAD], dtype=torch.int64, device="cuda")  # ADDED to; [5] beyond
        host, dev = _dims_table(sizes, c)
        native.launch_residual_batch(filt, NAME[c], src.data_ptr() + pitch * halo + 16, pitch, rb, 0, H, -halo, H + halo,
                                     counters.data_ptr(), len(sizes), stride, 0, H,
                                     torch.cuda.current_stream().cuda_stream, border, dims=host, dims_ptr=dev.data_ptr())
        got = counters.cpu().numpy().tolist()
        assert got[5] == 0xDEAD
        assert [g - s for g, s in zip(got[:5], (5, 0, 7, 0, 11))] == want, (filt, border, c)
        assert np.array_equal(src.cpu().numpy(), src_host.reshape(-1))
        # one image (batch = 1) through the single-image entry point
        one_host, one_dev = _dims_table(sizes[3:4], c)
        n = native.launch_residual(filt, NAME[c], src.data_ptr() + 3 * stride + pitch * halo + 16, pitch, rb, 0, H, -halo,
                                   H + halo, 0, H, border=border, dims=one_host, dims_ptr=one_dev.data_ptr())
        assert int(n) == want[3]


# ---- guards -------------------------------------------------------------------


def test_guards(native):
    import torch

    c, h, w, steps = 3, 8, 16, 2
    rb = w * c
    lay = native.frame_layout(rb, h, steps)
    pitch, fbytes = lay["pitch"], lay["bytes"]
    src = torch.zeros(3 * fbytes, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(3 * fbytes, dtype=torch.uint8, device="cuda")
    base = pitch * steps + 16
    good = [(rb, h), (3, 1)]
    _, dev = _dims_table([(w, h), (1, 1)], c)

    def launch(variant="auto", filt="gaussian", st=steps, r0=0, r1=h, g_row0=0, **kw):
        kw.setdefault("batch", 2)
        kw.setdefault("batch_stride", fbytes)
        native.launch_stencil(filt, "rgb", src.data_ptr() + base, dst.data_ptr() + base, pitch, rb, r0, r1, -steps,
                              h + steps, st, g_row0, h, torch.cuda.current_stream().cuda_stream, variant, **kw)

    def resid(filt="gaussian", r0=0, r1=h, g_row0=0, **kw):
        cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
        native.launch_residual_batch(filt, "rgb", src.data_ptr() + base, pitch, rb, r0, r1, -steps, h + steps,
                                     cnt.data_ptr(), 2, fbytes, g_row0, h, **kw)

    both = dict(dims=good, dims_ptr=dev.data_ptr())
    for call in (lambda **kw: launch("auto", "gaussian", **kw), lambda **kw: launch("float_temporal", "box", **kw),
                 lambda **kw: resid("gaussian", **kw), lambda **kw: resid("box", **kw)):
        with pytest.raises(RuntimeError, match="dims and dims_host must be given together"):
            call(dims=good)
        with pytest.raises(RuntimeError, match="dims and dims_host must be given together"):
            call(dims_ptr=dev.data_ptr())
        with pytest.raises(RuntimeError, match="dims needs whole images"):
            call(r0=1, **both)
        with pytest.raises(RuntimeError, match="dims needs whole images"):
            call(r1=h - 1, **both)
        with pytest.raises(RuntimeError, match="dims needs whole images"):
            call(g_row0=1, **both)
        for bad_rb in (0, 2, 4, rb + 3):
            with pytest.raises(RuntimeError, match=r"dims\[1\].row_bytes .* is no whole number of pixels inside the envelope"):
                call(dims=[(rb, h), (bad_rb, 1)], dims_ptr=dev.data_ptr())
        for bad_h in (0, -1, h + 1):
            with pytest.raises(RuntimeError, match=r"dims\[0\].height .* is outside \[1, the envelope's 8\]"):
                call(dims=[(rb, bad_h), (3, 1)], dims_ptr=dev.data_ptr())
        with pytest.raises(RuntimeError, match="must hold `batch`"):
            call(dims=good[:1], dims_ptr=dev.data_ptr())
    # the single-step variants refuse dims by name
    for variant, filt in (("binomial", "gaussian"), ("int9", "gaussian"), ("float9", "box")):
        with pytest.raises(RuntimeError, match=f"dims not supported by kernel '{variant}'"):
            launch(variant, filt, st=1, batch=1, dims=good[:1], dims_ptr=dev.data_ptr())
    # forced buffer-op mode with an image row that is not whole dwords (the envelope's row is: 48 bytes)
    native.set_swar_shape(4, 8, 8)
    native.set_prefetch_mode(1)
    with pytest.raises(RuntimeError, match="whole dwords per row of every image"):
        launch("temporal", **both)
    launch("temporal", dims=[(rb, h), (12, 1)], dims_ptr=torch.tensor([[rb, h], [12, 1]], dtype=torch.int32,
                                                                   device="cuda").data_ptr())
    native.set_prefetch_mode(-1)
    torch.cuda.synchronize()
    # batch = 1 with dims is allowed, and a device table beyond the envelope is clamped by the kernel
    dst.zero_()
    wild = torch.tensor([[1 << 20, 1 << 20]], dtype=torch.int32, device="cuda")
    launch("temporal", batch=1, dims=[(rb, h)], dims_ptr=wild.data_ptr())
    torch.cuda.synchronize()
    assert int(dst[:fbytes].sum()) == 0 and int(dst[fbytes:].sum()) == 0  # zeros in, zeros out, nothing beyond


# ---- engine and API -----------------------------------------------------------


def _mixed(c, sizes, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size=(h, w, c) if c > 1 else (h, w), dtype=np.uint8) for w, h in sizes]


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("filt", ["gaussian", "box"])
def test_batch_engine_run_images(native, pconv_mod, filt, border):
    import torch

    native.set_swar_shape(4, 8, 8)
    native.set_float_shape(8, 4)
    c, W, H, cap, fuse, reps = 3, 77, 61, 5, 8, 40
    eng = pconv_mod.BatchEngine(W, H, "rgb", cap, filt, fuse=fuse, border=border)
    large = _mixed(c, [(77, 61), (70, 60), (77, 1), (1, 61), (64, 33)], 1)
    small = _mixed(c, [(5, 4), (1, 1), (33, 20), (2, 61)], 2)
    for imgs in (large, small):  # the smaller images land on the larger ones' stale bytes
        out = eng.run_images(imgs, reps)
        assert eng.stats.launches == math.ceil(reps / fuse)
        assert len(out) == len(imgs)
        for im, o in zip(imgs, out):
            assert isinstance(o, np.ndarray) and o.shape == im.shape
            assert np.array_equal(o, pconv_mod.numpy_convolve(im, reps, filt, border=border)), (filt, border, im.shape)
    # a plain uniform call after a mixed one
    stack = np.stack(_mixed(c, [(W, H)] * 3, 3))
    got = eng(stack, 11)
    for b in range(3):
        assert np.array_equal(got[b], pconv_mod.numpy_convolve(stack[b], 11, filt, border=border))
    # CUDA tensors in, CUDA tensors out
    dev = [torch.from_numpy(im).cuda() for im in small]
    out = eng.run_images(dev, 9)
    for im, o in zip(small, out):
        assert isinstance(o, torch.Tensor) and o.is_cuda and o.dtype == torch.uint8 and tuple(o.shape) == im.shape
        assert np.array_equal(o.cpu().numpy(), pconv_mod.numpy_convolve(im, 9, filt, border=border))
    with pytest.raises(ValueError, match="envelope"):
        eng.run_images([np.zeros((H + 1, 3, c), np.uint8)], 1)
    with pytest.raises(ValueError, match="capacity"):
        eng.run_images(small + small, 1)
    # the native engine insists on the uploaded count while the mode lasts
    eng.run_images(small, 1)
    with pytest.raises(RuntimeError, match="mixed-size upload holds 4"):
        eng._eng.run(1, 3)


@pytest.mark.parametrize("geom", rcp.GEOMS, ids=lambda g: f"{rcp.NAME[g[0]]}-{g[3]}")
def test_run_images_until_stable(native, pconv_mod, geom):
    native.set_swar_shape(4, 8, 8)
    native.set_float_shape(8, 4)
    c, h, w, filt = geom
    border = "replicate"
    stack = rcp.recipe(c, h, w)
    # the recipe's images cropped to differing sizes (image k loses k % 3 rows and k % 4 columns)
    imgs = [np.ascontiguousarray(stack[k][:h - k % 3, :w - k % 4]) for k in range(len(stack))]
    eng = pconv_mod.BatchEngine(w, h, rcp.NAME[c], len(imgs), filt, fuse=8, border=border)
    for max_reps, k in rcp.RUNS:
        outs, infos = eng.run_images_until_stable(imgs, max_reps, k)
        held = eng.residual_images()
        for b, im in enumerate(imgs):
            ro, ri = pconv_mod.convolve_until_stable(im, max_reps, filt, check_every=k, backend="numpy", border=border)
            assert np.array_equal(outs[b], ro) and infos[b] == ri, (geom, max_reps, b, infos[b], ri)
            assert int(held[b]) == ri.residual
    res = eng.residual_images(imgs)
    assert res.dtype == np.int64
    assert res.tolist() == [pconv_mod.numpy_residual(im, filt, border) for im in imgs]


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("filt", ["gaussian", "box"])
def test_convolve_many_hip(native, pconv_mod, filt, border):
    import torch

    native.set_swar_shape(4, 8, 8)
    native.set_float_shape(8, 4)
    c, reps = 3, 11
    sizes = [(45, 33), (44, 30), (40, 33), (45, 20), (9, 7), (8, 7), (9, 5), (1, 1), (45, 32), (3, 2), (7, 7)]
    imgs = _mixed(c, sizes, 4)
    from pconv.ops import stencil

    buckets = pconv_mod.size_buckets(sizes, "rgb", 8, batch_size=3)
    assert len(buckets) >= 4 and len(pconv_mod.size_buckets(sizes, "rgb", 8)) >= 2
    ref = [pconv_mod.convolve(im, reps, filt, backend="numpy", border=border) for im in imgs]
    kw = dict(reps=reps, filter=filt, backend="hip", border=border)
    for bs in (3, None):
        got = pconv_mod.convolve_many(imgs, batch_size=bs, **kw)
        assert len(got) == len(imgs)
        for g, r in zip(got, ref):
            assert isinstance(g, np.ndarray) and np.array_equal(g, r)
    dev = [torch.from_numpy(im).cuda() for im in imgs]
    got = pconv_mod.convolve_many(dev, reps, filt, border=border, batch_size=3)  # auto -> hip
    for g, r in zip(got, ref):
        assert g.is_cuda and np.array_equal(g.cpu().numpy(), r)
    res = pconv_mod.residual_many(imgs, filt, backend="hip", border=border)
    assert res.tolist() == [pconv_mod.numpy_residual(im, filt, border) for im in imgs]
    outs, infos = pconv_mod.convolve_many_until_stable(imgs[4:8], 24, filt, check_every=8, backend="hip", border=border)
    for im, o, info in zip(imgs[4:8], outs, infos):
        ro, ri = pconv_mod.convolve_until_stable(im, 24, filt, check_every=8, backend="numpy", border=border)
        assert np.array_equal(o, ro) and info == ri
    assert pconv_mod.convolve_many([], backend="hip") == []
    assert len(stencil._BATCH_ENGINES) <= 2
