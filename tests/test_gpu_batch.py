"""Image batches on a real MI355X: B same-size images advance in one fused
launch of the SWAR tile kernel, the buffer-op tile kernel and the float
temporal kernel (StencilLaunch batch / batch_stride), then the BatchEngine,
``convolve_batch(backend="hip")`` and ``conv --frames``.

Kernel level: B frames lie at stride S in one allocation between canaries.
Every launch is compared BYTE FOR BYTE with the expected destination
allocation — each image's rows are the NumPy oracle of that image alone, and
everything else (pad columns, ghost rows, the gaps between frames, the frames
a partial batch leaves out) is what it was — and the source must be unmodified.
Image contents differ per image; image 0 is all 255 and image 1 all 0 (which
stays all 0: images never read each other's rows).

Shapes are forced and tuning is off: no case spends time tuning."""
import json
import math
import subprocess

import numpy as np
import pytest

from conftest import CONV_BIN

pytestmark = pytest.mark.gpu

GUARD = 4096
CANARY = 0xA5
UNTOUCHED = 0x5A
NAME = {1: "grey", 3: "rgb", 4: "rgba"}
NEG_TAPS = ([3, 1, 0, 2, 5, 1, -1, 2, 4], 17)  # the negative-tap custom filter of test_gpu_kernels.py
BORDERS = ["zero", "replicate"]
STEPS = (1, 3, 8, 16)

# hard-coded copies of the shape tables (tests/test_shape_tables.py pins them):
# parametrize needs them at collection time, before a device is touched
SWAR_SHAPES = [(8, 8, 8), (8, 8, 4), (8, 16, 4), (8, 4, 8), (4, 8, 8), (4, 6, 8), (4, 5, 8), (4, 4, 8), (4, 3, 8),
               (4, 4, 16), (4, 2, 16), (4, 3, 16), (8, 2, 16), (8, 4, 16), (4, 16, 4), (4, 12, 4), (4, 16, 8),
               (4, 12, 8), (4, 20, 8)]
PF_SHAPES = [(4, 8, 8), (4, 16, 4), (4, 12, 4), (4, 16, 8), (4, 12, 8), (4, 20, 8)]
FLOAT_SHAPES = [(16, 8), (16, 4), (8, 8), (8, 4), (4, 8)]

_IMGS = {}  # (c, h, w) -> the 5 images of that geometry
_REF = {}   # (filter key, border, c, h, w, steps) -> their oracles


def test_shape_lists_are_the_native_tables(native):
    assert [tuple(s) for s in native.swar_shapes()] == SWAR_SHAPES
    assert sorted(tuple(s) for s in native.swar_prefetch_shapes()) == sorted(PF_SHAPES)
    assert [tuple(s) for s in native.float_shapes()] == FLOAT_SHAPES


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


def _images(c, h, w, n=5):
    key = (c, h, w)
    if key not in _IMGS:
        rng = np.random.default_rng(7919 * c + 104729 * h + w)
        shape = (h, w, c) if c > 1 else (h, w)
        imgs = [np.full(shape, 255, np.uint8), np.zeros(shape, np.uint8)]
        imgs += [rng.integers(0, 256, size=shape, dtype=np.uint8) for _ in range(3)]
        _IMGS[key] = imgs
    return _IMGS[key][:n]


def _oracles(pconv_mod, fkey, filt, border, c, h, w, steps, n):
    key = (fkey, border, c, h, w, steps)
    if key not in _REF:
        _REF[key] = [pconv_mod.numpy_convolve(im, steps, filt, border=border) for im in _images(c, h, w)]
    return _REF[key][:n]


def _launch_batch(native, pconv_mod, fkey, filt, c, h, w, steps, variant, border, batch, capacity=None, gap=48,
                  nfilt=None):
    """`batch` images of (c, h, w) in one launch, in allocations of `capacity`
    frames; returns the list of mismatches (empty: all as expected)."""
    import torch

    capacity = batch if capacity is None else capacity
    rb, halo = w * c, steps
    lay = native.frame_layout(rb, h, halo)
    pitch, fbytes = lay["pitch"], lay["bytes"]
    stride = fbytes + gap  # a multiple of 16 with a gap between the frames
    imgs = _images(c, h, w, capacity)
    refs = _oracles(pconv_mod, fkey, filt, border, c, h, w, steps, capacity)
    src_host = np.zeros((capacity, stride), np.uint8)
    exp_host = np.zeros((capacity, stride), np.uint8)
    for b in range(capacity):
        fr = src_host[b, :fbytes].reshape(h + 2 * halo, pitch)
        fr[halo:halo + h, 16:16 + rb] = imgs[b].reshape(h, rb)
        if b < batch:
            ex = exp_host[b, :fbytes].reshape(h + 2 * halo, pitch)
            ex[halo:halo + h, 16:16 + rb] = refs[b].reshape(h, rb)
        else:
            exp_host[b] = UNTOUCHED  # a partial batch leaves these frames as they were
    total = capacity * stride
    src = torch.full((total + 2 * GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    dst = torch.full((total + 2 * GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    src[GUARD:GUARD + total] = torch.from_numpy(src_host.reshape(-1)).cuda()
    dst[GUARD:GUARD + total] = 0
    if capacity > batch:
        dst[GUARD + batch * stride:GUARD + total] = UNTOUCHED
    base = GUARD + pitch * halo + 16
    native.launch_stencil(filt if nfilt is None else nfilt, NAME[c], src.data_ptr() + base, dst.data_ptr() + base, pitch,
                          rb, 0, h, -halo, h + halo, steps, 0, h, torch.cuda.current_stream().cuda_stream, variant,
                          border=border, batch=batch, batch_stride=stride)
    torch.cuda.synchronize()
    d = dst.cpu().numpy()
    case = (fkey, variant, border, c, h, w, steps, batch, capacity)
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


# ---- the geometry formulas of swar_geom / ft_geom -------------------------


def _swar_geom(lw, m, nw, c, steps):
    hl = (steps * c + lw - 1) // lw
    vbytes, vrows = (64 - 2 * hl) * lw, m * nw - 2 * steps
    return vbytes, vrows, vbytes > 0 and vrows > 0 and lw >= c


def _swar_image(lw, m, nw, c, steps, dword_rows):
    """The smallest image with 3 strips (an odd count: the last pair has no B
    strip) and 2 row tiles: 4 tiles per image, so 3 and 5 images give 12 and
    20 workgroups, no multiple of 8 (the XCD remap takes its remainder path)."""
    vbytes, vrows, ok = _swar_geom(lw, m, nw, c, steps)
    assert ok
    w = 2 * vbytes // c + 1
    while (w * c) % 4 and dword_rows:  # the buffer-op kernel takes rows of whole dwords
        w += 1
    h = vrows + 1
    strips, row_tiles = math.ceil(w * c / vbytes), math.ceil(h / vrows)
    assert strips == 3 and row_tiles == 2
    tiles = ((strips + 1) // 2) * row_tiles
    assert (3 * tiles) % 8 and (5 * tiles) % 8
    return h, w


def test_example_geometries_of_the_rule():
    # shape {4, 8, 8} at 8 steps: vbytes 240 / 208 / 192 and vrows 48 (grey / RGB / RGBA)
    assert [_swar_geom(4, 8, 8, c, 8)[:2] for c in (1, 3, 4)] == [(240, 48), (208, 48), (192, 48)]
    assert _swar_image(4, 8, 8, 1, 8, False) == (49, 481)
    assert _swar_image(4, 8, 8, 3, 8, False) == (49, 139)
    assert _swar_image(4, 8, 8, 4, 8, True) == (49, 97)


def _grid_mapping(native, pconv_mod, shape, kernel, border):
    lw, m, nw = shape
    native.set_swar_shape(lw, m, nw)
    native.set_prefetch_mode(1 if kernel == "bufop" else 0)
    bad, ran = [], 0
    for c in (1, 3, 4):
        for steps in STEPS:
            if not _swar_geom(lw, m, nw, c, steps)[2]:
                continue
            h, w = _swar_image(lw, m, nw, c, steps, kernel == "bufop")
            for form in (0, 1):
                native.set_swar_alt(form)
                for swizzle in (True, False):
                    native.set_xcd_swizzle(swizzle)
                    for batch in (3, 5):
                        got = _launch_batch(native, pconv_mod, "gaussian", "gaussian", c, h, w, steps, "temporal",
                                            border, batch)
                        bad += [g + (f"form {form} swizzle {swizzle}",) for g in got]
                        ran += 1
    assert ran >= 8
    assert not bad, bad[:6]


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("shape", SWAR_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_swar_grid_mapping(native, pconv_mod, shape, border):
    _grid_mapping(native, pconv_mod, shape, "tile", border)


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("shape", PF_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bufop_grid_mapping(native, pconv_mod, shape, border):
    _grid_mapping(native, pconv_mod, shape, "bufop", border)


def _float_filters(native):
    return [("box", "box", None), ("edge", "edge", None),
            ("neg", NEG_TAPS, native.Filter.custom(NEG_TAPS[0], NEG_TAPS[1], "custom"))]


def _float_image(m, nw, c, steps):
    """>= 2 column tiles and >= 2 row tiles of the float kernel's tile."""
    hl = (steps * c + 7) // 8
    vlanes, vrows = 64 - 2 * hl, m * nw - 2 * steps
    assert vlanes > 0 and vrows > 0
    w = 8 * vlanes // c + 1
    h = vrows + 1
    assert math.ceil(math.ceil(w * c / 8) / vlanes) == 2 and math.ceil(h / vrows) == 2
    return h, w


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("shape", FLOAT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_float_grid_mapping(native, pconv_mod, shape, border):
    m, nw = shape
    native.set_float_shape(m, nw)
    bad = []
    for c in (1, 3):
        for steps in (1, 4):
            h, w = _float_image(m, nw, c, steps)
            for fkey, filt, nfilt in _float_filters(native):
                bad += _launch_batch(native, pconv_mod, fkey, filt, c, h, w, steps, "float_temporal", border, 3,
                                     nfilt=nfilt)
    assert not bad, bad[:6]


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("kernel", ["tile", "bufop", "float"])
def test_one_and_two_pixel_images(native, pconv_mod, kernel, border):
    native.set_swar_shape(4, 8, 8)
    native.set_float_shape(8, 4)
    native.set_prefetch_mode(1 if kernel == "bufop" else 0)
    bad = []
    # the buffer-op kernel takes rows of whole dwords: its one- and two-pixel rows are RGBA
    for c in ((4,) if kernel == "bufop" else (1, 3, 4)):
        for h in (1, 2):
            for w in (1, 2):
                for steps in (1, 8):
                    if kernel == "float":
                        bad += _launch_batch(native, pconv_mod, "box", "box", c, h, w, steps, "float_temporal", border,
                                             3)
                    else:
                        bad += _launch_batch(native, pconv_mod, "gaussian", "gaussian", c, h, w, steps, "temporal",
                                             border, 3)
    assert not bad, bad[:6]


@pytest.mark.parametrize("kernel", ["tile", "bufop", "float"])
def test_partial_batch_leaves_the_other_frames_alone(native, pconv_mod, kernel):
    native.set_swar_shape(4, 8, 8)
    native.set_float_shape(8, 4)
    native.set_prefetch_mode(1 if kernel == "bufop" else 0)
    h, w = _swar_image(4, 8, 8, 4, 8, True)
    variant, fkey = ("float_temporal", "box") if kernel == "float" else ("temporal", "gaussian")
    assert not _launch_batch(native, pconv_mod, fkey, fkey, 4, h, w, 8, variant, "zero", batch=2, capacity=4)


def test_auto_routes_a_one_step_batch_to_the_temporal_kernels(native, pconv_mod):
    native.set_swar_shape(4, 8, 8)
    native.set_float_shape(8, 4)
    for fkey in ("gaussian", "box"):
        assert not _launch_batch(native, pconv_mod, fkey, fkey, 3, 9, 21, 1, "auto", "zero", 3)


@pytest.mark.parametrize("kernel", ["tile", "bufop", "float"])
def test_stride_beyond_32_bits(native, pconv_mod, kernel):
    """Two 16x8 grey frames 2^32 + 4096 bytes apart inside two untouched
    allocations: only the two frames (and a canary ring around each) are ever
    written or read."""
    import torch

    native.set_swar_shape(4, 8, 8)
    native.set_float_shape(8, 4)
    native.set_prefetch_mode(1 if kernel == "bufop" else 0)
    variant, fkey = ("float_temporal", "box") if kernel == "float" else ("temporal", "gaussian")
    c, h, w, steps = 1, 8, 16, 8
    stride = (1 << 32) + 4096
    lay = native.frame_layout(w, h, steps)
    pitch, fbytes = lay["pitch"], lay["bytes"]
    assert fbytes + 2 * GUARD < (2 << 20)
    imgs = _images(c, h, w)[2:4]  # two random images
    refs = _oracles(pconv_mod, fkey, fkey, "zero", c, h, w, steps, 5)[2:4]
    src = torch.empty(stride + (2 << 20), dtype=torch.uint8, device="cuda")
    dst = torch.empty(stride + (2 << 20), dtype=torch.uint8, device="cuda")
    frames, exps = [], []
    for b in range(2):
        fr = np.zeros((h + 2 * steps, pitch), np.uint8)
        fr[steps:steps + h, 16:16 + w] = imgs[b]
        ex = np.zeros_like(fr)
        ex[steps:steps + h, 16:16 + w] = refs[b]
        frames.append(fr)
        exps.append(ex)
        lo = b * stride  # [canary | frame | canary]
        for t, body in ((src, torch.from_numpy(fr.reshape(-1)).cuda()), (dst, None)):
            t[lo:lo + GUARD] = CANARY
            t[lo + GUARD + fbytes:lo + 2 * GUARD + fbytes] = CANARY
            if body is None:
                t[lo + GUARD:lo + GUARD + fbytes] = 0
            else:
                t[lo + GUARD:lo + GUARD + fbytes] = body
    base = GUARD + pitch * steps + 16
    native.launch_stencil(fkey, NAME[c], src.data_ptr() + base, dst.data_ptr() + base, pitch, w, 0, h, -steps, h + steps,
                          steps, 0, h, torch.cuda.current_stream().cuda_stream, variant, batch=2, batch_stride=stride)
    torch.cuda.synchronize()
    for b in range(2):
        lo = b * stride
        for t, want in ((dst, exps[b]), (src, frames[b])):
            blk = t[lo:lo + 2 * GUARD + fbytes].cpu().numpy()
            assert (blk[:GUARD] == CANARY).all() and (blk[-GUARD:] == CANARY).all(), (kernel, b, "canary")
            assert np.array_equal(blk[GUARD:-GUARD], want.reshape(-1)), (kernel, b)
    del src, dst
    torch.cuda.empty_cache()


def test_guards(native):
    import torch

    c, h, w, steps = 1, 8, 16, 2
    lay = native.frame_layout(w, h, steps)
    pitch, fbytes = lay["pitch"], lay["bytes"]
    src = torch.zeros(3 * fbytes, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(3 * fbytes, dtype=torch.uint8, device="cuda")
    base = pitch * steps + 16

    def launch(variant="auto", filt="gaussian", st=steps, **kw):
        native.launch_stencil(filt, "grey", src.data_ptr() + base, dst.data_ptr() + base, pitch, w, 0, h, -steps,
                              h + steps, st, 0, h, torch.cuda.current_stream().cuda_stream, variant, **kw)

    for variant, filt in (("auto", "gaussian"), ("float_temporal", "box")):
        with pytest.raises(RuntimeError, match="batch must be >= 1"):
            launch(variant, filt, batch=0, batch_stride=fbytes)
        with pytest.raises(RuntimeError, match="smaller than a frame"):
            launch(variant, filt, batch=2, batch_stride=fbytes - 16)
        with pytest.raises(RuntimeError, match="multiple of 16"):
            launch(variant, filt, batch=2, batch_stride=fbytes + 8)
    with pytest.raises(RuntimeError, match="exceeds grid.z"):
        launch("float_temporal", "box", batch=65536, batch_stride=fbytes)
    for variant, filt in (("binomial", "gaussian"), ("int9", "gaussian"), ("float9", "box")):
        with pytest.raises(RuntimeError, match=f"batch not supported by kernel '{variant}'"):
            launch(variant, filt, st=1, batch=2, batch_stride=fbytes)
    # the residual launch is one image's: it takes no batch at all
    with pytest.raises(TypeError):
        native.launch_residual("gaussian", "grey", src.data_ptr() + base, pitch, w, 0, h, -steps, h + steps, 0, h,
                               batch=2)
    torch.cuda.synchronize()
    assert int(dst.sum()) == 0  # no refused launch wrote anything
    # batch = 1 ignores the stride, as before
    launch(batch=1, batch_stride=7)
    torch.cuda.synchronize()


# ---- engine and API ---------------------------------------------------


@pytest.mark.parametrize("filt", ["gaussian", "box"])
def test_batch_engine(native, pconv_mod, filt):
    native.set_swar_shape(4, 8, 8)
    native.set_float_shape(8, 4)
    c, h, w, cap, fuse = 3, 61, 77, 4, 8
    stack = np.stack(_images(c, h, w, cap))
    eng = native.BatchEngine(w, h, "rgb", cap, filt, fuse=fuse)
    assert eng.capacity == cap and eng.fuse == fuse and eng.halo == fuse
    assert eng.batch_stride % eng.pitch == 0 and eng.batch_stride >= (h + 2 * fuse) * eng.pitch
    for reps in (1, 8, 20):  # 1, 1 and 3 launches: both end parities
        for n in (cap, 3):
            out = np.full_like(stack[:n], 0x77)
            eng.upload(stack[:n].reshape(-1), n)
            eng.run(reps, n)
            eng.download(out.reshape(-1), n)
            eng.synchronize()
            assert eng.stats.launches == math.ceil(reps / fuse), (reps, n)
            for b in range(n):
                ref = pconv_mod.numpy_convolve(stack[b], reps, filt)
                assert np.array_equal(out[b], ref), (filt, reps, n, b)
    with pytest.raises(RuntimeError, match="capacity"):
        eng.run(1, cap + 1)
    with pytest.raises(RuntimeError, match="batch not supported by kernel 'binomial'"):
        native.BatchEngine(w, h, "rgb", cap, "gaussian", fuse=1, variant="binomial")


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("filt", ["gaussian", "box"])
def test_convolve_batch_hip(native, pconv_mod, filt, border):
    import torch

    native.set_swar_shape(4, 8, 8)
    native.set_float_shape(8, 4)
    c, h, w, n, reps = 3, 33, 45, 7, 11
    rng = np.random.default_rng(99)
    stack = rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8)
    ref = np.stack([pconv_mod.convolve(stack[i], reps, filt, backend="numpy", border=border) for i in range(n)])
    kw = dict(reps=reps, filter=filt, backend="hip", border=border)
    # chunks of 3, 3 and 1 on one cached engine
    got = pconv_mod.convolve_batch(stack, batch_size=3, **kw)
    assert isinstance(got, np.ndarray) and np.array_equal(got, ref)
    # the default batch size takes all 7 at once
    assert np.array_equal(pconv_mod.convolve_batch(stack, **kw), ref)
    assert np.array_equal(pconv_mod.convolve_batch([stack[i] for i in range(n)], **kw), ref)
    got = pconv_mod.convolve_batch(torch.from_numpy(stack), batch_size=3, **kw)
    assert isinstance(got, torch.Tensor) and not got.is_cuda and np.array_equal(got.numpy(), ref)
    dev = torch.from_numpy(stack).cuda()
    got = pconv_mod.convolve_batch(dev, batch_size=3, **kw)
    assert isinstance(got, torch.Tensor) and got.device == dev.device and got.dtype == torch.uint8
    assert np.array_equal(got.cpu().numpy(), ref)
    # a non-contiguous CUDA view: every other image of a longer stack, grey
    wide = torch.from_numpy(np.ascontiguousarray(np.repeat(stack[..., 0], 2, axis=0))).cuda()
    view = wide[::2]
    assert not view.is_contiguous()
    got = pconv_mod.convolve_batch(view, backend="auto", reps=reps, filter=filt, border=border, batch_size=3)
    refg = np.stack([pconv_mod.convolve(stack[i, ..., 0], reps, filt, backend="numpy", border=border)
                     for i in range(n)])
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), refg)
    # an empty batch
    empty = pconv_mod.convolve_batch(dev[:0], **kw)
    assert empty.is_cuda and tuple(empty.shape) == (0, h, w, c)
    from pconv.ops import stencil

    assert len(stencil._BATCH_ENGINES) <= 2


def test_cli_frames_hip(pconv_mod, tmp_path):
    r = subprocess.run([CONV_BIN, "s.raw", "77", "61", "20", "rgb", "--synthetic", "3", "--frames", "4", "--check",
                        "--json", "--quiet", "--out", "out.raw"], cwd=tmp_path, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    js = json.loads(r.stdout.strip().splitlines()[-1])
    assert js["frames"] == 4 and js["mismatches"] == 0 and js["backend"] == "hip"
    assert js["launches"] == math.ceil(20 / js["fuse"])
    out = np.fromfile(tmp_path / "out.raw", dtype=np.uint8).reshape(4, 61, 77, 3)
    for k in range(4):
        src = pconv_mod.synthetic_image(77, 61, "rgb", seed=3 + k)
        assert np.array_equal(out[k], pconv_mod.numpy_convolve(src, 20, "gaussian")), k
