"""Depth 16 on a real MI355X: the 16-bit temporal kernel (k_swar16) through the
raw launch on canary-guarded frames, every row of swar16_shapes() forced, both
step forms, band frames, image sets (batch, active table, dims table), the
launch guards, the public API and the CLI.

Reference: cpu_fused_launch(depth=16) on the same frame (its sanitized twin
test is tests/cpp/test_depth16_native.cpp), NumPy for lone images.  The source
and destination allocations are filled with a canary byte — pads, ghost rows,
gaps and guard bands included — and the destination is compared BYTE FOR BYTE
with the expected allocation: what a launch may write holds the reference,
everything else is still the canary.

Sizes come from the shape under test, not from a workload: with hl =
ceil(steps C / NP) halo lanes, vs = (64 - 2 hl) NP valid samples per strip and
vrows = M NW - 2 steps valid rows per tile, widths and heights sit at one
pixel, on either side of a tile edge and at two tiles plus a rest."""
import json
import math
import subprocess

import numpy as np
import pytest

from conftest import CONV_BIN

pytestmark = pytest.mark.gpu

GUARD = 4096
CANARY = 0xA5
NAME = {1: "grey", 3: "rgb", 4: "rgba"}
BORDERS = ["zero", "replicate"]
STEPS = (1, 2, 3, 8, 16)
# a copy of the kernel's table (test_shape_table_is_the_documented_one pins it)
SHAPES = [(8, 8, 8), (4, 16, 4), (4, 8, 8), (4, 4, 8), (4, 2, 16)]


@pytest.fixture(autouse=True)
def forced(native):
    prev = native.set_autotune(False)
    yield
    native.set_swar16_shape(0, 0, 0)
    native.set_swar_alt(-1)
    native.set_autotune(prev)


def _values(rng, h, n):
    """(h, n) uint16 samples: full-range random with planted blocks of 65535,
    a 0 / 65535 checkerboard and the 0x00FF / 0xFF00 byte-order pattern."""
    a = rng.integers(0, 65536, size=(h, n), dtype=np.uint16)
    a[h // 5:h // 5 + 4, n // 7:n // 7 + 9] = 65535
    yy, xx = np.mgrid[0:h, 0:n]
    cb = (((yy + xx) & 1) * 65535).astype(np.uint16)
    a[h // 2:h // 2 + 3, :n // 2] = cb[h // 2:h // 2 + 3, :n // 2]
    bo = np.where(xx & 1, 0xFF00, 0x00FF).astype(np.uint16)
    a[(3 * h) // 4:(3 * h) // 4 + 2, n // 3:] = bo[(3 * h) // 4:(3 * h) // 4 + 2, n // 3:]
    return a


def _shape_geom(shape, c, steps):
    np_, m, nw = shape
    hl = -(-steps * c // np_)
    return (64 - 2 * hl) * np_, m * nw - 2 * steps  # vs, vrows


def _alloc(torch, frames_u8):
    """A canary-guarded device copy of `frames_u8` (any shape, uint8)."""
    n = frames_u8.size
    buf = torch.full((n + 2 * GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    buf[GUARD:GUARD + n] = torch.from_numpy(np.ascontiguousarray(frames_u8).reshape(-1)).cuda()
    return buf


def _launch(native, src_frames, lay, halo, c, r0, r1, steps, g_row0, height, border, variant="temporal", **kw):
    """One depth-16 launch.  src_frames: (F, rows + 2 halo, pitch) uint8, the
    frames one after the other (stride = a frame).  Returns the destination
    allocation's frames in the same shape; the guard bands are checked here and
    the source must come back unmodified."""
    import torch

    src = _alloc(torch, src_frames)
    dst = _alloc(torch, np.full(src_frames.shape, CANARY, np.uint8))
    base = GUARD + lay["pitch"] * halo + 16
    rows = src_frames.shape[1] - 2 * halo
    native.launch_stencil("gaussian", NAME[c], src.data_ptr() + base, dst.data_ptr() + base, lay["pitch"],
                          lay["row_bytes"], r0, r1, -halo, rows + halo, steps, g_row0, height,
                          torch.cuda.current_stream().cuda_stream, variant, border=border, depth=16, **kw)
    torch.cuda.synchronize()
    d = dst.cpu().numpy()
    assert (d[:GUARD] == CANARY).all() and (d[-GUARD:] == CANARY).all(), "write outside the allocation"
    assert np.array_equal(src.cpu().numpy()[GUARD:-GUARD], src_frames.reshape(-1)), "the source was modified"
    return d[GUARD:-GUARD].reshape(src_frames.shape)


def _cpu_frame(native, clean, lay, halo, c, r0, r1, steps, g_row0, height, border):
    """cpu_fused_launch(depth=16) on one clean frame ((rows + 2 halo, pitch)
    uint8, zeros outside the image); the destination frame, zero-initialised."""
    rows = clean.shape[0] - 2 * halo
    out = np.zeros_like(clean)
    native.cpu_fused_launch("gaussian", NAME[c], lay["row_bytes"], rows, halo, clean.reshape(-1), out.reshape(-1),
                            r0, r1, steps, g_row0, height, border=border, depth=16)
    return out


def _whole_image_case(native, rng, c, h, w, steps, border):
    """The whole h x w image in one launch: (mismatch description or None)."""
    rb = w * c * 2
    halo = steps
    lay = native.frame_layout(rb, h, halo)
    img = _values(rng, h, w * c)
    clean = np.zeros((h + 2 * halo, lay["pitch"]), np.uint8)
    clean[halo:halo + h, 16:16 + rb] = img.view(np.uint8).reshape(h, rb)
    dirty = clean.copy()
    dirty[:halo, :] = 0xFF  # ghost rows beyond the image and every pad column: garbage
    dirty[halo + h:, :] = 0xFF
    dirty[:, :16] = 0xFF
    dirty[:, 16 + rb:] = 0xFF
    got = _launch(native, dirty[None], lay, halo, c, 0, h, steps, 0, h, border)[0]
    want = np.full_like(clean, CANARY)
    want[halo:halo + h, 16:16 + rb] = _cpu_frame(native, clean, lay, halo, c, 0, h, steps, 0, h,
                                                 border)[halo:halo + h, 16:16 + rb]
    if np.array_equal(got, want):
        return None
    bad = np.argwhere(got != want)
    return (h, w, steps, border, len(bad), bad[:3].tolist())


def test_shape_table_is_the_documented_one(native):
    assert [tuple(s) for s in native.swar16_shapes()] == SHAPES
    assert len(SHAPES) <= 6
    with pytest.raises(RuntimeError, match="not instantiated"):
        native.set_swar16_shape(4, 5, 8)


@pytest.mark.parametrize("channels", [1, 3, 4])
@pytest.mark.parametrize("shape", SHAPES)
def test_every_shape_both_forms_around_tile_edges(native, shape, channels):
    """Each row of swar16_shapes() forced, x both step forms x both borders x
    steps, on sizes derived from the shape: the one-pixel image, widths and
    heights on either side of a tile edge, and the two-tile case."""
    c = channels
    native.set_swar16_shape(*shape)
    rng = np.random.default_rng(1000 * shape[0] + 100 * shape[1] + 10 * shape[2] + c)
    bad, ran = [], 0
    for steps in STEPS:
        vs, vrows = _shape_geom(shape, c, steps)
        if vs <= 0 or vrows <= 0:
            continue  # the shape does not allow this step count
        wpx = -(-vs // c)
        widths = [1, 2, 5, wpx - 1, wpx + 1, 2 * wpx + 3]
        heights = [1, 2, 3, vrows - 1, vrows + 1, 2 * vrows + 3]
        # one pixel; small; each side of the tile edge in x and in y; two tiles both ways
        sizes = [(heights[0], widths[0]), (heights[1], widths[2]), (heights[2], widths[1]),
                 (heights[3], widths[3]), (heights[4], widths[4]), (heights[3], widths[4]),
                 (heights[5], widths[5])]
        sizes = [(h, w) for h, w in dict.fromkeys(sizes) if h >= 1 and w >= 1]
        for k, (h, w) in enumerate(sizes):
            for form in (0, 1):
                native.set_swar_alt(form)
                # both borders on every size, alternating which form sees which first
                for border in BORDERS:
                    if steps >= 8 and k in (1, 2) and border == BORDERS[form]:
                        continue  # the small sizes at deep fusion: one border per form
                    r = _whole_image_case(native, rng, c, h, w, steps, border)
                    ran += 1
                    if r:
                        bad.append((form,) + r)
    assert ran > 0
    assert not bad, bad[:8]


@pytest.mark.parametrize("steps", [1, 3, 8])
@pytest.mark.parametrize("border", BORDERS)
def test_band_frames(native, border, steps):
    """Band frames of a taller image: g_row0 != 0, frames whose owned rows reach
    past the image, partial [r0, r1), ghost rows beyond the image holding
    garbage."""
    H, h, w, c, halo = 100, 30, 45, 3, 8
    rb = w * c * 2
    lay = native.frame_layout(rb, h, halo)
    rng = np.random.default_rng(31 * steps + len(border))
    for shape in ((4, 4, 8), (8, 8, 8)):
        native.set_swar16_shape(*shape)
        for g_row0 in (0, 35, H - h, -3, H - h + 4):
            clean = np.zeros((h + 2 * halo, lay["pitch"]), np.uint8)
            dirty = np.full_like(clean, 0xEE)
            for fr in range(-halo, h + halo):
                if 0 <= g_row0 + fr < H:
                    row = _values(rng, 1, w * c).view(np.uint8).reshape(-1)
                    clean[halo + fr, 16:16 + rb] = row
                    dirty[halo + fr, 16:16 + rb] = row
            for (r0, r1) in [(0, h), (-(halo - steps), h + (halo - steps)), (steps, h - steps), (-3, 5),
                             (h - 2, h + 1), (7, 8)]:
                if r0 - steps < -halo or r1 + steps > h + halo or r0 >= r1:
                    continue
                got = _launch(native, dirty[None], lay, halo, c, r0, r1, steps, g_row0, H, border)[0]
                cpu = _cpu_frame(native, clean, lay, halo, c, r0, r1, steps, g_row0, H, border)
                lo, hi = max(r0, -g_row0), min(r1, H - g_row0)
                want = np.full_like(clean, CANARY)
                if lo < hi:
                    want[halo + lo:halo + hi, 16:16 + rb] = cpu[halo + lo:halo + hi, 16:16 + rb]
                assert np.array_equal(got, want), (shape, g_row0, r0, r1)


def _image_set_frames(native, rng, c, H, W, steps, sizes):
    """Frames of one H x W envelope, image k of `sizes` [(h, w)] top-left in
    frame k, stale 0xFF right of and below it: (lay, dirty frames, images)."""
    rb = W * c * 2
    lay = native.frame_layout(rb, H, steps)
    frames = np.full((len(sizes), H + 2 * steps, lay["pitch"]), 0xFF, np.uint8)
    imgs = []
    for k, (h, w) in enumerate(sizes):
        img = _values(rng, h, w * c)
        imgs.append(img)
        frames[k, steps:steps + h, 16:16 + w * c * 2] = img.view(np.uint8).reshape(h, w * c * 2)
    return lay, frames, imgs


def _lone(pconv_mod, img, c, steps, border):
    h = img.shape[0]
    x = img.reshape(h, -1, c) if c > 1 else img
    return pconv_mod.numpy_convolve(x, steps, "gaussian", border).reshape(h, -1)


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("channels", [1, 3])
def test_image_sets(native, pconv_mod, channels, border):
    """A 5-frame batch; an active table {0, 2, 4} with the unnamed frames
    untouched; a dims table with a one-pixel image, the envelope and sizes
    straddling vs / vrows, stale 0xFF right of and below each image.  Each image
    equals a lone run."""
    import torch

    c, steps, shape = channels, 3, (4, 4, 8)
    native.set_swar16_shape(*shape)
    vs, vrows = _shape_geom(shape, c, steps)
    wpx = -(-vs // c)
    H, W = 2 * vrows + 3, wpx + 9
    rng = np.random.default_rng(77 + c)
    # --- batch of 5 same-size images -----------------------------------
    lay, frames, imgs = _image_set_frames(native, rng, c, H, W, steps, [(H, W)] * 5)
    stride = frames[0].size
    rb = lay["row_bytes"]

    def expect(active, sizes):
        want = np.full_like(frames, CANARY)
        for k in active:
            h, w = sizes[k]
            want[k, steps:steps + h, 16:16 + w * c * 2] = _lone(pconv_mod, imgs[k], c, steps,
                                                                border).view(np.uint8).reshape(h, w * c * 2)
        return want

    got = _launch(native, frames, lay, steps, c, 0, H, steps, 0, H, border, batch=5, batch_stride=stride)
    assert np.array_equal(got, expect(range(5), [(H, W)] * 5)), "batch"
    # --- active table {0, 2, 4} ------------------------------------------
    act = torch.tensor([0, 2, 4], dtype=torch.int32, device="cuda")
    got = _launch(native, frames, lay, steps, c, 0, H, steps, 0, H, border, batch=3, batch_stride=stride,
                  active=[0, 2, 4], active_ptr=act.data_ptr(), batch_frames=5)
    assert np.array_equal(got, expect([0, 2, 4], [(H, W)] * 5)), "active"
    # --- dims table ---------------------------------------------------------
    sizes = [(1, 1), (H, W), (vrows - 1, wpx - 1), (vrows + 1, wpx + 1), (vrows, wpx)]
    lay, frames, imgs = _image_set_frames(native, rng, c, H, W, steps, sizes)
    dims = [(w * c * 2, h) for h, w in sizes]
    dev = torch.tensor(dims, dtype=torch.int32, device="cuda")
    got = _launch(native, frames, lay, steps, c, 0, H, steps, 0, H, border, batch=5, batch_stride=stride, dims=dims,
                  dims_ptr=dev.data_ptr())
    assert np.array_equal(got, expect(range(5), sizes)), "dims"
    # dims and an active table together
    got = _launch(native, frames, lay, steps, c, 0, H, steps, 0, H, border, batch=3, batch_stride=stride, dims=dims,
                  dims_ptr=dev.data_ptr(), active=[0, 2, 4], active_ptr=act.data_ptr(), batch_frames=5)
    assert np.array_equal(got, expect([0, 2, 4], sizes)), "dims + active"
    assert rb == W * c * 2


def test_guards_name_the_problem_and_launch_nothing(native):
    """Odd row_bytes, a dims entry that is no whole pixel, a misaligned pointer
    for a 16-byte-lane shape, variant binomial and a filter other than the
    gaussian: each a named error, the destination still all canary."""
    import torch

    c, h, w, steps = 3, 9, 13, 2
    rb = w * c * 2
    lay = native.frame_layout(rb, h, steps)
    frame = np.zeros((1, h + 2 * steps, lay["pitch"]), np.uint8)
    src = _alloc(torch, frame)
    dst = _alloc(torch, np.full(frame.shape, CANARY, np.uint8))
    base = GUARD + lay["pitch"] * steps + 16
    s = torch.cuda.current_stream().cuda_stream

    def launch(filt="gaussian", off=0, row_bytes=rb, variant="temporal", **kw):
        native.launch_stencil(filt, "rgb", src.data_ptr() + base + off, dst.data_ptr() + base + off, lay["pitch"],
                              row_bytes, 0, h, -steps, h + steps, steps, 0, h, s, variant, depth=16, **kw)

    with pytest.raises(RuntimeError, match="no whole number of depth-16 pixels"):
        launch(row_bytes=rb - 1)
    with pytest.raises(RuntimeError, match="no whole number of depth-16 pixels"):
        launch(row_bytes=rb - 2)  # whole samples, but no whole rgb pixel
    dims = [(rb - 3, h)]
    dev = torch.tensor(dims, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match=r"dims\[0\].row_bytes .* is no whole number of pixels"):
        launch(dims=dims, dims_ptr=dev.data_ptr())
    native.set_swar16_shape(8, 8, 8)
    with pytest.raises(RuntimeError, match="multiples of 16 bytes"):
        launch(off=8)
    native.set_swar16_shape(0, 0, 0)
    with pytest.raises(RuntimeError, match="depth 16 not supported by kernel 'binomial'"):
        native.launch_stencil("gaussian", "rgb", src.data_ptr() + base, dst.data_ptr() + base, lay["pitch"], rb, 0, h,
                              -1, h + 1, 1, 0, h, s, "binomial", depth=16)
    with pytest.raises(RuntimeError, match="depth 16 runs the gaussian filter only"):
        launch(filt="box", variant="auto")
    with pytest.raises(RuntimeError, match="depth must be 8 or 16"):
        native.launch_stencil("gaussian", "rgb", src.data_ptr() + base, dst.data_ptr() + base, lay["pitch"], rb, 0, h,
                              -steps, h + steps, steps, 0, h, s, "temporal", depth=12)
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == CANARY).all(), "a refused launch wrote something"


def test_auto_variant_and_model_pick_at_every_step_count(native, pconv_mod, rng):
    """Nothing forced: variant auto routes every step count (1 included) to the
    16-bit kernel and the pick runs it, here and for a taller image."""
    for (h, w, c) in [(61, 77, 3), (300, 900, 1)]:
        img = _values(rng, h, w * c)
        rb = w * c * 2
        for steps in (1, 5, 16):
            lay = native.frame_layout(rb, h, steps)
            frame = np.zeros((1, h + 2 * steps, lay["pitch"]), np.uint8)
            frame[0, steps:steps + h, 16:16 + rb] = img.view(np.uint8).reshape(h, rb)
            got = _launch(native, frame, lay, steps, c, 0, h, steps, 0, h, "zero", variant="auto")[0]
            ref = _lone(pconv_mod, img, c, steps, "zero")
            assert np.array_equal(got[steps:steps + h, 16:16 + rb], ref.view(np.uint8).reshape(h, rb)), (h, w, steps)


# ---- public API -------------------------------------------------------------


def _rgb16(rng, h, w, c=3):
    return _values(rng, h, w * c).reshape((h, w, c) if c > 1 else (h, w))


@pytest.mark.parametrize("border", BORDERS)
def test_convolve_and_engine(pconv_mod, rng, border):
    import torch

    img = _rgb16(rng, 61, 77)
    ref = pconv_mod.numpy_convolve(img, 21, "gaussian", border)
    out = pconv_mod.convolve(img, 21, backend="hip", border=border)
    assert out.dtype == np.uint16 and np.array_equal(out, ref)
    t = torch.from_numpy(img).cuda()
    out = pconv_mod.convolve(t, 21, border=border)
    assert out.dtype == torch.uint16 and out.is_cuda and np.array_equal(out.cpu().numpy(), ref)
    eng = pconv_mod.Engine(77, 61, "rgb", border=border, depth=16)
    assert eng.fuse == 8 and eng.row_bytes == 77 * 6
    assert np.array_equal(eng(img, 21), ref)
    assert np.array_equal(eng(t, 21).cpu().numpy(), ref)
    with pytest.raises(TypeError):
        eng(t.to(torch.uint8), 1)
    with pytest.raises(ValueError, match="depth 16"):
        eng.residual(img)
    with pytest.raises(ValueError, match="depth 16"):
        pconv_mod.Engine(77, 61, "rgb", depth=16, graph=True)
    with pytest.raises(ValueError, match="gaussian filter only"):
        pconv_mod.convolve(t, 1, "box")


def test_batches_and_mixed_sizes(pconv_mod, rng):
    import torch

    stack = np.stack([_rgb16(rng, 33, 47) for _ in range(3)])
    ref = np.stack([pconv_mod.numpy_convolve(x, 11, "gaussian", "replicate") for x in stack])
    out = pconv_mod.convolve_batch(stack, 11, backend="hip", border="replicate")
    assert out.dtype == np.uint16 and np.array_equal(out, ref)
    t = torch.from_numpy(stack).cuda()
    eng = pconv_mod.BatchEngine(47, 33, "rgb", capacity=3, border="replicate", depth=16)
    got = eng(t, 11)
    assert got.dtype == torch.uint16 and got.is_cuda and np.array_equal(got.cpu().numpy(), ref)
    assert np.array_equal(eng.run_numpy(stack[:2], 11), ref[:2])
    with pytest.raises(ValueError, match="depth 16"):
        eng.residual(stack)
    imgs = [_rgb16(rng, h, w, 1) for h, w in [(40, 50), (1, 1), (37, 64)]]
    outs = pconv_mod.convolve_many(imgs, 9, backend="hip")
    for o, x in zip(outs, imgs):
        assert o.dtype == np.uint16 and np.array_equal(o, pconv_mod.numpy_convolve(x, 9))
    outs = eng.run_images([x[:20, :30] for x in stack], 4)
    for o, x in zip(outs, stack):
        assert np.array_equal(o, pconv_mod.numpy_convolve(np.ascontiguousarray(x[:20, :30]), 4, border="replicate"))


@pytest.mark.parametrize("border", BORDERS)
def test_cross_depth_property_on_the_gpu(pconv_mod, rng, border):
    """A uint8 image widened to uint16 gives the widened 8-bit result: ties the
    16-bit kernel to the 8-bit one."""
    x = rng.integers(0, 256, size=(70, 90, 3), dtype=np.uint8)
    a = pconv_mod.convolve(x.astype(np.uint16), 13, backend="hip", border=border)
    b = pconv_mod.convolve(x, 13, backend="hip", border=border)
    assert np.array_equal(a, b.astype(np.uint16))


@pytest.mark.parametrize("frames", [1, 3])
def test_cli_synthetic_check(pconv_mod, tmp_path, frames):
    args = [CONV_BIN, "s.raw", "77", "61", "5", "rgb", "--depth", "16", "--synthetic", "7", "--check", "--json",
            "--quiet", "--out", "out.raw"] + (["--frames", str(frames)] if frames > 1 else [])
    r = subprocess.run(args, cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    js = json.loads(r.stdout.strip().splitlines()[-1])
    assert js["depth"] == 16 and js["mismatches"] == 0 and js["backend"] == "hip"
    assert js["launches"] == math.ceil(5 / js["fuse"])
    out = np.fromfile(tmp_path / "out.raw", dtype="<u2").reshape(frames, 61, 77, 3)
    for k in range(frames):
        src = pconv_mod.synthetic_image(77, 61, "rgb", seed=7 + k, depth=16)
        assert np.array_equal(out[k], pconv_mod.numpy_convolve(src, 5, "gaussian")), k


def test_first_use_tuning(native, pconv_mod, rng):
    """Tuning on at one small geometry: bit-exact, the choice lands in the
    16-bit kernel's own table and swar_tuned() is unchanged."""
    native.clear_swar_tuning()
    before = native.swar_tuned()
    assert native.swar16_tuned() == []
    native.set_autotune(True)
    img = _rgb16(rng, 64, 80)
    eng = pconv_mod.Engine(80, 64, "rgb", fuse=4, depth=16)
    out = eng(img, 8)
    native.set_autotune(False)
    assert np.array_equal(out, pconv_mod.numpy_convolve(img, 8))
    tuned = native.swar16_tuned()
    assert len(tuned) == 1 and list(tuned[0][0][:4]) == [3, 4, 64, 80 * 6]
    assert tuple(tuned[0][1]) in SHAPES
    assert native.swar_tuned() == before
    native.clear_swar_tuning()
    assert native.swar16_tuned() == []
