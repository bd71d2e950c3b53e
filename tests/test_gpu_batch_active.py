"""Active-image tables on a real MI355X: launches of the SWAR tile kernel, the
buffer-op tile kernel, the float temporal kernel and the residual kernel over
SOME of the frames of one allocation (StencilLaunch active / active_host /
batch_frames).

The frames lie at a stride with a gap in one allocation; source and
destination are filled with a canary byte, pads, ghost rows and gaps included,
and every frame holds an image of its own (a launch that maps a slot to the
wrong frame reads the wrong image).  After a launch the destination is compared
BYTE FOR BYTE with the expected allocation: the image region of every active
frame is the NumPy oracle of that frame's image alone, everything else —
the frames the table does not name above all — is still the canary.  The
source must be unmodified.

Shapes are forced as in test_gpu_ragged.py (SWAR {4, 8, 8} in tile and
buffer-op mode, float {8, 8}) and tuning is off.  The buffer-op kernel takes
rows of whole dwords only (otherwise a forced buffer-op launch falls back to
the tile kernel), so its cases add the geometries widened to 16 pixels."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 4096
CANARY = 0xA5
NAME = {1: "grey", 3: "rgb", 4: "rgba"}
BORDERS = ["zero", "replicate"]
KERNELS = ["tile", "bufop", "float"]
GEOMS = [(1, 9, 13), (3, 21, 13)]  # (channels, height, width): the batch-convergence recipe's
DWORD_GEOMS = [(1, 9, 16), (3, 21, 16)]

_IMG = {}  # (frame, c, h, w) -> image
_REF = {}  # (filter, border, frame, c, h, w, steps) -> oracle


@pytest.fixture(autouse=True)
def forced(native):
    prev = native.set_autotune(False)
    native.set_swar_shape(4, 8, 8)
    native.set_float_shape(8, 8)
    yield
    native.set_prefetch_mode(-1)
    native.set_swar_shape(0, 0, 0)
    native.set_float_shape(0, 0)
    native.set_xcd_swizzle(True)
    native.set_autotune(prev)


def _select(native, kernel):
    """(variant, filter) of a kernel under test; sets the buffer-op mode."""
    native.set_prefetch_mode(1 if kernel == "bufop" else 0)
    return ("float_temporal", "box") if kernel == "float" else ("temporal", "gaussian")


def _image(frame, c, h, w):
    key = (frame, c, h, w)
    if key not in _IMG:
        rng = np.random.default_rng(7919 * frame + 613 * c + 104729 * h + w)
        img = rng.integers(0, 256, size=(h, w, c) if c > 1 else (h, w), dtype=np.uint8)
        img.setflags(write=False)
        _IMG[key] = img
    return _IMG[key]


def _oracle(pconv_mod, filt, border, frame, c, h, w, steps):
    key = (filt, border, frame, c, h, w, steps)
    if key not in _REF:
        _REF[key] = pconv_mod.numpy_convolve(_image(frame, c, h, w), steps, filt, border=border)
    return _REF[key]


def _table(entries):
    import torch

    return torch.tensor(list(entries), dtype=torch.int32, device="cuda").contiguous()


def _launch_active(native, pconv_mod, filt, c, H, W, steps, variant, border, frames, active, sizes=None, gap=48,
                   device_table=None):
    """`frames` frames of the geometry (c, H, W); frame b holds image b (of
    sizes[b] = (w, h) top-left in its frame when `sizes` is given, which also
    makes the launch carry the extents table, indexed by frame).  One launch
    over the frames `active` names (None: a plain batch launch over all of
    them).  Returns the list of mismatches (empty: all as expected)."""
    import torch

    rb, halo = W * c, steps
    lay = native.frame_layout(rb, H, halo)
    pitch, fbytes = lay["pitch"], lay["bytes"]
    stride = fbytes + gap
    total = frames * stride
    size_of = (lambda b: (W, H)) if sizes is None else (lambda b: sizes[b])
    src_host = np.full((frames, stride), CANARY, np.uint8)
    exp_host = np.full((frames, stride), CANARY, np.uint8)
    for b in range(frames):
        w, h = size_of(b)
        fr = src_host[b, :fbytes].reshape(H + 2 * halo, pitch)
        fr[halo:halo + h, 16:16 + w * c] = _image(b, c, h, w).reshape(h, w * c)
    for b in (range(frames) if active is None else active):
        w, h = size_of(b)
        ex = exp_host[b, :fbytes].reshape(H + 2 * halo, pitch)
        ex[halo:halo + h, 16:16 + w * c] = _oracle(pconv_mod, filt, border, b, c, h, w, steps).reshape(h, w * c)
    src = torch.full((total + 2 * GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    dst = torch.full((total + 2 * GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    src[GUARD:GUARD + total] = torch.from_numpy(src_host.reshape(-1)).cuda()
    kw = {}
    keep = []
    if sizes is not None:
        host = [(w * c, h) for w, h in sizes]
        dev = torch.tensor(host, dtype=torch.int32, device="cuda").contiguous()
        keep.append(dev)
        kw.update(dims=host, dims_ptr=dev.data_ptr())
    if active is None:
        kw.update(batch=frames)
    else:
        dev = _table(active if device_table is None else device_table)
        keep.append(dev)
        kw.update(batch=len(active), active=list(active), active_ptr=dev.data_ptr(), batch_frames=frames)
    base = GUARD + pitch * halo + 16
    native.launch_stencil(filt, NAME[c], src.data_ptr() + base, dst.data_ptr() + base, pitch, rb, 0, H, -halo, H + halo,
                          steps, 0, H, torch.cuda.current_stream().cuda_stream, variant, border=border,
                          batch_stride=stride, **kw)
    torch.cuda.synchronize()
    d = dst.cpu().numpy()
    case = (filt, variant, border, c, H, W, steps, frames, None if active is None else tuple(active))
    bad = []
    if not ((d[:GUARD] == CANARY).all() and (d[-GUARD:] == CANARY).all()):
        bad.append(case + ("write outside the allocation",))
    got = d[GUARD:-GUARD].reshape(frames, stride)
    if not np.array_equal(got, exp_host):
        b = int(np.argwhere((got != exp_host).any(axis=1))[0][0])
        off = np.argwhere(got[b] != exp_host[b])[:3].reshape(-1).tolist()
        where = [(o // pitch - halo, o % pitch - 16) if o < fbytes else ("gap", o - fbytes) for o in off]
        bad.append(case + (f"frame {b}: first differing (row, byte) {where}",))
    s = src.cpu().numpy()
    if not ((s[:GUARD] == CANARY).all() and (s[-GUARD:] == CANARY).all()
            and np.array_equal(s[GUARD:-GUARD], src_host.reshape(-1))):
        bad.append(case + ("the source was modified",))
    return bad


# ---- subsets of five frames -------------------------------------------------


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_subset_launches(native, pconv_mod, kernel, border):
    variant, filt = _select(native, kernel)
    bad, ran = [], 0
    for c, h, w in GEOMS + (DWORD_GEOMS if kernel == "bufop" else []):
        for steps in (1, 3):
            for active in ([1, 3], [4], [0, 1, 2, 3, 4]):
                bad += _launch_active(native, pconv_mod, filt, c, h, w, steps, variant, border, 5, active)
                ran += 1
    assert ran == (24 if kernel == "bufop" else 12)
    assert not bad, bad[:6]


@pytest.mark.parametrize("kernel", KERNELS)
def test_auto_routes_a_one_step_active_launch_to_the_temporal_kernels(native, pconv_mod, kernel):
    _, filt = _select(native, kernel)
    assert not _launch_active(native, pconv_mod, filt, 3, 21, 16, 1, "auto", "zero", 3, [2])


# ---- more than one tile per image, more than 8 images -----------------------


def _tiles_per_image(kernel, c, h, w, steps):
    """swar_geom / ft_geom of the forced shapes: (tiles along the row, tiles down the rows)."""
    if kernel == "float":
        hl = (steps * c + 7) // 8
        vlanes, vrows = 64 - 2 * hl, 8 * 8 - 2 * steps
        return math.ceil(math.ceil(w * c / 8) / vlanes), math.ceil(h / vrows)
    hl = (steps * c + 3) // 4
    vbytes, vrows = (64 - 2 * hl) * 4, 8 * 8 - 2 * steps
    return (math.ceil(w * c / vbytes) + 1) // 2, math.ceil(h / vrows)


@pytest.mark.parametrize("swizzle", [True, False])
@pytest.mark.parametrize("kernel", KERNELS)
def test_several_tiles_per_image_and_more_than_eight_images(native, pconv_mod, kernel, swizzle):
    """500x61 grey at 3 steps: 248 output bytes per strip (3 strips, 2 strip
    pairs) and 58 output rows per tile under SWAR {4, 8, 8}, 496 bytes and 58
    rows under float {8, 8} — 2 x 2 tiles per image either way.  9 of 12 frames
    are 36 workgroups: the image index is tile / 4 of the remapped id."""
    variant, filt = _select(native, kernel)
    native.set_xcd_swizzle(swizzle)
    c, h, w, steps = 1, 61, 500, 3
    assert _tiles_per_image(kernel, c, h, w, steps) == (2, 2)
    active = [0, 1, 3, 4, 6, 7, 8, 10, 11]
    bad = []
    for border in BORDERS:
        bad += _launch_active(native, pconv_mod, filt, c, h, w, steps, variant, border, 12, active)
    assert not bad, bad[:6]


# ---- with per-image extents -------------------------------------------------


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_active_with_dims_is_indexed_by_frame(native, pconv_mod, kernel, border):
    """Five frames of five sizes (rows of whole dwords: the buffer-op kernel
    takes them too), active = [1, 3]: frames 1 and 3 are convolved as lone
    images of THEIR sizes — a table read by slot would give frame 1 the
    envelope's extent and frame 3 frame 1's."""
    variant, filt = _select(native, kernel)
    c, H, W, steps = 3, 61, 164, 3
    assert _tiles_per_image(kernel, c, H, W, steps) == (2, 2)
    sizes = [(164, 61), (8, 5), (100, 61), (84, 59), (156, 1)]
    assert all((w * c) % 4 == 0 for w, _ in sizes)
    bad = _launch_active(native, pconv_mod, filt, c, H, W, steps, variant, border, 5, [1, 3], sizes=sizes)
    bad += _launch_active(native, pconv_mod, filt, c, H, W, steps, variant, border, 5, [0, 2, 4], sizes=sizes)
    assert not bad, bad[:6]


# ---- a device table that differs from its host copy ----------------------------


@pytest.mark.parametrize("kernel", KERNELS)
def test_a_wrong_device_table_stays_inside_the_frames(native, pconv_mod, kernel):
    """The guards read the host copy; the kernels clamp what they load to
    batch_frames - 1: entries far beyond the frames, and negative ones, land on
    the last frame (which here is the frame the host copy names)."""
    variant, filt = _select(native, kernel)
    for wild in (1 << 20, -5, 0x7FFFFFFF):
        assert not _launch_active(native, pconv_mod, filt, 3, 21, 16, 3, variant, "replicate", 3, [2],
                                  device_table=[wild])


# ---- the residual kernel ------------------------------------------------------


def _residual_active(native, pconv_mod, filt, border, c, H, W, frames, active, sizes=None):
    import torch

    halo = 1
    rb = W * c
    lay = native.frame_layout(rb, H, halo)
    pitch, fbytes = lay["pitch"], lay["bytes"]
    stride = fbytes + 48
    src_host = np.full((frames, stride), CANARY, np.uint8)
    want = []
    for b in range(frames):
        w, h = (W, H) if sizes is None else sizes[b]
        img = _image(b, c, h, w)
        fr = src_host[b, :fbytes].reshape(H + 2 * halo, pitch)
        fr[halo:halo + h, 16:16 + w * c] = img.reshape(h, w * c)
        want.append(int(pconv_mod.numpy_residual(img, filt, border)))
    assert all(x > 0 for x in want)
    src = torch.from_numpy(src_host.reshape(-1)).cuda()
    start = [0x0123456789AB0000 + 7919 * b for b in range(frames + 1)]  # distinct sentinels; [frames]: beyond
    counters = torch.tensor(start, dtype=torch.int64, device="cuda")
    table = _table(active)
    kw = dict(active=list(active), active_ptr=table.data_ptr(), batch_frames=frames)
    if sizes is not None:
        host = [(w * c, h) for w, h in sizes]
        dev = torch.tensor(host, dtype=torch.int32, device="cuda").contiguous()
        kw.update(dims=host, dims_ptr=dev.data_ptr())
    native.launch_residual_batch(filt, NAME[c], src.data_ptr() + pitch * halo + 16, pitch, rb, 0, H, -halo, H + halo,
                                 counters.data_ptr(), len(active), stride, 0, H,
                                 torch.cuda.current_stream().cuda_stream, border, **kw)
    got = counters.cpu().numpy().tolist()
    exp = [start[b] + (want[b] if b in active else 0) for b in range(frames)] + [start[frames]]
    assert got == exp, (filt, border, c, H, W, active, [g - s for g, s in zip(got, start)], want)
    assert np.array_equal(src.cpu().numpy(), src_host.reshape(-1))


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("filt", ["gaussian", "box"])  # the int form and the float form
def test_residual_counts_land_on_the_frames_counters(native, pconv_mod, filt, border):
    R = native.RESIDUAL_BLOCK_ROWS
    for c, H, W in [(1, 9, 13), (3, 21, 13), (3, R + 8, 1024 // 3 + 30)]:  # the last: 2 x 2 workgroups per image
        for active in ([1, 3], [4], [0, 1, 2, 3, 4]):
            _residual_active(native, pconv_mod, filt, border, c, H, W, 5, active)
    assert math.ceil((R + 8) / R) == 2 and math.ceil((1024 // 3 + 30) * 3 / 1024) == 2
    # more than 8 images, several workgroups each
    _residual_active(native, pconv_mod, filt, border, 1, R + 1, 1100, 12, [0, 1, 3, 4, 6, 7, 8, 10, 11])
    # with the extents table, indexed by frame
    sizes = [(164, 61), (8, 5), (100, 61), (84, 59), (156, 1)]
    _residual_active(native, pconv_mod, filt, border, 3, 61, 164, 5, [1, 3], sizes=sizes)


# ---- no table ---------------------------------------------------------------------


@pytest.mark.parametrize("kernel", KERNELS)
def test_without_a_table_the_launch_is_the_batch_launch(native, pconv_mod, kernel):
    import torch

    variant, filt = _select(native, kernel)
    c, h, w, steps = 3, 21, 16, 3
    assert not _launch_active(native, pconv_mod, filt, c, h, w, steps, variant, "replicate", 5, None)
    # the binding's defaults are the call without the three arguments
    rb = w * c
    lay = native.frame_layout(rb, h, steps)
    pitch, fbytes = lay["pitch"], lay["bytes"]
    src = torch.zeros(2 * fbytes, dtype=torch.uint8, device="cuda")
    fr = np.zeros((2, h + 2 * steps, pitch), np.uint8)
    for b in range(2):
        fr[b, steps:steps + h, 16:16 + rb] = _image(b, c, h, w).reshape(h, rb)
    src.copy_(torch.from_numpy(fr.reshape(-1)))
    outs = []
    for kw in ({}, dict(active=None, active_ptr=0, batch_frames=1)):
        dst = torch.zeros(2 * fbytes, dtype=torch.uint8, device="cuda")
        base = pitch * steps + 16
        native.launch_stencil(filt, "rgb", src.data_ptr() + base, dst.data_ptr() + base, pitch, rb, 0, h, -steps,
                              h + steps, steps, 0, h, torch.cuda.current_stream().cuda_stream, variant,
                              border="replicate", batch=2, batch_stride=fbytes, **kw)
        torch.cuda.synchronize()
        outs.append(dst.cpu().numpy().reshape(2, h + 2 * steps, pitch))
    assert np.array_equal(outs[0], outs[1])
    for b in range(2):
        assert np.array_equal(outs[0][b, steps:steps + h, 16:16 + rb].reshape(_image(b, c, h, w).shape),
                              _oracle(pconv_mod, filt, "replicate", b, c, h, w, steps))


# ---- guards -------------------------------------------------------------------


def test_guards(native):
    import torch

    c, h, w, steps = 3, 8, 16, 2
    rb = w * c
    lay = native.frame_layout(rb, h, steps)
    pitch, fbytes = lay["pitch"], lay["bytes"]
    src = torch.zeros(4 * fbytes, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(4 * fbytes, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    base = pitch * steps + 16
    dev = _table([0, 1, 2, 3])

    def launch(variant="auto", filt="gaussian", st=steps, **kw):
        kw.setdefault("batch", 2)
        kw.setdefault("batch_stride", fbytes)
        native.launch_stencil(filt, "rgb", src.data_ptr() + base, dst.data_ptr() + base, pitch, rb, 0, h, -steps,
                              h + steps, st, 0, h, torch.cuda.current_stream().cuda_stream, variant, **kw)

    def resid(filt="gaussian", **kw):
        batch = kw.pop("batch", 2)
        stride = kw.pop("batch_stride", fbytes)
        native.launch_residual_batch(filt, "rgb", src.data_ptr() + base, pitch, rb, 0, h, -steps, h + steps,
                                     cnt.data_ptr(), batch, stride, 0, h, **kw)

    ptr = dict(active_ptr=dev.data_ptr(), batch_frames=4)
    for call in (lambda **kw: launch("auto", "gaussian", **kw), lambda **kw: launch("float_temporal", "box", **kw),
                 lambda **kw: resid("gaussian", **kw), lambda **kw: resid("box", **kw)):
        with pytest.raises(RuntimeError, match="active and active_host must be given together"):
            call(**ptr)  # the device table without its host copy
        with pytest.raises(RuntimeError, match="active and active_host must be given together"):
            call(active=[0, 1], batch_frames=4)
        with pytest.raises(RuntimeError, match=r"active\[1\] = 1 does not exceed the entry before it"):
            call(active=[1, 1], **ptr)
        with pytest.raises(RuntimeError, match=r"active\[1\] = 0 does not exceed the entry before it"):
            call(active=[2, 0], **ptr)
        with pytest.raises(RuntimeError, match=r"active\[1\] = 4 is outside \[0, batch_frames 4\)"):
            call(active=[1, 4], **ptr)
        with pytest.raises(RuntimeError, match=r"active\[0\] = -1 is outside \[0, batch_frames 4\)"):
            call(active=[-1, 2], **ptr)
        with pytest.raises(RuntimeError, match="active: the list must hold `batch` frame indices"):
            call(active=[0, 1, 2], **ptr)
        with pytest.raises(RuntimeError, match="active holds 2 entries, more than batch_frames 1"):
            call(active=[0, 1], active_ptr=dev.data_ptr())  # batch_frames defaults to 1
        # the stride rules of the FRAMES, also for a single entry
        with pytest.raises(RuntimeError, match="multiple of 16"):
            call(active=[3], batch=1, batch_stride=fbytes + 8, **ptr)
        with pytest.raises(RuntimeError, match="smaller than a frame"):
            call(active=[3], batch=1, batch_stride=fbytes - 16, **ptr)
        # with dims the list is indexed by frame: batch_frames pairs
        with pytest.raises(RuntimeError, match="must hold `batch_frames`"):
            call(active=[1, 3], dims=[(rb, h), (3, 1)], dims_ptr=dev.data_ptr(), **ptr)
    # the single-step variants refuse a table by name
    for variant, filt in (("binomial", "gaussian"), ("int9", "gaussian"), ("float9", "box")):
        with pytest.raises(RuntimeError, match=f"active not supported by kernel '{variant}'"):
            launch(variant, filt, st=1, batch=1, active=[2], **ptr)
    # forced buffer-op mode: the whole-dword rule is evaluated over the active frames only
    native.set_prefetch_mode(1)
    odd = [(rb, h), (3, 1), (rb, h), (rb, h)]
    dims_dev = torch.tensor(odd, dtype=torch.int32, device="cuda").contiguous()
    with pytest.raises(RuntimeError, match="whole dwords per row of every image"):
        launch("temporal", active=[1, 2], dims=odd, dims_ptr=dims_dev.data_ptr(), **ptr)
    even = _table([0, 2])
    launch("temporal", active=[0, 2], dims=odd, dims_ptr=dims_dev.data_ptr(), active_ptr=even.data_ptr(), batch_frames=4)
    native.set_prefetch_mode(-1)
    torch.cuda.synchronize()
    # no refused launch ran: zeros in, zeros out, and no counter moved
    assert int(dst.sum()) == 0 and cnt.cpu().tolist() == [0, 0, 0, 0]
