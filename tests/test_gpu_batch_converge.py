"""Batches stop at their fixed points, on a real MI355X: the residual kernel
with an image batch (one launch, one 64-bit counter per image), then
``BatchEngine.residual`` / ``run_until_stable`` and
``convolve_batch_until_stable(backend="hip")``.

Kernel level: B frames lie at stride ``frame bytes + 48`` in one allocation
between canaries, the ghost rows hold garbage; the counters are a 64-bit tensor
with sentinel entries on both sides and a non-zero start value in every slot.
Every launch must ADD image b's oracle count to slot b, leave every other word
of the counter tensor alone and leave the source allocation byte-identical.

Engine and API level: every image of a batch ends as the single-image
NumPy-backend run of that image ends, in bytes and in StableInfo.

Exact integers and exact bytes only.  Tuning is off, shapes and fuse are forced."""
import math

import numpy as np
import pytest

from batch_converge_recipe import BORDERS, GEOMS, NAME, RUNS, check_spread, oracle, recipe

pytestmark = pytest.mark.gpu

GUARD = 4096
CANARY = 0xA5
GAPFILL = 0x5A
GARBAGE = 0xEE
GAP = 48
SENTINELS = 4
SENTINEL = 0x5A5A5A5A5A5A5A5A
NEG_TAPS = ([3, 1, 0, 2, 5, 1, -1, 2, 4], 17)  # the negative-tap custom filter of test_gpu_kernels.py

_IMGS = {}  # (c, h, w) -> the 5 images of that geometry
_RES = {}   # (filter key, border, c, h, w) -> their oracle counts


@pytest.fixture(autouse=True)
def forced(native):
    prev = native.set_autotune(False)
    native.set_swar_shape(4, 8, 8)
    native.set_float_shape(8, 4)
    yield
    native.set_swar_shape(0, 0, 0)
    native.set_float_shape(0, 0)
    native.set_autotune(prev)


def _filters(pconv_mod, filt):
    if filt == "neg":
        return pconv_mod.get_filter(NEG_TAPS), pconv_mod.native.Filter.custom(NEG_TAPS[0], NEG_TAPS[1], "custom")
    return filt, filt


def _images(c, h, w):
    """All 255, all 0, three random."""
    key = (c, h, w)
    if key not in _IMGS:
        rng = np.random.default_rng(15485863 * c + 1009 * h + w)
        shape = (h, w, c) if c > 1 else (h, w)
        imgs = [np.full(shape, 255, np.uint8), np.zeros(shape, np.uint8)]
        imgs += [rng.integers(0, 256, size=shape, dtype=np.uint8) for _ in range(3)]
        _IMGS[key] = imgs
    return _IMGS[key]


def _counts(pconv_mod, filt, border, c, h, w):
    key = (filt, border, c, h, w)
    if key not in _RES:
        pf, _ = _filters(pconv_mod, filt)
        _RES[key] = [pconv_mod.numpy_residual(im, pf, border) for im in _images(c, h, w)]
    return _RES[key]


def _start(slots):
    return [1000003 + 7919 * b for b in range(slots)]


def _launch(native, imgs, nfilt, border, batch, capacity=None, batch_stride=None, raw=False):
    """One batched residual launch over the first `batch` of `capacity` frames
    (frame b holds imgs[b], or garbage where imgs[b] is None).  Checks that the
    sentinels and the slots >= batch of the counter tensor and every byte of
    the source allocation are what they were; returns the per-image amounts
    added to slots [0, batch)."""
    import torch

    capacity = len(imgs) if capacity is None else capacity
    first = next(im for im in imgs if im is not None)
    h, w = first.shape[:2]
    c = 1 if first.ndim == 2 else first.shape[2]
    rb, halo = w * c, 1
    lay = native.frame_layout(rb, h, halo)
    pitch, fbytes = lay["pitch"], lay["bytes"]
    stride = fbytes + GAP
    host = np.full((capacity, stride), GAPFILL, np.uint8)
    for b in range(capacity):
        if imgs[b] is None:
            host[b, :fbytes] = GARBAGE
            continue
        fr = host[b, :fbytes].reshape(h + 2 * halo, pitch)
        fr[:] = 0
        fr[:, 16:16 + rb] = GARBAGE  # ghost rows: outside the image nothing may be read as data
        fr[halo:halo + h, 16:16 + rb] = imgs[b].reshape(h, rb)
    total = capacity * stride
    before = np.full(total + 2 * GUARD, CANARY, np.uint8)
    before[GUARD:GUARD + total] = host.reshape(-1)
    src = torch.from_numpy(before).cuda()
    start = _start(capacity)
    words = [SENTINEL] * SENTINELS + start + [SENTINEL] * SENTINELS
    ctr = torch.tensor(words, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    native.launch_residual_batch(nfilt, NAME[c], src.data_ptr() + GUARD + pitch * halo + 16, pitch, rb, 0, h, -halo,
                                 h + halo, ctr.data_ptr() + 8 * SENTINELS, batch,
                                 stride if batch_stride is None else batch_stride, 0, h,
                                 torch.cuda.current_stream().cuda_stream, border=border)
    torch.cuda.synchronize()
    got = ctr.cpu().tolist()
    assert got[:SENTINELS] == [SENTINEL] * SENTINELS and got[-SENTINELS:] == [SENTINEL] * SENTINELS, "sentinel hit"
    slots = got[SENTINELS:-SENTINELS]
    assert slots[batch:] == start[batch:], "a counter beyond the batch moved"
    assert np.array_equal(src.cpu().numpy(), before), "the kernel wrote into the source allocation"
    return [slots[b] - start[b] for b in range(batch)]


def _widths(c):
    """Pixel widths whose row bytes sit just below, at and above 16 and 1024, plus one pixel."""
    ws = {1}
    for edge in (16, 1024):
        ws.update({(edge - 1) // c, -(-edge // c), edge // c + 1})
    return sorted(x for x in ws if x >= 1)


# ---- kernel ------------------------------------------------------------


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("filt", ["gaussian", "box", "neg"])
def test_counts_per_image_equal_the_oracle(pconv_mod, native, filt, border):
    _, nf = _filters(pconv_mod, filt)
    bad, ran = [], 0
    for c in (1, 3, 4):
        for w in _widths(c):
            for h in (1, 2, native.RESIDUAL_BLOCK_ROWS + 1):
                got = _launch(native, _images(c, h, w), nf, border, 5)
                want = _counts(pconv_mod, filt, border, c, h, w)
                ran += 1
                if got != want:
                    bad.append((c, h, w, got, want))
    assert ran == 3 * (7 + 5 + 7)  # widths per channel count x heights
    assert not bad, (len(bad), bad[:8])


@pytest.mark.parametrize("border", BORDERS)
def test_partial_batch(pconv_mod, native, border):
    """batch = 2 in allocations of 4 frames: frames 2 and 3 hold garbage and
    are never counted, counters 2 and 3 keep their start values (_launch)."""
    for c, h, w, filt in [(3, 33, 45, "gaussian"), (1, 9, 13, "box")]:
        imgs = _images(c, h, w)
        got = _launch(native, [imgs[2], imgs[3], None, None], filt, border, batch=2, capacity=4)
        assert got == _counts(pconv_mod, filt, border, c, h, w)[2:4], (c, h, w, filt)


def test_a_zero_image_between_two_white_ones_counts_zero(pconv_mod, native):
    for c, h, w, filt in [(1, 9, 13, "gaussian"), (3, 33, 45, "box"), (4, 2, 5, "gaussian")]:
        imgs = _images(c, h, w)
        want = _counts(pconv_mod, filt, "zero", c, h, w)
        assert want[0] > 0 and want[1] == 0
        assert _launch(native, [imgs[0], imgs[1], imgs[0]], filt, "zero", 3) == [want[0], 0, want[0]]


def _fixed_point(pconv_mod, img, filt, border):
    x = img
    for _ in range(2000):
        nxt = pconv_mod.ops.reference.numpy_step(x, filt, border)
        if np.array_equal(nxt, x):
            break
        x = nxt
    assert pconv_mod.numpy_residual(x, filt, border) == 0
    return x


@pytest.mark.parametrize("c,h,w,filt", [(1, 9, 13, "gaussian"), (3, 21, 13, "box")])
def test_fixed_point_and_one_flipped_byte(pconv_mod, native, c, h, w, filt):
    """An oracle fixed point (replicate: not all zero) in the middle slot counts
    0 while its neighbours do not; flipping its first / last byte changes its
    counter only, by the oracle's amount."""
    imgs = _images(c, h, w)
    want = _counts(pconv_mod, filt, "replicate", c, h, w)
    fix = _fixed_point(pconv_mod, imgs[2], filt, "replicate")
    assert fix.any() and want[3] > 0 and want[4] > 0
    assert _launch(native, [imgs[3], fix, imgs[4]], filt, "replicate", 3) == [want[3], 0, want[4]]
    for pos in (0, fix.size - 1):
        x = fix.copy()
        x.reshape(-1)[pos] ^= 0x80
        changed = pconv_mod.numpy_residual(x, filt, "replicate")
        assert changed > 0
        assert _launch(native, [imgs[3], x, imgs[4]], filt, "replicate", 3) == [want[3], changed, want[4]], pos
    # the same for a random image in the first and the last slot
    for slot in (0, 2):
        for pos in (0, imgs[2].size - 1):
            x = imgs[2].copy()
            x.reshape(-1)[pos] ^= 0x80
            batch = [imgs[3], imgs[3], imgs[3]]
            batch[slot] = x
            exp = [want[3]] * 3
            exp[slot] = pconv_mod.numpy_residual(x, filt, "replicate")
            assert _launch(native, batch, filt, "replicate", 3) == exp, (slot, pos)


@pytest.mark.parametrize("border", BORDERS)
def test_many_workgroups_per_image(pconv_mod, native, border):
    """3 x 70x2100 grey random: 9 workgroups each, 27 in the launch (no
    multiple of 8); every image's atomics land on its own counter."""
    h, w = 70, 2100
    assert math.ceil(w / 1024) * math.ceil(h / native.RESIDUAL_BLOCK_ROWS) == 9
    imgs = _images(1, h, w)[2:5]
    for filt in ("gaussian", "box"):
        want = _counts(pconv_mod, filt, border, 1, h, w)[2:5]
        assert len(set(want)) == 3 and min(want) > h * w // 2
        assert _launch(native, imgs, filt, border, 3) == want, filt


def test_stride_beyond_32_bits(pconv_mod, native):
    """Two 16x8 grey frames 2^32 + 4096 bytes apart in one allocation: only the
    two frames (a canary ring around each) are read, nothing is written."""
    import torch

    c, h, w, halo = 1, 8, 16, 1
    stride = (1 << 32) + 4096
    lay = native.frame_layout(w, h, halo)
    pitch, fbytes = lay["pitch"], lay["bytes"]
    assert fbytes + 2 * GUARD < (2 << 20)
    imgs = _images(c, h, w)[2:4]
    want = _counts(pconv_mod, "gaussian", "replicate", c, h, w)[2:4]
    assert want[0] != want[1]
    src = torch.empty(stride + (2 << 20), dtype=torch.uint8, device="cuda")
    blocks = []
    for b in range(2):
        blk = np.full(fbytes + 2 * GUARD, CANARY, np.uint8)
        fr = blk[GUARD:GUARD + fbytes].reshape(h + 2 * halo, pitch)
        fr[:] = 0
        fr[:, 16:16 + w] = GARBAGE
        fr[halo:halo + h, 16:16 + w] = imgs[b]
        blocks.append(blk)
        src[b * stride:b * stride + blk.size] = torch.from_numpy(blk).cuda()
    start = _start(2)
    ctr = torch.tensor([SENTINEL] + start + [SENTINEL], dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    native.launch_residual_batch("gaussian", "grey", src.data_ptr() + GUARD + pitch * halo + 16, pitch, w, 0, h, -halo,
                                 h + halo, ctr.data_ptr() + 8, 2, stride, 0, h,
                                 torch.cuda.current_stream().cuda_stream, border="replicate")
    torch.cuda.synchronize()
    got = ctr.cpu().tolist()
    assert got[0] == SENTINEL and got[3] == SENTINEL
    assert [got[1] - start[0], got[2] - start[1]] == want
    for b in range(2):
        assert np.array_equal(src[b * stride:b * stride + blocks[b].size].cpu().numpy(), blocks[b]), b
    del src
    torch.cuda.empty_cache()


@pytest.mark.parametrize("border", BORDERS)
def test_batch_of_one_is_launch_residual(pconv_mod, native, border):
    import torch

    for c, h, w, filt in [(3, 33, 45, "gaussian"), (1, 70, 2100, "box"), (4, 2, 5, "gaussian")]:
        img = _images(c, h, w)[3]
        want = _counts(pconv_mod, filt, border, c, h, w)[3]
        # the stride of one image is ignored, whatever it is
        for stride in (7, 0, None):
            assert _launch(native, [img], filt, border, 1, batch_stride=stride) == [want], (c, h, w, stride)
        rb = w * c
        lay = native.frame_layout(rb, h, 1)
        fr = np.zeros((h + 2, lay["pitch"]), np.uint8)
        fr[:, 16:16 + rb] = GARBAGE
        fr[1:1 + h, 16:16 + rb] = img.reshape(h, rb)
        src = torch.from_numpy(fr.reshape(-1)).cuda()
        one = native.launch_residual(filt, NAME[c], src.data_ptr() + lay["pitch"] + 16, lay["pitch"], rb, 0, h, -1,
                                     h + 1, 0, h, torch.cuda.current_stream().cuda_stream, border=border)
        assert int(one) == want


def test_guards(native):
    import torch

    h, w, halo = 33, 16, 1
    lay = native.frame_layout(w, h, halo)
    pitch, fbytes = lay["pitch"], lay["bytes"]
    src = torch.zeros(3 * fbytes, dtype=torch.uint8, device="cuda")
    start = _start(3)
    ctr = torch.tensor(start, dtype=torch.int64, device="cuda")

    def launch(batch, stride):
        native.launch_residual_batch("gaussian", "grey", src.data_ptr() + pitch * halo + 16, pitch, w, 0, h, -halo,
                                     h + halo, ctr.data_ptr(), batch, stride, 0, h,
                                     torch.cuda.current_stream().cuda_stream)

    for batch in (0, -1):
        with pytest.raises(RuntimeError, match="launch_residual: batch must be >= 1"):
            launch(batch, fbytes)
    with pytest.raises(RuntimeError, match="multiple of 16"):
        launch(2, fbytes + 8)
    with pytest.raises(RuntimeError, match="smaller than a frame"):
        launch(2, fbytes - 16)
    # 33 rows are 2 workgroups per image: 2^30 images are 2^31 workgroups
    assert math.ceil(h / native.RESIDUAL_BLOCK_ROWS) == 2
    with pytest.raises(RuntimeError, match="too many workgroups"):
        launch(1 << 30, fbytes)
    # the geometry guards hold per image
    with pytest.raises(RuntimeError, match="exceed frame"):
        native.launch_residual_batch("gaussian", "grey", src.data_ptr() + pitch * halo + 16, pitch, w, 0, h + 1, -halo,
                                     h + halo, ctr.data_ptr(), 2, fbytes, 0, 100)
    torch.cuda.synchronize()
    assert ctr.cpu().tolist() == start  # no refused launch touched a counter
    # the single-image binding is what it was: no batch keyword
    with pytest.raises(TypeError):
        native.launch_residual("gaussian", "grey", src.data_ptr() + pitch * halo + 16, pitch, w, 0, h, -halo, h + halo,
                               0, h, batch=2)
    launch(3, fbytes)
    torch.cuda.synchronize()
    assert ctr.cpu().tolist() == start  # three all-zero images, zero border: nothing to add


# ---- engine and API ------------------------------------------------------


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("filt", ["gaussian", "box"])
def test_native_batch_engine_residual(pconv_mod, native, filt, border):
    c, h, w, cap, fuse = 3, 33, 45, 4, 8
    imgs = _images(c, h, w)
    stack = np.stack(imgs[:1] + imgs[2:5])  # all 255 and the three random ones
    eng = native.BatchEngine(w, h, "rgb", cap, filt, fuse=fuse, border=border)
    assert eng.residual(0) == []
    for n in (cap, 3):
        eng.upload(stack[:n].reshape(-1), n)
        want = [pconv_mod.numpy_residual(stack[b], filt, border) for b in range(n)]
        assert len(set(want)) >= 3  # (all 255 is a fixed point under replicate, the random images differ)
        assert eng.residual(n) == want, n
        assert eng.residual(n) == want, n  # the counters run on: a check is a difference
        for reps in (8, 20):  # 1 and 3 launches: both end parities
            eng.upload(stack[:n].reshape(-1), n)
            eng.run(reps, n)
            want = [pconv_mod.numpy_residual(pconv_mod.numpy_convolve(stack[b], reps, filt, border=border), filt,
                                             border) for b in range(n)]
            assert eng.residual(n) == want, (n, reps)
    with pytest.raises(RuntimeError, match="capacity"):
        eng.residual(cap + 1)
    with pytest.raises(RuntimeError, match="capacity"):
        eng.run_until_stable(8, 8, cap + 1)
    with pytest.raises(RuntimeError, match="check_every"):
        eng.run_until_stable(8, 0, cap)
    assert eng.run_until_stable(8, 8, 0) == []


def _launches(max_reps, k, fuse, last_reps_done):
    """Launches of the loop: chunks of k (the last shorter), the next chunk
    already enqueued when a check's counts arrive; it ends at the check that
    finds the last image converged (after `last_reps_done`) or at max_reps."""
    done = min(k, max_reps)
    chunks = [done]
    while True:
        nxt = min(k, max_reps - done)
        if nxt > 0:
            chunks.append(nxt)
        if done >= last_reps_done or nxt == 0:
            break
        done += nxt
    return sum(math.ceil(x / fuse) for x in chunks)


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("c,h,w,filt", GEOMS)
def test_run_until_stable(pconv_mod, native, c, h, w, filt, border):
    import torch

    from pconv.ops import stencil

    check_spread(pconv_mod, c, h, w, filt, border)
    stack = recipe(c, h, w)
    n = len(stack)
    eng = pconv_mod.BatchEngine(w, h, NAME[c], n, filt, fuse=4, border=border)
    assert eng.fuse == 4
    for max_reps, k in RUNS:
        refs, rinfos = oracle(pconv_mod, c, h, w, filt, border, max_reps, k)
        case = (filt, border, max_reps, k)
        out, infos = eng.run_until_stable(stack, max_reps, check_every=k)
        assert isinstance(out, np.ndarray) and infos == rinfos, case
        for b in range(n):
            assert np.array_equal(out[b], refs[b]), case + (b,)
        assert eng.stats.launches == _launches(max_reps, k, 4, max(i.reps_done for i in rinfos)), case
        # the resident frames are the returned images
        assert eng.residual().tolist() == [i.residual for i in rinfos], case
        # chunks of 3, 3 and 1 through the public entry, each with its own loop
        out, infos = pconv_mod.convolve_batch_until_stable(stack, max_reps, filt, check_every=k, backend="hip",
                                                           fuse=4, border=border, batch_size=3)
        assert isinstance(out, np.ndarray) and infos == rinfos, case
        assert np.array_equal(out, np.stack(refs)), case
        beng = next(reversed(stencil._BATCH_ENGINES.values()))
        assert beng.capacity == 3 and beng.stats.launches == _launches(max_reps, k, 4, rinfos[6].reps_done), case
    refs, rinfos = oracle(pconv_mod, c, h, w, filt, border, 24, 8)
    kw = dict(filter=filt, check_every=8, backend="hip", fuse=4, border=border)
    # a partial batch on the 7-image engine, and residual(stack)
    out, infos = eng.run_until_stable(stack[2:5], 24, check_every=8)
    assert infos == rinfos[2:5] and np.array_equal(out, np.stack(refs[2:5]))
    assert eng.residual().tolist() == [i.residual for i in rinfos[2:5]]
    assert eng.residual(stack).tolist() == [pconv_mod.numpy_residual(stack[b], filt, border) for b in range(n)]
    assert pconv_mod.residual_batch(stack, filt, backend="hip", border=border).tolist() == eng.residual().tolist()
    # a list of images
    out, infos = pconv_mod.convolve_batch_until_stable([stack[b] for b in range(n)], 24, **kw)
    assert isinstance(out, np.ndarray) and infos == rinfos and np.array_equal(out, np.stack(refs))
    # a CUDA stack in, a CUDA stack out; an empty one
    dev = torch.from_numpy(stack.copy()).cuda()
    out, infos = pconv_mod.convolve_batch_until_stable(dev, 24, batch_size=3, **kw)
    assert isinstance(out, torch.Tensor) and out.device == dev.device and out.dtype == torch.uint8
    assert infos == rinfos and np.array_equal(out.cpu().numpy(), np.stack(refs))
    tout, tinfos = eng.run_until_stable(dev, 24, check_every=8)
    assert tout.is_cuda and tinfos == rinfos and np.array_equal(tout.cpu().numpy(), np.stack(refs))
    assert eng.residual(dev).tolist() == eng.residual(stack).tolist()
    out, infos = pconv_mod.convolve_batch_until_stable(dev[:0], 24, **kw)
    assert out.is_cuda and tuple(out.shape) == (0,) + stack.shape[1:] and infos == []
    assert pconv_mod.residual_batch(dev[:0], filt, backend="hip", border=border).shape == (0,)
    # the default interval is 16 x fuse: every image stops at the next multiple of 64
    _, long_ = oracle(pconv_mod, c, h, w, filt, border, 400, 8)
    _, dinfos = eng.run_until_stable(stack, 400)
    for b in range(n):
        assert dinfos[b].converged and dinfos[b].reps_done == -(-long_[b].reps_done // 64) * 64, b
        assert dinfos[b].checks == dinfos[b].reps_done // 64 and dinfos[b].residual == 0, b
    _, pinfos = pconv_mod.convolve_batch_until_stable(stack, 400, filt, backend="hip", fuse=4, border=border)
    assert pinfos == dinfos
    assert len(stencil._BATCH_ENGINES) <= 2
    with pytest.raises(ValueError, match="max_reps"):
        eng.run_until_stable(stack, -1)
    with pytest.raises(ValueError, match="check_every"):
        eng.run_until_stable(stack, 8, check_every=0)
    with pytest.raises(ValueError, match="capacity"):
        eng.run_until_stable(np.concatenate([stack, stack]), 8)
