"""Replicate border on a real MI355X: the fused kernels (both SWAR tile
kernels in both step forms, the float temporal kernel in every tile shape)
bit-exact against the NumPy oracle / the CPU fused reference at the places the
border code can go wrong — the image's last pixel on a strip's last byte, on a
strip's first byte, across two strips, across two lanes; the image's first
and last row on a wave's first, last and interior register row; one- and
two-pixel images — then routing, band frames, the engines, the pipeline, the
one-device cluster, row streaming and two ranks over shm / ipc.

Shapes are forced and tuning is off: no case spends time tuning.  Every
launch is checked for writes outside the frame (canaries), into the pad
columns and outside the requested rows."""
import json
import subprocess

import numpy as np
import pytest

from conftest import CONV_BIN

pytestmark = pytest.mark.gpu

GUARD = 4096
CANARY = 0xA5
CH = {"grey": 1, "rgb": 3, "rgba": 4}
NAME = {1: "grey", 3: "rgb", 4: "rgba"}
NEG_TAPS = ([3, 1, 0, 2, 5, 1, -1, 2, 4], 17)  # the negative-tap custom filter of test_gpu_kernels.py

_REF = {}   # (filter key, c, h, w, steps) -> oracle result, shared by every case that needs it
_IMG = {}


def _image(c, h, w):
    key = (c, h, w)
    if key not in _IMG:
        rng = np.random.default_rng(1000003 * c + 1009 * h + w)
        _IMG[key] = rng.integers(0, 256, size=(h, w, c) if c > 1 else (h, w), dtype=np.uint8)
    return _IMG[key]


def _oracle(pconv_mod, fkey, filt, c, h, w, steps):
    key = (fkey, c, h, w, steps)
    if key not in _REF:
        _REF[key] = pconv_mod.numpy_convolve(_image(c, h, w), steps, filt, border="replicate")
    return _REF[key]


def _launch(native, frame_rows, rb, h, halo, filt, c, r0, r1, steps, g_row0, height, variant, border="replicate"):
    """One launch on a frame given as (h + 2 halo, row_bytes) rows (ghost rows
    included); returns the destination frame as (h + 2 halo, pitch) after the
    canary / pad-column / outside-rows checks."""
    import torch

    lay = native.frame_layout(rb, h, halo)
    full = np.zeros((h + 2 * halo, lay["pitch"]), np.uint8)
    full[:, 16:16 + rb] = frame_rows
    bufs = []
    for _ in range(2):
        b = torch.full((lay["bytes"] + 2 * GUARD,), CANARY, dtype=torch.uint8, device="cuda")
        b[GUARD:GUARD + lay["bytes"]] = 0
        bufs.append(b)
    src, dst = bufs
    src[GUARD:GUARD + lay["bytes"]] = torch.from_numpy(full.reshape(-1)).cuda()
    base = lay["pitch"] * halo + 16
    native.launch_stencil(filt, NAME[c], src.data_ptr() + GUARD + base, dst.data_ptr() + GUARD + base, lay["pitch"],
                          rb, r0, r1, -halo, h + halo, steps, g_row0, height,
                          torch.cuda.current_stream().cuda_stream, variant, border=border)
    torch.cuda.synchronize()
    d = dst.cpu().numpy()
    assert (d[:GUARD] == CANARY).all() and (d[-GUARD:] == CANARY).all(), "write outside the frame"
    dv = d[GUARD:-GUARD].reshape(h + 2 * halo, lay["pitch"])
    assert (dv[:, :16] == 0).all() and (dv[:, 16 + rb:] == 0).all(), "write into the pad columns"
    lo, hi = max(r0, -g_row0), min(r1, height - g_row0)
    outside = np.ones(h + 2 * halo, bool)
    outside[halo + lo:halo + hi] = False
    assert (dv[outside] == 0).all(), "write outside the requested rows"
    assert np.array_equal(src.cpu().numpy()[GUARD:-GUARD], full.reshape(-1)), "the source frame was modified"
    return dv, full


def _whole(native, pconv_mod, fkey, filt, c, h, w, steps, variant, nfilt=None):
    """The whole image in one launch against the oracle; `filt` names the
    filter for the oracle, `nfilt` (default: the same) for the native launch.
    Returns the mismatching case (empty: bit-exact), so that a test reports
    every failing geometry of its sweep at once."""
    img = _image(c, h, w)
    rb = w * c
    halo = steps
    rows = np.zeros((h + 2 * halo, rb), np.uint8)
    rows[halo:halo + h] = img.reshape(h, rb)
    dv, _ = _launch(native, rows, rb, h, halo, filt if nfilt is None else nfilt, c, 0, h, steps, 0, h, variant)
    got = dv[halo:halo + h, 16:16 + rb].reshape(img.shape)
    ref = _oracle(pconv_mod, fkey, filt, c, h, w, steps)
    if np.array_equal(got, ref):
        return []
    return [(fkey, variant, c, h, w, steps, np.argwhere(got != ref)[:3].tolist())]


def _control(native, pconv_mod, fkey, filt, c, variant, nfilt=None, w=8):
    """The forced kernel under the zero border still gives the zero-border
    bytes, and those differ from the replicate oracle: the sweeps above compare
    real launches with the right reference."""
    h, steps = 5, 2
    img = _image(c, h, w)
    rb = w * c
    rows = np.zeros((h + 2 * steps, rb), np.uint8)
    rows[steps:steps + h] = img.reshape(h, rb)
    dv, _ = _launch(native, rows, rb, h, steps, filt if nfilt is None else nfilt, c, 0, h, steps, 0, h, variant,
                    border="zero")
    got = dv[steps:steps + h, 16:16 + rb].reshape(img.shape)
    assert np.array_equal(got, pconv_mod.numpy_convolve(img, steps, filt))
    assert not np.array_equal(got, _oracle(pconv_mod, fkey, filt, c, h, w, steps))
    assert not _whole(native, pconv_mod, fkey, filt, c, h, w, steps, variant, nfilt=nfilt)


def _widths(c, strip, lane_bytes, dword_rows):
    """Pixel widths that put the image's last pixel (c bytes) on a strip's last
    byte, on a strip's first byte, across two strips and (c > 1) across two
    lanes inside a strip — each where the pixel size allows it within three
    strips — plus one- and two-pixel rows and rows of whole and of partial
    dwords.  `strip` = valid bytes per strip of the forced tile.  dword_rows
    (the buffer-op kernel's contract): only rows of whole dwords, so the last
    pixel always ends a lane; it ends a strip, or follows a strip's first dword."""
    if dword_rows:
        q = c * 4 if c % 4 else c  # lcm(c, 4)
        k = next(k for k in (1, 2, 3) if (k * strip) % q == 0)
        rbs = {q, 2 * q, k * strip - q, k * strip, k * strip + q}
        if c == 4:
            rbs.add(strip + c)  # begins on the second strip's first byte
        return sorted(rb // c for rb in rbs if rb > 0)
    k = next(k for k in (1, 2, 3) if (k * strip) % c == 0)
    rbs = {c, 2 * c, k * strip, k * strip + c}
    for b in (strip, 2 * strip):  # across two strips
        rbs.update(rb for rb in range(b + 1, b + c) if rb % c == 0)
    # across two lanes, inside the first strip (a 4-byte pixel never does: lanes hold 4 or 8 bytes)
    rbs.update([rb for rb in range(c, strip, c) if (rb - c) // lane_bytes != (rb - 1) // lane_bytes][:1])
    rbs.add(next(rb for rb in range(3 * c, 12 * c, c) if rb % 4 == 0))
    if c != 4:
        rbs.add(next(rb for rb in range(3 * c, 12 * c, c) if rb % 4 != 0))
    return sorted(rb // c for rb in rbs)


def _heights(steps, m, vrows):
    """Image heights that put the last row on a wave's first, last and an
    interior register row (global row 0 sits on register row steps % m: the
    step counts cover its three cases), one- and two-row images, and one image
    of two tiles."""
    hs = {1, 2}
    for target in {0, m - 1, 1 % m}:
        hs.add(next(h for h in range(3, 3 + m) if (steps + h - 1) % m == target))
    hs.add(vrows + 3)
    return sorted(hs)


# (kernel, step form, tile shape): forms 0 and 1 of k_swar on one 8-byte-lane
# shape and two 4-byte-lane shapes (one with 16 waves), and the buffer-op form.
SWAR_CASES = [("tile", f, s) for f in (0, 1) for s in ((8, 4, 8), (4, 3, 16), (4, 8, 8))] + \
             [("bufop", 0, (4, 8, 8)), ("bufop", 1, (4, 8, 8)), ("bufop", 1, (4, 12, 4))]


@pytest.fixture
def forced(native):
    import torch

    native.set_autotune(False)
    yield native
    torch.cuda.synchronize()
    native.set_prefetch_mode(-1)
    native.set_swar_shape(0, 0, 0)
    native.set_swar_alt(-1)
    native.set_float_shape(0, 0)
    native.set_autotune(True)
    native.clear_swar_tuning()


@pytest.mark.parametrize("channels", ["grey", "rgb", "rgba"])
@pytest.mark.parametrize("kernel,form,shape", SWAR_CASES)
def test_swar_replicate_bit_exact(pconv_mod, forced, kernel, form, shape, channels):
    native = forced
    c = CH[channels]
    lw, m, nw = shape
    native.set_swar_alt(form)
    native.set_swar_shape(lw, m, nw)
    native.set_prefetch_mode(1 if kernel == "bufop" else 0)
    ran, bad = 0, []
    for steps in (1, 2, 3, 8, 16):
        hl = -(-steps * c // lw)
        vrows = m * nw - 2 * steps
        if vrows <= 0 or 2 * hl >= 64:
            continue  # the forced shape cannot run this step count (the launch would fall back to the model's)
        strip = (64 - 2 * hl) * lw
        for w in _widths(c, strip, lw, kernel == "bufop"):
            for h in _heights(steps, m, vrows):
                bad += _whole(native, pconv_mod, "gaussian", "gaussian", c, h, w, steps, "temporal")
                ran += 1
    assert ran > 50
    assert not bad, (len(bad), ran, bad[:12])
    _control(native, pconv_mod, "gaussian", "gaussian", c, "temporal")


FT_SHAPES = [(16, 8), (8, 8), (16, 4), (8, 4), (4, 8)]


@pytest.mark.parametrize("channels", ["grey", "rgb", "rgba"])
@pytest.mark.parametrize("filt", ["box", "edge", "neg"])
@pytest.mark.parametrize("shape", FT_SHAPES)
def test_float_temporal_replicate_bit_exact(pconv_mod, forced, shape, filt, channels):
    native = forced
    c = CH[channels]
    m, nw = shape
    native.set_float_shape(m, nw)
    f = native.Filter.custom(NEG_TAPS[0], NEG_TAPS[1], "custom") if filt == "neg" else filt
    pf = pconv_mod.get_filter(NEG_TAPS) if filt == "neg" else filt
    bad = []
    for steps in (1, 3, 4):
        hl = -(-steps * c // 8)
        vrows = m * nw - 2 * steps
        strip = (64 - 2 * hl) * 8
        ws = set(_widths(c, strip, 8, False))
        for valid in (1, 4, 5, 8):  # bytes of the row's last 8-byte chunk (RGBA rows end on 4 or 8 only)
            ws.update([w for w in range(1, 40) if (w * c) % 8 == valid % 8][:1])
        hs = _heights(steps, m, vrows) if steps != 3 else [1, 2, m, m + 1]
        for w in sorted(ws):
            for h in hs:
                bad += _whole(native, pconv_mod, filt, pf, c, h, w, steps, "float_temporal", nfilt=f)
    assert not bad, (len(bad), bad[:12])
    _control(native, pconv_mod, filt, pf, c, "float_temporal", nfilt=f)


@pytest.mark.parametrize("filt", ["gaussian", "box", "edge", "neg", "int"])
def test_single_step_auto_routes_to_a_temporal_kernel(pconv_mod, native, filt):
    """steps == 1 with variant auto: the single-step kernels know only the
    frame's zero pad, so replicate runs on the temporal kernels — and matches."""
    int_taps = ([1, 0, 3, 2, 4, 0, 1, 3, 2], 16)  # int_exact, not the gaussian: bit-identical in the float kernel
    taps = {"neg": NEG_TAPS, "int": int_taps}.get(filt)
    nf = native.Filter.custom(taps[0], taps[1], "custom") if taps else filt
    pf = pconv_mod.get_filter(taps) if taps else filt
    bad = []
    for c in (1, 3, 4):
        for (h, w) in [(1, 1), (5, 1), (1, 5), (17, 16), (31, 100)]:
            bad += _whole(native, pconv_mod, filt, pf, c, h, w, 1, "auto", nfilt=nf)
    assert not bad, bad


@pytest.mark.parametrize("variant", ["binomial", "int9", "float9"])
def test_single_step_variants_reject_replicate(native, variant):
    import torch

    lay = native.frame_layout(64, 8, 1)
    src = torch.zeros(lay["bytes"], dtype=torch.uint8, device="cuda")
    dst = torch.zeros(lay["bytes"], dtype=torch.uint8, device="cuda")
    base = lay["pitch"] + 16
    with pytest.raises(RuntimeError, match="border 'replicate' not supported by kernel '%s'" % variant):
        native.launch_stencil("gaussian", "grey", src.data_ptr() + base, dst.data_ptr() + base, lay["pitch"], 64, 0, 8,
                              -1, 9, 1, 0, 8, 0, variant, border="replicate")
    with pytest.raises(RuntimeError, match="not supported by kernel"):
        native.BandEngine(16, 8, "grey", "gaussian", variant=variant, border="replicate")
    with pytest.raises(RuntimeError, match="unknown border"):
        native.BandEngine(16, 8, "grey", "gaussian", border="mirror")
    torch.cuda.synchronize()
    assert int(dst.max()) == 0


@pytest.mark.parametrize("filt,variant", [("gaussian", "temporal"), ("gaussian", "auto"), ("box", "float_temporal"),
                                          ("edge", "auto")])
@pytest.mark.parametrize("steps", [1, 3, 8])
def test_band_frames_against_cpu_fused_launch(native, filt, variant, steps):
    """Band frames of a taller image: a band edge that is no image edge behaves
    as ever, ghost rows outside the image hold 0xEE and are ignored, partial
    [r0, r1).  Reference: cpu_fused_launch on the same frame."""
    H, h, w, c, halo = 100, 30, 45, 3, 8
    rb = w * c
    rng = np.random.default_rng(7 * steps + len(filt))
    for g_row0 in (0, 35, H - h, -3, H - h + 4):
        # g_row0 < 0 / > H - h: frames whose OWNED rows reach past the image, too
        rows = np.full((h + 2 * halo, rb), 0xEE, np.uint8)
        for fr in range(-halo, h + halo):
            if 0 <= g_row0 + fr < H:
                rows[halo + fr] = rng.integers(0, 256, rb, dtype=np.uint8)
        for (r0, r1) in [(0, h), (-(halo - steps), h + (halo - steps)), (steps, h - steps), (-3, 5), (h - 2, h + 1),
                         (7, 8)]:
            if r0 - steps < -halo or r1 + steps > h + halo or r0 >= r1:
                continue
            gpu, full = _launch(native, rows, rb, h, halo, filt, c, r0, r1, steps, g_row0, H, variant)
            cpu = np.zeros_like(full)
            native.cpu_fused_launch(filt, "rgb", rb, h, halo, full.reshape(-1), cpu.reshape(-1), r0, r1, steps, g_row0,
                                    H, border="replicate")
            lo, hi = max(r0, -g_row0), min(r1, H - g_row0)
            assert np.array_equal(gpu[halo + lo:halo + hi], cpu[halo + lo:halo + hi]), (g_row0, r0, r1, steps)


def test_engines_replicate_then_zero_in_one_process(pconv_mod, rng):
    """61x97 RGB, 40 repetitions through four entries — numpy in, cuda tensor
    in, a captured rep-loop graph, a BandPipeline step graph — each equal to the
    oracle, and a zero-border engine of the same geometry afterwards still
    returns the zero-border bytes (kernels, tuned shapes and caches are shared
    across borders; results are not)."""
    import torch
    from pconv.parallel.dist_engine import DistributedBlur

    w, h, reps = 61, 97, 40
    img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    rep = pconv_mod.numpy_convolve(img, reps, border="replicate")
    zero = pconv_mod.numpy_convolve(img, reps)
    assert not np.array_equal(rep, zero)

    def pipeline(border):
        blur = DistributedBlur(w, h, "rgb", "gaussian", reps, rank=0, world=1, device=0, slots=2, step_graphs=True,
                               border=border)
        assert blur.pipe.graphs and blur.pipe.step_graphs
        blur.load_image(img)
        return blur.step(reps).reshape(h, w, 3)

    entries = {
        "numpy": lambda b: pconv_mod.convolve(img, reps, backend="hip", border=b),
        "tensor": lambda b: pconv_mod.convolve(torch.from_numpy(img).cuda(), reps, border=b).cpu().numpy(),
        "graph": lambda b: pconv_mod.convolve(img, reps, backend="hip", graph=True, border=b),
        "pipeline": pipeline,
    }
    for name, run in entries.items():
        assert np.array_equal(run("replicate"), rep), name
        assert np.array_equal(run("zero"), zero), name
        assert np.array_equal(run("replicate"), rep), name
    pipe = pconv_mod.FilterPipeline.from_spec("gaussian:7,box:2,edge:1")
    assert np.array_equal(pipe.apply(img, backend="hip", border="replicate"), pipe.reference(img, border="replicate"))
    const = np.full((h, w, 3), 200, np.uint8)
    assert (pconv_mod.convolve(const, reps, backend="hip", border="replicate") == 200).all()


@pytest.mark.parametrize("filt,halo,fuse", [("gaussian", 4, 4), ("gaussian", 1, 1), ("box", 3, 3)])
def test_local_cluster_replicate(pconv_mod, rng, filt, halo, fuse):
    n = pconv_mod.native
    img = rng.integers(0, 256, size=(50, 45, 3), dtype=np.uint8)
    cl = n.LocalCluster(45, 50, "rgb", filt, 3, 0, halo, fuse, border="replicate")
    for reps, preload in ((1, False), (13, True)):
        cl.upload(img.reshape(-1), preload)
        cl.run(reps)
        out = np.empty_like(img)
        cl.download(out.reshape(-1))
        assert np.array_equal(out, pconv_mod.numpy_convolve(img, reps, filt, border="replicate")), reps


@pytest.mark.parametrize("mode", ["direct", "head"])
def test_row_streamed_image_replicate(pconv_mod, rng, mode):
    from pconv.parallel.dist_engine import DistributedBlur

    w, h, reps = 67, 133, 21
    blur = DistributedBlur(w, h, "rgb", "gaussian", reps, device=0, slots=2, stream_chunks=4, stream_min_bytes=0,
                           step_graphs=None if mode == "head" else False, border="replicate")
    assert len(blur.engine.stream_plan(reps, 0, h).chunks) == 4
    img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    blur.load_image(img)
    out = blur.step(reps).reshape(h, w, 3)
    if mode == "head":
        assert blur.pipe.streamed_heads >= 1
    assert np.array_equal(out, pconv_mod.numpy_convolve(img, reps, border="replicate"))


@pytest.mark.parametrize("extra", [[], ["--graph"], ["--filter", "box"], ["--gpus", "2", "--transport", "shm"],
                                   ["--gpus", "2", "--transport", "ipc", "--exchange-halo"]])
def test_cli_replicate_check(pconv_mod, tmp_path, rng, extra):
    """`conv img.raw 64 48 20 rgb --border replicate --check`: one GPU, and two
    ranks on one GPU over the shm and the ipc transport."""
    img = rng.integers(0, 256, size=(48, 64, 3), dtype=np.uint8)
    pconv_mod.write_raw(str(tmp_path / "img.raw"), img)
    r = subprocess.run([CONV_BIN, "img.raw", "64", "48", "20", "rgb", "--border", "replicate", "--check", "--json",
                        "--explain", "--timeout", "30"] + extra, cwd=tmp_path, capture_output=True, text=True,
                       timeout=150)
    assert r.returncode == 0, r.stderr
    meta = json.loads(r.stdout.strip().splitlines()[-1])
    assert meta["mismatches"] == 0 and meta["border"] == "replicate"
    filt = extra[extra.index("--filter") + 1] if "--filter" in extra else "gaussian"
    out = pconv_mod.read_raw(str(tmp_path / "blur_img.raw"), 64, 48, "rgb")
    assert np.array_equal(out, pconv_mod.numpy_convolve(img, 20, filt, border="replicate"))
