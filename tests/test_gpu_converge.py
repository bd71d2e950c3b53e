"""The residual kernel and the run to the fixed point on a real MI355X.

The kernel's count against the NumPy oracle's at the row widths and heights
where its tail mask, its lane / workgroup boundaries and its row march can go
wrong; fixed points give exactly zero and one changed byte gives the oracle's
count; band frames with garbage beyond the image edge; nothing but the counter
is written (canaries, pads, the frame itself); the engine's run_until_stable
against the NumPy backend; two ranks on one GPU over shm and ipc.

Exact integers and exact bytes only.  Tuning is off and fuse is forced."""
import json
import subprocess

import numpy as np
import pytest

from conftest import CONV_BIN

pytestmark = pytest.mark.gpu

GUARD = 4096
CANARY = 0xA5
NAME = {1: "grey", 3: "rgb", 4: "rgba"}
NEG_TAPS = ([3, 1, 0, 2, 5, 1, -1, 2, 4], 17)  # the negative-tap custom filter of test_gpu_kernels.py
FILTERS = ["gaussian", "box", "edge", "neg"]
BORDERS = ["zero", "replicate"]

_IMG = {}
_FIX = {}


def _filters(pconv_mod, filt):
    if filt == "neg":
        return pconv_mod.get_filter(NEG_TAPS), pconv_mod.native.Filter.custom(NEG_TAPS[0], NEG_TAPS[1], "custom")
    return filt, filt


def _image(c, h, w):
    key = (c, h, w)
    if key not in _IMG:
        rng = np.random.default_rng(1000003 * c + 1009 * h + w)
        _IMG[key] = rng.integers(0, 256, size=(h, w, c) if c > 1 else (h, w), dtype=np.uint8)
    return _IMG[key]


def _fixed_point(pconv_mod, c, h, w, filt, border):
    """The oracle's fixed point of a random image (computed once per case)."""
    key = (c, h, w, filt, border)
    if key not in _FIX:
        x = _image(c, h, w)
        for _ in range(2000):
            nxt = pconv_mod.ops.reference.numpy_step(x, filt, border)
            if np.array_equal(nxt, x):
                break
            x = nxt
        assert pconv_mod.numpy_residual(x, filt, border) == 0
        _FIX[key] = x
    return _FIX[key]


def _canary_frame(native, frame_rows, rb, h, halo):
    """A frame given as (h + 2 halo, row_bytes) rows (ghost rows included) on
    the device, zero pad columns, canaries around it: the buffer, its layout
    and the address of (row 0, column 0)."""
    import torch

    lay = native.frame_layout(rb, h, halo)
    full = np.zeros((h + 2 * halo, lay["pitch"]), np.uint8)
    full[:, 16:16 + rb] = frame_rows
    buf = torch.full((lay["bytes"] + 2 * GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    buf[GUARD:GUARD + lay["bytes"]] = torch.from_numpy(full.reshape(-1)).cuda()
    return buf, lay, buf.data_ptr() + GUARD + lay["pitch"] * halo + 16


def _count(native, frame_rows, rb, h, halo, filt, c, r0, r1, g_row0, height, border):
    """The kernel's count on such a frame, after checking that it wrote
    nothing: the canaries around the frame, the pad columns and the frame
    itself are unchanged."""
    import torch

    src, lay, row0 = _canary_frame(native, frame_rows, rb, h, halo)
    before = src.cpu().numpy().copy()
    torch.cuda.synchronize()
    n = native.launch_residual(filt, NAME[c], row0, lay["pitch"], rb, r0, r1, -halo, h + halo,
                               g_row0, height, torch.cuda.current_stream().cuda_stream, border=border)
    torch.cuda.synchronize()
    after = src.cpu().numpy()
    assert (after[:GUARD] == CANARY).all() and (after[-GUARD:] == CANARY).all(), "write outside the frame"
    assert np.array_equal(after, before), "the kernel wrote into the frame"
    return int(n)


def _whole(native, pconv_mod, img, filt, border):
    """Kernel count of a whole image (one ghost row either side, holding
    garbage: outside the image nothing may be read as data)."""
    pf, nf = _filters(pconv_mod, filt)
    h, w = img.shape[:2]
    c = 1 if img.ndim == 2 else img.shape[2]
    rb = w * c
    rows = np.full((h + 2, rb), 0xEE, np.uint8)
    rows[1:1 + h] = img.reshape(h, rb)
    return _count(native, rows, rb, h, 1, nf, c, 0, h, 0, h, border), pconv_mod.numpy_residual(img, pf, border)


def _widths(c):
    """Pixel widths whose row bytes sit below, at (where c divides it) and
    above one 16-byte chunk and one workgroup's 64 lanes x 16 bytes; one pixel;
    for RGB also W = 11, whose last pixel straddles two chunks."""
    ws = {1}
    for edge in (16, 1024):
        ws.update({(edge - 1) // c, -(-edge // c), edge // c + 1})
    if c == 3:
        ws.add(11)
    return sorted(x for x in ws if x >= 1)


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("filt", FILTERS)
def test_kernel_count_equals_oracle(pconv_mod, native, filt, border):
    rows_wg = native.RESIDUAL_BLOCK_ROWS
    bad, ran = [], 0
    for c in (1, 3, 4):
        if c == 1:
            assert {1, 15, 16, 17, 1023, 1024, 1025} <= set(_widths(1))
        for w in _widths(c):
            for h in (1, 2, rows_wg + 1):
                got, want = _whole(native, pconv_mod, _image(c, h, w), filt, border)
                ran += 1
                if got != want:
                    bad.append((c, h, w, got, want))
    assert ran >= 60
    assert not bad, (len(bad), bad[:12])


def _step_changes(native, img, filt, c, variant):
    """Bytes of [0, row_bytes) that one single-step launch_stencil changes
    (zero border, one garbage ghost row either side as in _whole)."""
    import torch

    h, rb = img.shape[0], img.shape[1] * c
    rows = np.full((h + 2, rb), 0xEE, np.uint8)
    rows[1:1 + h] = img.reshape(h, rb)
    src, lay, s0 = _canary_frame(native, rows, rb, h, 1)
    dst, _, d0 = _canary_frame(native, np.zeros((h + 2, rb), np.uint8), rb, h, 1)
    native.launch_stencil(filt, NAME[c], s0, d0, lay["pitch"], rb, 0, h, -1, h + 1, 1, 0, h,
                          torch.cuda.current_stream().cuda_stream, variant)
    torch.cuda.synchronize()
    d = dst.cpu().numpy()
    assert (d[:GUARD] == CANARY).all() and (d[-GUARD:] == CANARY).all(), "write outside the frame"
    out = d[GUARD:GUARD + lay["bytes"]].reshape(h + 2, lay["pitch"])[1:1 + h, 16:16 + rb]
    return int(np.count_nonzero(out != rows[1:1 + h]))


@pytest.mark.parametrize("filt,variant", [("gaussian", "int9"), ("box", "float9"), ("neg", "float9")])
def test_residual_counts_what_the_single_step_changes(pconv_mod, native, filt, variant):
    """The two users of the nine-tap core agree: launch_residual's count is the
    number of bytes k_generic9 changes, and both are the oracle's.  Row bytes
    17, 31, 32, 33, 35, 36 end the row at different places of a lane's 24-byte
    window (nearest whole pixels for 3 and 4 channels); 1029 crosses a
    workgroup in x."""
    pf, nf = _filters(pconv_mod, filt)
    bad, ran = [], 0
    for c in (1, 3, 4):
        ws = sorted({max(1, round(rb / c)) for rb in (17, 31, 32, 33, 35, 36)} | ({1029} if c == 1 else set()))
        if c == 1:
            assert ws == [17, 31, 32, 33, 35, 36, 1029]
        for w in ws:
            for h in (1, 2, native.RESIDUAL_BLOCK_ROWS + 1):
                img = _image(c, h, w)
                got, want = _whole(native, pconv_mod, img, filt, "zero")
                stepped = _step_changes(native, img, nf, c, variant)
                ran += 1
                if not got == stepped == want:
                    bad.append((c, h, w, got, stepped, want))
    assert ran == 3 * (7 + 4 + 3)
    assert not bad, (len(bad), bad[:12])


@pytest.mark.parametrize("border", BORDERS)
def test_many_workgroups_add_to_one_counter(pconv_mod, native, border):
    """70x2100 and 330x4100 grey, random (nearly every byte changes): 9 and 55
    workgroups' atomics land on the one counter."""
    for (h, w) in [(70, 2100), (330, 4100)]:
        for filt in ("gaussian", "box"):
            got, want = _whole(native, pconv_mod, _image(1, h, w), filt, border)
            assert got == want and want > h * w // 2, (h, w, filt)


@pytest.mark.parametrize("c,h,w,filt", [(1, 9, 13, "gaussian"), (3, 21, 13, "box"), (3, 21, 13, "gaussian")])
@pytest.mark.parametrize("border", BORDERS)
def test_zero_is_exactly_zero(pconv_mod, native, border, c, h, w, filt):
    fix = _fixed_point(pconv_mod, c, h, w, filt, border)
    if border == "zero":
        assert not fix.any()
    else:
        assert fix.any()
    got, want = _whole(native, pconv_mod, fix, filt, border)
    assert got == want == 0
    rb = w * c
    flat_positions = [0, h * rb - 1, 15 if rb > 15 else rb - 1]  # first byte, last byte, last byte of a 16-byte chunk
    for pos in flat_positions:
        x = fix.copy()
        x.reshape(-1)[pos] ^= 0x80
        got, want = _whole(native, pconv_mod, x, filt, border)
        assert got == want and want > 0, (pos, got, want)


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("filt", ["gaussian", "box", "neg"])
def test_band_frames(pconv_mod, native, filt, border):
    """Top, middle and bottom band of a 40-row image, halo 3: ghost rows beyond
    the image edge hold 0xEE, a band edge inside the image reads its ghost
    row; each count is the oracle's over the band's rows and the three sum to
    the image's."""
    pf, nf = _filters(pconv_mod, filt)
    H, w, c, halo = 40, 15, 3, 3
    rb = w * c
    img = _image(c, H, w)
    flat = img.reshape(H, rb)
    step = pconv_mod.numpy_convolve(img, 1, pf, border).reshape(H, rb)
    total = 0
    for (y0, rows) in [(0, 13), (13, 14), (27, 13)]:
        frame = np.full((rows + 2 * halo, rb), 0xEE, np.uint8)
        for fr in range(-halo, rows + halo):
            if 0 <= y0 + fr < H:
                frame[halo + fr] = flat[y0 + fr]
        got = _count(native, frame, rb, rows, halo, nf, c, 0, rows, y0, H, border)
        assert got == int(np.count_nonzero(step[y0:y0 + rows] != flat[y0:y0 + rows])), (y0, rows)
        total += got
        # two ghost rows either side as well: those beyond the image are clipped, not counted
        lo, hi = max(y0 - 2, 0), min(y0 + rows + 2, H)
        assert _count(native, frame, rb, rows, halo, nf, c, -2, rows + 2, y0, H, border) == \
            int(np.count_nonzero(step[lo:hi] != flat[lo:hi])), (y0, rows)
    assert total == pconv_mod.numpy_residual(img, pf, border)


def test_launch_residual_rejects_rows_outside_the_frame(native):
    import torch

    lay = native.frame_layout(64, 8, 1)
    src = torch.zeros(lay["bytes"], dtype=torch.uint8, device="cuda")
    base = lay["pitch"] + 16
    with pytest.raises(RuntimeError, match="exceed frame"):
        native.launch_residual("gaussian", "grey", src.data_ptr() + base, lay["pitch"], 64, 0, 9, -1, 9, 0, 100)
    with pytest.raises(RuntimeError, match="pitch too small"):
        native.launch_residual("gaussian", "grey", src.data_ptr() + base, 64, 64, 0, 8, -1, 9, 0, 8)


@pytest.fixture
def untuned(native):
    import torch

    native.set_autotune(False)
    yield native
    torch.cuda.synchronize()
    native.set_autotune(True)
    native.clear_swar_tuning()


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("c,h,w,filt", [(1, 9, 13, "gaussian"), (3, 21, 13, "box")])
def test_engine_run_until_stable(pconv_mod, untuned, c, h, w, filt, border, graph):
    import torch

    img = _image(c, h, w)
    eng = pconv_mod.Engine(w, h, NAME[c], filt, fuse=4, graph=graph, border=border)
    assert eng.fuse == 4
    ref, rinfo = pconv_mod.convolve_until_stable(img, 400, filt, check_every=8, backend="numpy", border=border)
    assert rinfo.converged and rinfo.reps_done % 8 == 0
    out, info = eng.run_until_stable(img, 400, check_every=8)
    assert info == rinfo
    assert np.array_equal(out, ref)
    assert eng.residual() == 0
    # a CUDA tensor in, a CUDA tensor out
    tout, tinfo = eng.run_until_stable(torch.from_numpy(img).cuda(), 400, check_every=8)
    assert tout.is_cuda and tinfo == rinfo and np.array_equal(tout.cpu().numpy(), ref)
    # the maximum first: the count describes the returned image, and the resident frame
    ref10, rinfo10 = pconv_mod.convolve_until_stable(img, 10, filt, check_every=8, backend="numpy", border=border)
    out10, info10 = eng.run_until_stable(img, 10, check_every=8)
    assert info10 == rinfo10 and not info10.converged and info10.reps_done == 10 and info10.checks == 2
    assert np.array_equal(out10, ref10)
    want = pconv_mod.numpy_residual(ref10, filt, border)
    assert eng.residual() == want == info10.residual > 0
    assert eng.residual(ref10) == want
    # the default interval is 16 x fuse; the public entry agrees
    _, dinfo = eng.run_until_stable(img, 400)
    # (the fixed point is first reached in (reps_done - 8, reps_done]: the next multiple of 64)
    assert dinfo.converged and dinfo.reps_done == -(-rinfo.reps_done // 64) * 64
    assert dinfo.checks == dinfo.reps_done // 64
    pout, pinfo = pconv_mod.convolve_until_stable(img, 400, filt, check_every=8, backend="hip", fuse=4, graph=graph,
                                                  border=border)
    assert pinfo == rinfo and np.array_equal(pout, ref)
    assert pconv_mod.residual(img, filt, backend="hip", border=border) == pconv_mod.numpy_residual(img, filt, border)


def _conv(args, cwd):
    r = subprocess.run([CONV_BIN] + args, cwd=cwd, capture_output=True, text=True, timeout=150)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1]), r.stderr


def test_cli_one_gpu_and_two_ranks_on_it(pconv_mod, tmp_path):
    """24x20 RGB, replicate, --converge-every 8: one GPU against the oracle
    (--check), then two ranks on the one GPU over shm and over ipc — the same
    file, the same outcome, and no more exchanges than one per chunk plus one."""
    w, h = 24, 20
    img = _image(3, h, w)
    pconv_mod.write_raw(str(tmp_path / "img.raw"), img)
    base = ["img.raw", str(w), str(h), "400", "rgb", "--backend", "hip", "--border", "replicate", "--converge-every",
            "8", "--json", "--check", "--timeout", "30"]
    one, err = _conv(base + ["--out", "one.raw"], tmp_path)
    _, rinfo = pconv_mod.convolve_until_stable(img, 400, check_every=8, backend="numpy", border="replicate")
    assert one["mismatches"] == 0 and one["reps"] == 400
    assert (one["reps_done"], one["converged"], one["residual"]) == (rinfo.reps_done, True, 0)
    assert f"fixed point after {rinfo.reps_done} repetitions" in err
    ref = pconv_mod.read_raw(str(tmp_path / "one.raw"), w, h, "rgb")
    assert np.array_equal(ref, pconv_mod.numpy_convolve(img, 400, border="replicate"))
    for transport in ("shm", "ipc"):
        two, err = _conv(base + ["--gpus", "2", "--transport", transport, "--out", f"{transport}.raw"], tmp_path)
        assert two["mismatches"] == 0
        for k in ("reps", "reps_done", "converged", "residual"):
            assert two[k] == one[k], (transport, k)
        assert two["exchanges"] <= two["reps_done"] // 8 + 1, (transport, two["exchanges"])
        assert np.array_equal(pconv_mod.read_raw(str(tmp_path / f"{transport}.raw"), w, h, "rgb"), ref), transport
        assert f"fixed point after {rinfo.reps_done} repetitions" in err
    # the maximum first, with a graph-captured loop
    short, err = _conv(base[:3] + ["10"] + base[4:] + ["--graph", "--out", "short.raw"], tmp_path)
    want = pconv_mod.numpy_residual(pconv_mod.numpy_convolve(img, 10, border="replicate"), border="replicate")
    assert short["mismatches"] == 0 and short["reps_done"] == 10 and short["converged"] is False
    assert short["residual"] == want > 0
    assert f"no fixed point within 10 repetitions ({want} bytes still change)" in err
