"""Stopping at the fixed point, CPU side: the NumPy oracle's residual, the
native CPU residual (serial and OpenMP) against it along whole trajectories,
`convolve_until_stable`, the `conv --converge-every` CLI on the CPU backend
and the torchrun program on two ranks.

Every comparison is an exact integer or exact bytes; every expected value is
computed here by the NumPy oracle."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import CONV_BIN, ROOT

NEG_TAPS = ([3, 1, 0, 2, 5, 1, -1, 2, 4], 17)  # the negative-tap custom filter of test_gpu_kernels.py
FILTERS = ["gaussian", "box", "edge", "neg"]
BORDERS = ["zero", "replicate"]
SHAPES = [(1, 1), (1, 7), (7, 1), (9, 13), (21, 13)]
NAME = {1: "grey", 3: "rgb", 4: "rgba"}
MAX_STATES = 700  # the named filters reach their fixed point far below (21x13: < 200 repetitions)

_TRAJ = {}


def _filters(pconv_mod, filt):
    """(oracle filter, native filter) of a case name."""
    if filt == "neg":
        return pconv_mod.get_filter(NEG_TAPS), pconv_mod.native.Filter.custom(NEG_TAPS[0], NEG_TAPS[1], "custom")
    return filt, filt


def _image(c, h, w):
    rng = np.random.default_rng(7919 * c + 101 * h + w)
    return rng.integers(0, 256, size=(h, w, c) if c > 1 else (h, w), dtype=np.uint8)


def _trajectory(pconv_mod, filt, border, c, h, w):
    """[(state, oracle residual)] from the image to its fixed point (or to
    MAX_STATES states), computed once per case."""
    key = (filt, border, c, h, w)
    if key not in _TRAJ:
        pf, _ = _filters(pconv_mod, filt)
        x = _image(c, h, w)
        states = []
        while len(states) < MAX_STATES:
            nxt = pconv_mod.ops.reference.numpy_step(x, pf, border)
            res = int(np.count_nonzero(nxt != x))
            states.append((x, res))
            if res == 0:
                break
            x = nxt
        _TRAJ[key] = states
    return _TRAJ[key]


def test_numpy_residual_is_its_definition(pconv_mod):
    for filt in FILTERS:
        pf, _ = _filters(pconv_mod, filt)
        for border in BORDERS:
            for c in (1, 3):
                img = _image(c, 9, 13)
                want = int(np.count_nonzero(pconv_mod.numpy_convolve(img, 1, pf, border) != img))
                assert pconv_mod.numpy_residual(img, pf, border) == want
                assert want > 0
    black = np.zeros((5, 6, 3), np.uint8)
    assert pconv_mod.numpy_residual(black) == 0
    const = np.full((5, 6), 77, np.uint8)
    assert pconv_mod.numpy_residual(const, border="replicate") == 0
    assert pconv_mod.numpy_residual(const, border="zero") > 0
    with pytest.raises(ValueError):
        pconv_mod.numpy_residual(black, border="mirror")


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("filt", FILTERS)
def test_cpu_residual_along_the_trajectory(pconv_mod, filt, border):
    """cpu_residual, serial and OpenMP, equals the oracle's count at EVERY
    state from the random image to the fixed point: large counts at the start,
    the small counts of the last states, and exactly 0 at the fixed point."""
    n = pconv_mod.native
    _, nf = _filters(pconv_mod, filt)
    for c in (1, 3, 4):
        for (h, w) in SHAPES:
            traj = _trajectory(pconv_mod, filt, border, c, h, w)
            if filt != "neg":
                assert traj[-1][1] == 0, ("no fixed point", filt, border, c, h, w)
            for i, (x, want) in enumerate(traj):
                for omp in (False, True):
                    got = n.cpu_residual(x.reshape(-1), w, h, NAME[c], nf, omp, 2 if omp else 0, border=border)
                    assert got == want, (filt, border, c, h, w, i, omp)
            if traj[-1][1] == 0:
                x = traj[-1][0]
                assert n.cpu_residual(x.reshape(-1), w, h, NAME[c], nf, False, 0, border=border) == 0
                if border == "zero" and filt != "neg":
                    assert not x.any()  # the zero border's fixed point is the black image
                if len(traj) > 1:
                    assert 0 < traj[-2][1] <= x.size


def test_cpu_residual_openmp_team(pconv_mod):
    """An image large enough for the OpenMP row loop to run as a team (the
    reduction over threads), both borders, against the oracle."""
    n = pconv_mod.native
    img = _image(3, 150, 131)
    for border in BORDERS:
        for filt in ("gaussian", "box"):
            want = pconv_mod.numpy_residual(img, filt, border)
            assert n.cpu_residual(img.reshape(-1), 131, 150, "rgb", filt, True, 3, border=border) == want
            assert pconv_mod.residual(img, filt, backend="omp", threads=3, border=border) == want
            assert pconv_mod.residual(img, filt, backend="cpu", border=border) == want
            assert pconv_mod.residual(img, filt, backend="numpy", border=border) == want


def test_cpu_frame_residual_ignores_ghost_rows_outside_the_image(pconv_mod):
    """A band frame: ghost rows beyond the image edge hold garbage and are
    read as zeros (zero border) or not at all (replicate); a band edge inside
    the image reads its ghost row.  The bands' counts sum to the image's."""
    n = pconv_mod.native
    H, w, c, halo = 30, 11, 3, 3
    rb = w * c
    img = _image(c, H, w).reshape(H, rb)
    for border in BORDERS:
        for filt in ("gaussian", "edge"):
            step = pconv_mod.numpy_convolve(img.reshape(H, w, c), 1, filt, border).reshape(H, rb)
            total = 0
            for (y0, rows) in [(0, 10), (10, 12), (22, 8)]:
                lay = n.frame_layout(rb, rows, halo)
                frame = np.zeros((rows + 2 * halo, lay["pitch"]), np.uint8)
                for fr in range(-halo, rows + halo):
                    g = y0 + fr
                    frame[halo + fr, 16:16 + rb] = img[g] if 0 <= g < H else 0xEE
                got = n.cpu_frame_residual(filt, "rgb", rb, rows, halo, frame.reshape(-1), 0, rows, y0, H, False,
                                           border=border)
                assert got == int(np.count_nonzero(step[y0:y0 + rows] != img[y0:y0 + rows])), (border, filt, y0)
                total += got
            assert total == pconv_mod.numpy_residual(img.reshape(H, w, c), filt, border)


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("c,h,w", [(1, 9, 13), (3, 21, 13)])
def test_convolve_until_stable_omp(pconv_mod, c, h, w, border):
    img = _image(c, h, w)
    traj = _trajectory(pconv_mod, "gaussian", border, c, h, w)
    assert traj[-1][1] == 0
    first = next(i for i, (_, res) in enumerate(traj) if res == 0)
    want_reps = -(-first // 8) * 8  # the first multiple of 8 at which the oracle's residual is 0
    assert 0 < want_reps <= 400
    for backend in ("omp", "cpu", "numpy"):
        out, info = pconv_mod.convolve_until_stable(img, 400, check_every=8, backend=backend, border=border)
        assert isinstance(info, pconv_mod.StableInfo)
        assert info.converged and info.residual == 0, backend
        assert info.reps_done == want_reps and info.checks == want_reps // 8, backend
        assert np.array_equal(out, pconv_mod.numpy_convolve(img, 400, "gaussian", border)), backend
        assert np.array_equal(out, pconv_mod.numpy_convolve(img, info.reps_done, "gaussian", border)), backend
    # the maximum reached first: not converged, the count describes the returned image
    plain = pconv_mod.numpy_convolve(img, 10, "gaussian", border)
    for backend in ("omp", "cpu", "numpy"):
        out, info = pconv_mod.convolve_until_stable(img, 10, check_every=8, backend=backend, border=border)
        assert not info.converged and info.reps_done == 10 and info.checks == 2, backend
        assert info.residual == traj[10][1] == pconv_mod.numpy_residual(plain, "gaussian", border) > 0, backend
        assert np.array_equal(out, plain), backend
    # the CPU backends' default interval
    out, info = pconv_mod.convolve_until_stable(img, 400, backend="omp", border=border)
    assert info.converged and info.reps_done == -(-first // 32) * 32
    with pytest.raises(ValueError):
        pconv_mod.convolve_until_stable(img, 10, check_every=0, backend="omp")
    with pytest.raises(ValueError):
        pconv_mod.convolve_until_stable(img, -1, backend="omp")


def test_stable_info_is_frozen(pconv_mod):
    info = pconv_mod.StableInfo(8, True, 0, 1)
    with pytest.raises(Exception):
        info.reps_done = 9


def _run(args, cwd):
    return subprocess.run([CONV_BIN] + args, cwd=cwd, capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("backend", ["cpu", "omp"])
def test_cli_converge_every(pconv_mod, tmp_path, backend):
    c, h, w = 3, 21, 13
    img = _image(c, h, w)
    pconv_mod.write_raw(str(tmp_path / "pic.raw"), img)
    traj = _trajectory(pconv_mod, "gaussian", "replicate", c, h, w)
    first = next(i for i, (_, res) in enumerate(traj) if res == 0)
    want = -(-first // 8) * 8
    base = ["pic.raw", str(w), str(h), "400", "rgb", "--backend", backend, "--border", "replicate"]
    r = _run(base + ["--converge-every", "8", "--json", "--check"], tmp_path)
    assert r.returncode == 0, r.stderr
    meta = json.loads(r.stdout.strip().splitlines()[-1])
    assert meta["reps"] == 400 and meta["reps_done"] == want and meta["converged"] is True and meta["residual"] == 0
    assert meta["mismatches"] == 0
    assert f"fixed point after {want} repetitions" in r.stderr
    out = pconv_mod.read_raw(str(tmp_path / "blur_pic.raw"), w, h, "rgb")
    assert np.array_equal(out, pconv_mod.numpy_convolve(img, 400, border="replicate"))
    assert out.any()  # the replicate border's fixed point is not black
    # the maximum reached first
    r = _run(base[:3] + ["10"] + base[4:] + ["--converge-every", "8", "--json", "--check"], tmp_path)
    assert r.returncode == 0, r.stderr
    meta = json.loads(r.stdout.strip().splitlines()[-1])
    assert meta["reps_done"] == 10 and meta["converged"] is False and meta["residual"] == traj[10][1] > 0
    assert meta["mismatches"] == 0
    assert f"no fixed point within 10 repetitions ({traj[10][1]} bytes still change)" in r.stderr
    assert np.array_equal(pconv_mod.read_raw(str(tmp_path / "blur_pic.raw"), w, h, "rgb"),
                          pconv_mod.numpy_convolve(img, 10, border="replicate"))
    # --quiet drops the line; without the flag the JSON has none of the keys
    r = _run(base + ["--converge-every", "8", "--quiet"], tmp_path)
    assert r.returncode == 0 and "fixed point" not in r.stderr and r.stdout == ""
    r = _run(base[:3] + ["10"] + base[4:] + ["--json"], tmp_path)
    assert r.returncode == 0 and "fixed point" not in r.stderr
    meta = json.loads(r.stdout.strip().splitlines()[-1])
    assert not {"reps_done", "converged", "residual"} & set(meta)


def test_cli_converge_every_validation(tmp_path):
    base = ["s.raw", "8", "8", "4", "grey", "--synthetic", "1", "--backend", "cpu"]
    for bad in ("0", "-3", "x"):
        r = _run(base + ["--converge-every", bad], tmp_path)
        assert r.returncode == 1 and "invalid --converge-every" in r.stderr, bad
    r = _run(base + ["--converge-every"], tmp_path)
    assert r.returncode == 1 and "missing value for --converge-every" in r.stderr
    r = _run(base + ["--converge-every", "2", "--checkpoint-every", "2"], tmp_path)
    assert r.returncode == 1 and "--converge-every cannot be combined with --checkpoint-every" in r.stderr
    r = _run(["--help"], tmp_path)
    assert r.returncode == 0 and "--converge-every K" in r.stdout


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _torchrun(world, args, cwd, timeout=240):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr", "127.0.0.1", f"--master-port={_free_port()}", "-m", "pconv.parallel.run"] + args
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2")
    return subprocess.run(cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=timeout)


def test_torchrun_converge_every(pconv_mod, tmp_path):
    """Two ranks (gloo halos, counts summed with the gloo all-reduce) stop at
    the same repetition as one rank and write the same file."""
    c, h, w = 3, 21, 13
    img = _image(c, h, w)
    pconv_mod.write_raw(str(tmp_path / "pic.raw"), img)
    traj = _trajectory(pconv_mod, "gaussian", "replicate", c, h, w)
    first = next(i for i, (_, res) in enumerate(traj) if res == 0)
    want = -(-first // 8) * 8
    files, metas = [], []
    for world in (1, 2):
        out = f"out{world}.raw"
        r = _torchrun(world, ["pic.raw", str(w), str(h), "400", "rgb", "--backend", "omp", "--border", "replicate",
                              "--converge-every", "8", "--json", "--check", "--out", out], tmp_path)
        assert r.returncode == 0, r.stderr[-3000:]
        meta = json.loads(r.stdout.strip().splitlines()[-1])
        assert meta["reps"] == 400 and meta["reps_done"] == want and meta["converged"] is True
        assert meta["residual"] == 0 and meta["mismatches"] == 0 and meta["ranks"] == world
        assert f"fixed point after {want} repetitions" in r.stderr
        files.append(pconv_mod.read_raw(str(tmp_path / out), w, h, "rgb"))
        metas.append(meta)
    assert np.array_equal(files[0], files[1])
    assert np.array_equal(files[0], pconv_mod.numpy_convolve(img, want, border="replicate"))
    r = _torchrun(1, ["pic.raw", str(w), str(h), "9", "rgb", "--backend", "omp", "--converge-every", "2",
                      "--checkpoint-every", "2"], tmp_path)
    assert r.returncode != 0 and "--converge-every cannot be combined with --checkpoint-every" in r.stderr
