"""bench.py's self-verification on the CPU (every BENCH line
must carry an oracle check).  The check is on by default in a --full run; each
rank's oracle is the CPU stencil of its band's dependency cone, which must
equal the rows of the whole-image oracle for every split, and the mismatch
count is what lands in the JSON line's "mismatches" field.  Also the plain
run (no --full): the headline only, and --dump-outputs."""
import importlib.util
import os
import sys
import types

import numpy as np
import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _args(bench, argv):
    old = sys.argv
    try:
        sys.argv = ["bench.py"] + argv
        return bench.parse()
    finally:
        sys.argv = old


def test_check_is_on_by_default(bench):
    assert _args(bench, []).check is True
    assert _args(bench, ["--check"]).check is True
    assert _args(bench, ["--no-check"]).check is False


def test_full_is_off_by_default(bench):
    """A plain run times the headline only; --full adds the check and the
    other figures after it (the check stays on by default there)."""
    a = _args(bench, ["--gpus", "1", "--steps", "5", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and (a.steps, a.warmup) == (5, 2)
    a = _args(bench, ["--full", "--dump-outputs", "some/dir"])
    assert a.full is True and a.check is True and a.dump_outputs == "some/dir"
    with pytest.raises(SystemExit):
        _args(bench, ["--native", "--dump-outputs", "some/dir"])


def test_dump_outputs_files(bench, tmp_path, monkeypatch):
    """--dump-outputs: float32 copies of the rows, one file per rank at N>1;
    an output over the size limit becomes the same seeded sample every time."""
    rows = np.random.default_rng(3).integers(0, 256, size=(7, 30), dtype=np.uint8)
    p = bench.dump_outputs(str(tmp_path / "a"), rows, 0, 1, 1234)
    assert p == str(tmp_path / "a" / "output.npy")
    got = np.load(p)
    assert got.dtype == np.float32 and np.array_equal(got, rows.astype(np.float32))
    assert bench.dump_outputs(str(tmp_path / "a"), rows, 2, 4, 1234).endswith("output_rank2.npy")
    assert bench.DUMP_LIMIT_BYTES <= 64 * 2 ** 20
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4 * 100)  # room for 100 float32 values in all
    s1 = np.load(bench.dump_outputs(str(tmp_path / "b"), rows, 0, 1, 1234))
    s2 = np.load(bench.dump_outputs(str(tmp_path / "c"), rows, 0, 1, 1234))
    assert s1.shape == (100,) and s1.nbytes <= 400 and np.array_equal(s1, s2)
    assert set(s1.tolist()) <= set(rows.reshape(-1).astype(np.float32).tolist())
    other = np.load(bench.dump_outputs(str(tmp_path / "d"), rows, 0, 1, 99))
    assert not np.array_equal(s1, other)  # the positions follow the seed
    half = np.load(bench.dump_outputs(str(tmp_path / "e"), rows, 1, 2, 1234))
    assert half.shape == (50,)  # every rank takes its share of the limit


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_step(pconv_mod, tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR`: the line
    keeps the contract's fields and carries none of the --full figures; the
    dumped rows are the oracle's, byte for byte (a small image: 3 images in
    flight over 7 steps, so the last step's slot is not slot 0)."""
    import json
    import subprocess

    w, h, reps = 157, 93, 9
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
           "--width", str(w), "--height", str(h), "--reps", str(reps), "--slots", "3", "--seed", "77",
           "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    meta = json.loads(lines[0])
    assert meta["steps"] == 7 and meta["ms_per_step"] > 0 and meta["value"] > 0 and meta["unit"] == "Mpix/s"
    assert meta["higher_is_better"] is True and meta["dtype"].startswith("fp32-exact") and meta["metric"]
    for k in ("mismatches", "latency_ms", "copy_floor", "loop_only", "halo_modes", "resident_loop"):
        assert k not in meta, k
    assert meta["windows"] is None
    assert os.listdir(tmp_path / "out") == ["output.npy"]
    got = np.load(tmp_path / "out" / "output.npy")
    ref = pconv_mod.numpy_convolve(pconv_mod.synthetic_image(w, h, "rgb", seed=77), reps)
    assert got.dtype == np.float32 and np.array_equal(got, ref.reshape(h, -1).astype(np.float32))


@pytest.mark.parametrize("w,h,ch,reps,filt", [(37, 50, "rgb", 9, "gaussian"), (64, 41, "grey", 40, "gaussian"),
                                              (23, 60, "rgb", 7, "box")])
def test_cone_oracle_equals_whole_image_rows(bench, pconv_mod, w, h, ch, reps, filt):
    n = pconv_mod.native
    img = pconv_mod.synthetic_image(w, h, ch, seed=5)
    whole = pconv_mod.numpy_convolve(img, reps, filt).reshape(h, -1)
    for world in (1, 2, 3, 5, 8):
        for rank in range(world):
            band = n.row_band(h, world, rank)
            a = types.SimpleNamespace(width=w, height=h, channels=ch, reps=reps, filter=filt, seed=5)
            ref = bench.oracle_rows(a, band)
            assert np.array_equal(ref, whole[band.y0:band.y0 + band.rows]), (world, rank)
            # the JSON field: bytes that differ from the oracle (single process: no reduction)
            assert bench.mismatching_bytes(ref.copy(), ref) == 0
            bad = ref.copy()
            bad[0, :3] ^= 1
            assert bench.mismatching_bytes(bad, ref) == 3
