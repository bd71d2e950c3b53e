"""First-use tuning on a real MI355X: the path every default call runs.

Group A: with tuning on and every row of a family's shape table ranked, the
tuner times each candidate on the real launch; the frame is canary-guarded, so
a candidate that writes one byte too many shows.  The launch leaves exactly one
entry under its key, and repeating it is a hit: the table is unchanged.

Group B: a cached choice serves launches its key (channels, steps, rows, row
bytes, images, live workgroups) cannot tell from the one that was tuned: the
other border, a band of a taller image, a dims table with other row-byte
residues, an active table, pointers aligned to 8 bytes only, a forced step
form.  Each must be byte-exact on the cached choice or on a legal stand-in.

One launch helper (Case) for the whole file.  Source and destination lie
between GUARD canary bytes; every source byte that is not image data — pad
columns, ghost rows outside the image, the rest of an envelope, the gaps
between frames — is JUNK; the destination is prefilled with the canary and
compared BYTE FOR BYTE with an expected allocation that holds the reference
where the launch may write and the canary everywhere else.  The source must
come back unmodified.

References: exact_gaussian (tests/exact_reference.py, int64) for the gaussian
in both depths, pconv.numpy_convolve for the float filters (float32 by
definition), cpu_fused_launch for band frames.  Image values are uniform random
with a saturated block, a 0 / max checkerboard and 0 / max column groups
planted in them (exact_reference.adversarial)."""
import numpy as np
import pytest

from exact_reference import adversarial, exact_gaussian

pytestmark = pytest.mark.gpu

GUARD = 4096
CANARY = 0xA5
JUNK = 0x77
GAP = 48
NAME = {1: "grey", 3: "rgb", 4: "rgba"}
BORDERS = ["zero", "replicate"]
STEPS = (1, 3, 8, 16)
# fixed: under tuning no single shape defines the edges.  One pixel; one tile of most shapes; RGB and RGBA rows
# of 2-5 strips and two row tiles of the small shapes.
SIZES = [(1, 1), (37, 53), (70, 200)]
NEG_TAPS = ([3, 1, 0, 2, 5, 1, -1, 2, 4], 17)

# family -> (variant, depth, filter for numpy_convolve, index into _tables())
FAMILIES = {
    "swar": ("temporal", 8, "gaussian", 0),
    "box": ("float_temporal", 8, "box", 1),  # uniform taps
    "neg": ("float_temporal", 8, NEG_TAPS, 1),  # non-uniform, a negative tap
    "swar16": ("temporal", 16, "gaussian", 2),
}
ALL = list(FAMILIES)

_IMG = {}  # (depth, c, h, w, seed) -> (h, w * c) samples
_REF = {}  # (family, border, steps, depth, c, h, w, seed) -> reference samples


@pytest.fixture(autouse=True)
def settings(native):
    prev = native.set_autotune(True)
    native.clear_swar_tuning()
    yield
    native.set_tune_candidates(6)
    native.set_prefetch_mode(-1)
    native.set_swar_alt(-1)
    native.set_swar_shape(0, 0, 0)
    native.set_float_shape(0, 0)
    native.set_swar16_shape(0, 0, 0)
    native.set_xcd_swizzle(True)
    native.clear_swar_tuning()
    native.set_autotune(prev)


def _tables(native):
    """The three caches, as plain lists: SWAR, float, 16-bit."""
    return tuple([(list(k), tuple(s)) for k, s in t()]
                 for t in (native.swar_tuned, native.float_tuned, native.swar16_tuned))


def _image(depth, c, h, w, seed=0):
    key = (depth, c, h, w, seed)
    if key not in _IMG:
        rng = np.random.default_rng(7919 * seed + 613 * c + 104729 * h + 17 * w + depth)
        img = adversarial(rng, h, w * c, c, np.uint16 if depth == 16 else np.uint8)
        img.setflags(write=False)
        _IMG[key] = img
    return _IMG[key]


def _reference(pconv_mod, fam, border, steps, c, h, w, seed=0):
    """The lone image's result, (h, w * c) samples."""
    _, depth, filt, _ = FAMILIES[fam]
    key = (fam, border, steps, depth, c, h, w, seed)
    if key not in _REF:
        img = _image(depth, c, h, w, seed)
        x = img.reshape(h, w, c) if c > 1 else img
        if filt == "gaussian":
            ref = exact_gaussian(x, steps, border)
        else:
            ref = pconv_mod.numpy_convolve(x, steps, filt, border)
        ref = np.ascontiguousarray(ref.reshape(h, w * c))
        ref.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


def _bytes(samples):
    """(h, n) samples as (h, n x bytes per sample) uint8, little-endian as in memory."""
    return np.ascontiguousarray(samples).view(np.uint8).reshape(samples.shape[0], -1)


class Case:
    """One launch, built once and launched any number of times.

    `frames` frames of the envelope (c, H, W) lie GAP bytes apart, `lead` bytes
    into the allocation's body.  Frame b holds image b, of sizes[b] = (w, h),
    top-left.  The launch takes the first `batch` frames, or those `active`
    names; with `dims` it carries the extents table.  band = (g_row0, height):
    the single frame is rows [g_row0, g_row0 + H) of a `height`-row image, ghost
    rows inside that image hold its data."""

    def __init__(self, native, pconv_mod, fam, c, H, W, steps, border, sizes=None, frames=1, batch=None, dims=False,
                 active=None, band=None, lead=0, seed=0):
        self.native, self.fam, self.c, self.H, self.steps, self.border = native, fam, c, H, steps, border
        self.variant, self.depth, filt, self.table = FAMILIES[fam]
        self.filter = native.Filter.custom(NEG_TAPS[0], NEG_TAPS[1], "custom") if filt is NEG_TAPS else filt
        bps = self.depth // 8
        self.rb, self.halo = W * c * bps, steps
        halo = steps
        lay = native.frame_layout(self.rb, H, halo)
        self.pitch, self.fbytes = lay["pitch"], lay["bytes"]
        assert lay["pad_left"] == 16 and self.pitch % 16 == 0 and self.fbytes == (H + 2 * halo) * self.pitch
        self.stride = self.fbytes + GAP
        self.frames, self.lead, self.active = frames, lead, active
        self.batch = (frames if batch is None else batch) if active is None else len(active)
        self.g_row0, self.height = band if band else (0, H)
        sizes = [(W, H)] * frames if sizes is None else sizes
        assert len(sizes) == frames and all(1 <= w <= W and 1 <= h <= H for w, h in sizes)
        self.dims = [(w * c * bps, h) for w, h in sizes] if dims else None
        body = lead + frames * self.stride
        self.src_host = np.full(body, JUNK, np.uint8)
        self.exp_host = np.full(body, CANARY, np.uint8)
        launched = range(self.batch) if active is None else active
        for b, (w, h) in enumerate(sizes):
            fr = self._frame(self.src_host, b)
            ex = self._frame(self.exp_host, b)
            if band:
                assert frames == 1 and not dims
                self._fill_band(pconv_mod, fr, ex, W, seed)
                continue
            fr[halo:halo + h, 16:16 + w * c * bps] = _bytes(_image(self.depth, c, h, w, seed + b))
            if b in launched:
                ref = _reference(pconv_mod, fam, border, steps, c, h, w, seed + b)
                ex[halo:halo + h, 16:16 + w * c * bps] = _bytes(ref)

    def _frame(self, body, b):
        o = self.lead + b * self.stride
        return body[o:o + self.fbytes].reshape(self.H + 2 * self.halo, self.pitch)

    def _fill_band(self, pconv_mod, fr, ex, W, seed):
        """Rows of the taller image into the frame; the expected rows from
        cpu_fused_launch on the clean frame (zeros where the frame holds junk)."""
        H, halo, rb, c = self.H, self.halo, self.rb, self.c
        whole = _bytes(_image(self.depth, c, self.height, W, seed + 100))
        clean = np.zeros_like(fr)
        for r in range(-halo, H + halo):
            if 0 <= self.g_row0 + r < self.height:
                clean[halo + r, 16:16 + rb] = whole[self.g_row0 + r]
                fr[halo + r, 16:16 + rb] = whole[self.g_row0 + r]
        out = np.zeros_like(clean)
        self.native.cpu_fused_launch(self.filter, NAME[c], rb, H, halo, clean.reshape(-1), out.reshape(-1), 0, H,
                                     self.steps, self.g_row0, self.height, border=self.border, depth=self.depth)
        lo, hi = max(0, -self.g_row0), min(H, self.height - self.g_row0)
        assert lo < hi
        ex[halo + lo:halo + hi, 16:16 + rb] = out[halo + lo:halo + hi, 16:16 + rb]
        self.rows = hi - lo  # the rows the launch keeps, which is what the tuners key on

    def launch(self):
        """Runs the launch; the list of what is wrong afterwards (empty: nothing)."""
        import torch

        n = self.native
        body = self.src_host.size
        src = torch.full((body + 2 * GUARD,), CANARY, dtype=torch.uint8, device="cuda")
        dst = torch.full((body + 2 * GUARD,), CANARY, dtype=torch.uint8, device="cuda")
        src[GUARD:GUARD + body] = torch.from_numpy(self.src_host).cuda()
        kw, keep = {}, []
        if self.frames > 1:
            kw.update(batch_stride=self.stride)
        if self.dims is not None:
            dev = torch.tensor(self.dims, dtype=torch.int32, device="cuda").contiguous()
            keep.append(dev)
            kw.update(dims=self.dims if self.active is not None else self.dims[:self.batch], dims_ptr=dev.data_ptr())
        if self.active is not None:
            dev = torch.tensor(list(self.active), dtype=torch.int32, device="cuda").contiguous()
            keep.append(dev)
            kw.update(active=list(self.active), active_ptr=dev.data_ptr(), batch_frames=self.frames)
        base = GUARD + self.lead + self.pitch * self.halo + 16
        n.launch_stencil(self.filter, NAME[self.c], src.data_ptr() + base, dst.data_ptr() + base, self.pitch, self.rb,
                         0, self.H, -self.halo, self.H + self.halo, self.steps, self.g_row0, self.height,
                         torch.cuda.current_stream().cuda_stream, self.variant, border=self.border, batch=self.batch,
                         depth=self.depth, **kw)
        torch.cuda.synchronize()
        d, s = dst.cpu().numpy(), src.cpu().numpy()
        bad = []
        if not ((d[:GUARD] == CANARY).all() and (d[-GUARD:] == CANARY).all()):
            bad.append("write outside the destination allocation")
        got = d[GUARD:-GUARD]
        if not np.array_equal(got, self.exp_host):
            off = np.flatnonzero(got != self.exp_host)
            where = []
            for o in off[:3].tolist():
                b, r = divmod(o - self.lead, self.stride) if o >= self.lead else (-1, o)
                where.append((b, r // self.pitch - self.halo, r % self.pitch - 16, int(got[o]), int(self.exp_host[o]))
                             if 0 <= r < self.fbytes and b >= 0 else (b, "gap", r))
            bad.append(f"{len(off)} destination bytes differ; first (frame, row, byte, got, want): {where}")
        if not ((s[:GUARD] == CANARY).all() and (s[-GUARD:] == CANARY).all()
                and np.array_equal(s[GUARD:-GUARD], self.src_host)):
            bad.append("the source was modified")
        return bad


def _key_of(case, entry):
    """The key fields of one table entry that the launch determines, and the
    rest: (fields as expected?, choice).  rows: the launch's, clipped to the image."""
    k, shape = entry
    geom = [case.c, case.steps, getattr(case, "rows", case.H), case.rb]
    if case.fam == "swar":  # {channels, steps, rows, row_bytes, form, kern, batch, live}
        return k[:4] == geom and k[6] == case.batch, dict(shape=shape, form=k[4], kern=k[5], live=k[7])
    if case.fam == "swar16":  # {channels, steps, rows, row_bytes, form, batch, live}
        return k[:4] == geom and k[5] == case.batch, dict(shape=shape, form=k[4], live=k[6])
    uniform = 1 if case.fam == "box" else 0  # {channels, uniform, steps, rows, row_bytes, batch, live}
    return [k[0]] + k[2:5] == geom and k[1] == uniform and k[5] == case.batch, dict(shape=shape, live=k[6])


def _the_entry(native, case):
    """The one entry the case's first launch left: its family's table holds
    exactly it, under the launch's key, with a choice out of the family's shape
    table; the other families' tables are empty."""
    tabs = _tables(native)
    for i, t in enumerate(tabs):
        assert len(t) == (1 if i == case.table else 0), (case.fam, tabs)
    ok, choice = _key_of(case, tabs[case.table][0])
    assert ok, (case.fam, tabs[case.table][0])
    shapes = {"swar": native.swar_shapes, "swar16": native.swar16_shapes}.get(case.fam, native.float_shapes)()
    assert choice["shape"] in [tuple(s) for s in shapes], choice
    if "form" in choice:
        assert choice["form"] in (0, 1), choice
    if "kern" in choice:
        assert choice["kern"] in (0, 1), choice
        if choice["kern"] == 1:
            assert choice["shape"] in [tuple(s) for s in native.swar_prefetch_shapes()], choice
    return choice


def _tune(native, case):
    """First launch of a cleared table: exact, and it leaves its one entry."""
    native.clear_swar_tuning()
    assert not case.launch()
    return _the_entry(native, case)


def _hit(native, case, what):
    """A launch the table must serve as it is: exact, and the table unchanged."""
    before = _tables(native)
    bad = case.launch()
    assert not bad, (what, bad)
    assert _tables(native) == before, what


# ---- Group A: every candidate runs the real launch ------------------------------


@pytest.mark.parametrize("channels", [1, 3, 4])
@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("fam", ALL)
def test_every_candidate_on_a_guarded_frame(native, pconv_mod, fam, border, channels):
    native.set_tune_candidates(32)  # more than any shape table holds: every row is timed
    assert len(native.swar_shapes()) <= 32
    for h, w in SIZES:
        for steps in STEPS:
            case = Case(native, pconv_mod, fam, channels, h, w, steps, border)
            # tuning off: exact, and nothing is cached
            native.set_autotune(False)
            native.clear_swar_tuning()
            assert not case.launch(), (h, w, steps, "untuned")
            assert _tables(native) == ([], [], []), (h, w, steps)
            # tuning on: every candidate writes the guarded frame, one entry lands
            native.set_autotune(True)
            bad = case.launch()
            assert not bad, (h, w, steps, "tuning", bad)
            _the_entry(native, case)
            _hit(native, case, (h, w, steps, "the same launch again"))


# ---- Group B: a cached choice and the launches its key cannot tell apart --------


@pytest.mark.parametrize("fam", ALL)
def test_hit_under_the_other_border(native, pconv_mod, fam):
    """B1: tuned under the zero border, hit under replicate."""
    c, h, w, steps = 3, 37, 53, 3
    x = Case(native, pconv_mod, fam, c, h, w, steps, "zero")
    y = Case(native, pconv_mod, fam, c, h, w, steps, "replicate")
    assert not np.array_equal(_reference(pconv_mod, fam, "zero", steps, c, h, w),
                              _reference(pconv_mod, fam, "replicate", steps, c, h, w))
    _tune(native, x)
    _hit(native, y, "replicate on the zero border's entry")
    _hit(native, x, "the tuned launch again")


@pytest.mark.parametrize("fam", ALL)
def test_hit_by_a_band_of_a_taller_image(native, pconv_mod, fam):
    """B2: tuned on a whole 30 x 45 RGB image; hit by the same frame as rows
    35..65 of a 100-row image.  At g_row0 = 74 the owned rows reach past the
    image bottom, the launch is clipped to 26 rows and that is the key's row
    count: its hit is on the entry of a whole 26 x 45 image, tuned beside the
    other.  Ghost rows inside the image hold data, those outside hold junk."""
    c, h, w, steps = 3, 30, 45, 3
    for border in BORDERS:
        x = Case(native, pconv_mod, fam, c, h, w, steps, border)
        x26 = Case(native, pconv_mod, fam, c, 26, w, steps, border, seed=5)
        mid = Case(native, pconv_mod, fam, c, h, w, steps, border, band=(35, 100))
        low = Case(native, pconv_mod, fam, c, h, w, steps, border, band=(74, 100))
        assert mid.rows == 30 and low.rows == 26
        _tune(native, x)
        assert not x26.launch()
        assert len(_tables(native)[x.table]) == 2
        _hit(native, mid, (border, "g_row0 = 35"))
        _hit(native, low, (border, "g_row0 = 74"))
        _hit(native, x, (border, "the tuned launch again"))
        _hit(native, x26, (border, "the 26-row launch again"))


def _tune_bufop(native, case):
    """Tunes `case` with the buffer-op kernel forced: the entry holds kern = 1
    (asserted: the tests below prove nothing otherwise)."""
    native.set_prefetch_mode(1)
    native.set_tune_candidates(32)
    choice = _tune(native, case)
    native.set_prefetch_mode(-1)
    assert choice["kern"] == 1, choice
    return choice


ENVELOPE = dict(c=3, H=49, W=140, steps=3)  # RGB 140 x 49: 420 row bytes


def _ragged(native, pconv_mod, fam, second_width, **kw):
    e = ENVELOPE
    return Case(native, pconv_mod, fam, e["c"], e["H"], e["W"], e["steps"], "zero",
                sizes=[(e["W"], e["H"]), (second_width, 1)], frames=2, dims=True, **kw)


def test_bufop_entry_and_a_dims_table_of_other_residues(native, pconv_mod):
    """B3: a one-row image of 12 bytes and one of 15 count alike (one strip, one
    row tile under every shape), so the two dims launches share a key; only the
    first may run the buffer-op kernel (whole dwords per row of every image)."""
    x = _ragged(native, pconv_mod, "swar", 4)  # dims [(420, 49), (12, 1)]
    y = _ragged(native, pconv_mod, "swar", 5, seed=3)  # dims [(420, 49), (15, 1)]
    assert x.dims == [(420, 49), (12, 1)] and y.dims == [(420, 49), (15, 1)]
    choice = _tune_bufop(native, x)
    assert choice["live"] > 0
    _hit(native, y, "15-byte rows on the buffer-op entry")
    _hit(native, x, "the tuned launch again")
    assert _the_entry(native, x)["kern"] == 1
    native.set_prefetch_mode(0)  # "never" holds on a hit too
    _hit(native, y, "15-byte rows, buffer-op kernel off")
    _hit(native, x, "the tuned launch, buffer-op kernel off")
    native.set_prefetch_mode(-1)
    _hit(native, x, "the tuned launch again")
    assert _the_entry(native, x)["kern"] == 1


def test_batch_engine_run_images_after_a_bufop_tuning(native, pconv_mod):
    """B3 through the public API: a BatchEngine whose first mixed-size call
    tuned to the buffer-op kernel takes a second call with a 5-pixel-wide RGB
    image (15 row bytes)."""
    e = ENVELOPE
    eng = pconv_mod.BatchEngine(e["W"], e["H"], "rgb", capacity=2)
    imgs = {w: _image(8, 3, h, w, seed=9).reshape(h, w, 3).copy() for w, h in [(140, 49), (4, 1), (5, 1)]}
    want = {w: exact_gaussian(x, e["steps"], "zero") for w, x in imgs.items()}
    native.set_prefetch_mode(1)
    native.set_tune_candidates(32)
    out = eng.run_images([imgs[140], imgs[4]], e["steps"])
    native.set_prefetch_mode(-1)
    assert np.array_equal(out[0], want[140]) and np.array_equal(out[1], want[4])
    swar = _tables(native)[0]
    assert [k[5] for k, _ in swar if k[:4] == [3, e["steps"], e["H"], 420] and k[6] == 2] == [1], swar
    out = eng.run_images([imgs[140], imgs[5]], e["steps"])
    assert np.array_equal(out[0], want[140]) and np.array_equal(out[1], want[5])
    assert _tables(native)[0] == swar


@pytest.mark.parametrize("fam", ["box", "neg", "swar16"])
def test_hit_by_a_dims_table_of_other_residues(native, pconv_mod, fam):
    """B3 for the families without a dword rule: plain hits."""
    x = _ragged(native, pconv_mod, fam, 4)
    y = _ragged(native, pconv_mod, fam, 5, seed=3)
    assert _tune(native, x)["live"] > 0
    _hit(native, y, "the other dims table")
    _hit(native, x, "the tuned launch again")


def test_bufop_entry_and_an_active_table(native, pconv_mod):
    """B4: frames 0-2 of five tune to the buffer-op kernel; the table {0, 2, 4}
    has the same count and the same live workgroups, and frame 4's rows are 15
    bytes.  An active launch never tunes: it must run the entry legally."""
    e = ENVELOPE
    sizes = [(140, 49), (4, 1), (140, 49), (140, 49), (5, 1)]
    args = (native, pconv_mod, "swar", e["c"], e["H"], e["W"], e["steps"], "zero")
    x = Case(*args, sizes=sizes, frames=5, batch=3, dims=True)
    y = Case(*args, sizes=sizes, frames=5, active=[0, 2, 4], dims=True)
    assert x.dims == [(420, 49), (12, 1), (420, 49), (420, 49), (15, 1)] and x.batch == y.batch == 3
    for b in (1, 3):  # what the table does not name stays canary
        assert (y._frame(y.exp_host, b) == CANARY).all()
    _tune_bufop(native, x)
    _hit(native, y, "active {0, 2, 4} on the buffer-op entry")
    _hit(native, x, "the tuned launch again")
    assert _the_entry(native, x)["kern"] == 1


def test_swar16_hit_with_pointers_aligned_to_8_bytes(native, pconv_mod):
    """B5: the 16-byte-lane shapes need 16-byte aligned pointers, which the key
    leaves out.  The same launch 8 bytes further into its allocations is exact,
    and afterwards the entry is a shape of 8-byte lanes: kept, or re-tuned."""
    c, h, w, steps = 3, 37, 53, 3
    x = Case(native, pconv_mod, "swar16", c, h, w, steps, "zero")
    y = Case(native, pconv_mod, "swar16", c, h, w, steps, "zero", lead=8)
    assert y.pitch % 16 == 0 and y.fbytes % 16 == 0
    _tune(native, x)
    bad = y.launch()
    assert not bad, bad
    assert _the_entry(native, y)["shape"][0] == 4
    _hit(native, y, "the moved launch again")
    _hit(native, x, "the aligned launch on what the moved one left")


@pytest.mark.parametrize("fam", ["swar", "swar16"])
def test_forced_step_form_on_a_hit(native, pconv_mod, fam):
    """B6: set_swar_alt on a cached entry: the shape stays, the form is the forced one."""
    for c, (h, w), steps in [(3, (37, 53), 3), (4, (70, 200), 8), (1, (37, 53), 16)]:
        x = Case(native, pconv_mod, fam, c, h, w, steps, "replicate")
        native.set_swar_alt(-1)
        _tune(native, x)
        for form in (0, 1):
            native.set_swar_alt(form)
            _hit(native, x, (c, h, w, steps, "form", form))
        native.set_swar_alt(-1)
        _hit(native, x, (c, h, w, steps, "tuned form"))
