// BatchEngine (see batch_engine.hpp).
#include "pconv/batch_engine.hpp"

#include <algorithm>
#include <cstring>
#include <string>

#include "pconv/cpu_stencil.hpp"
#include "pconv/schedule.hpp"
#include "pconv/trace.hpp"

namespace pconv {

BatchEngine::BatchEngine(const ImageGeom& geom, const Filter& filter, int capacity, const EngineOptions& opt)
    : geom_(geom), filter_(filter), opt_(opt), capacity_(capacity) {
  geom_.validate();
  PCONV_CHECK(capacity >= 1, "BatchEngine: capacity must be >= 1");
  // A batch runs on the temporal kernels only (launch_stencil routes Auto to
  // them for every step count); say so here, not at the first launch.
  const KernelVariant v = opt.variant;
  PCONV_CHECK(v == KernelVariant::Auto || v == KernelVariant::Temporal || v == KernelVariant::FloatTemporal,
              "BatchEngine: batch not supported by kernel '" + std::string(kernel_variant_name(v)) + "'");
  if (geom_.depth == 16) {
    PCONV_CHECK(filter_.binomial121, "BatchEngine: depth 16 runs the gaussian filter only, not '" + filter_.name + "'");
    PCONV_CHECK(v != KernelVariant::FloatTemporal, "BatchEngine: depth 16 not supported by kernel 'float_temporal'");
  }
  PlanConfig c;
  c.fuse = opt.fuse;
  c = normalize_plan_config(c, 0, kMaxFusedSteps);
  opt_.fuse = c.fuse;
  opt_.halo_depth = c.fuse;
  set_device(opt_.device);
  lay_ = FrameLayout::make(geom_.row_bytes(), geom_.height, opt_.fuse);
  stride_ = lay_.bytes();  // total_rows x pitch: whole pitches, a multiple of 16
  if (opt_.compute_stream) {
    cs_ = opt_.compute_stream;
  } else {
    own_cs_ = Stream::create(0);
    cs_ = own_cs_.get();
  }
  // Both allocations are zeroed once: pad columns, ghost rows and the frames
  // of images a partial batch leaves out are never written afterwards.
  for (auto& f : frame_) {
    f = DeviceBuffer(static_cast<size_t>(stride_ * capacity_));
    zero_words(f.data(), f.size());
  }
  ev_sync_ = Event::create();
  ev_t0_ = Event::create(true);
  ev_t1_ = Event::create(true);
  PCONV_HIP_CHECK(hipStreamSynchronize(cs_));
}

BatchEngine::~BatchEngine() {
  if (cs_) (void)hipStreamSynchronize(cs_);
}

void BatchEngine::check_n(const char* who, int n) const {
  PCONV_CHECK(n >= 0 && n <= capacity_, std::string(who) + ": " + std::to_string(n) + " images outside [0, capacity " +
                                            std::to_string(capacity_) + "]");
  PCONV_CHECK(sizes_.empty() || n == static_cast<int>(sizes_.size()),
              std::string(who) + ": " + std::to_string(n) + " images, but the mixed-size upload holds " +
                  std::to_string(sizes_.size()));
}

// ---- copies: one switch site per kind (opt_.kernel_copies: the CUs move the
// bytes, no SDMA engine and no runtime blit program) -------------------------

void BatchEngine::copy_words(uint8_t* dst, const uint8_t* src, size_t bytes, hipMemcpyKind kind) {
  const int64_t b = static_cast<int64_t>(bytes);
  if (opt_.kernel_copies)
    launch_copy_rows(src, b, dst, b, b, 1, cs_);
  else
    PCONV_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, kind, cs_));
}

void BatchEngine::zero_words(uint8_t* p, size_t bytes) {
  if (opt_.kernel_copies)
    launch_fill_zero(p, static_cast<int64_t>(bytes), cs_);
  else
    PCONV_HIP_CHECK(hipMemsetAsync(p, 0, bytes, cs_));
}

// n pitched 2-D copies, one per image — the call every other engine of this
// library uses for its rows — between the current frames and `packed`, where
// the images lie back to back with tight rows; image b is extents[b], or the
// engine's geometry for every image (null).  One hipMemcpy3DAsync could
// describe a whole uniform batch (the frames sit a whole number of pitches
// apart), but it has not been timed against this form; tools/batch_sweep.py
// reports the end-to-end time these copies give.
void BatchEngine::copy_images(bool to_frames, uint8_t* packed, int n, const ImageDims* extents, bool device) {
  const hipMemcpyKind kind =
      device ? hipMemcpyDeviceToDevice : (to_frames ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost);
  for (int b = 0; b < n; ++b) {
    const int64_t rb = extents ? extents[b].row_bytes : lay_.row_bytes, rows = extents ? extents[b].height : lay_.rows;
    uint8_t* frame = frame_at(cur_) + b * stride_;  // cur_ follows the launches: the newest frames
    const uint8_t* src = to_frames ? packed : frame;
    uint8_t* dst = to_frames ? frame : packed;
    const int64_t sp = to_frames ? rb : lay_.pitch, dp = to_frames ? lay_.pitch : rb;
    if (opt_.kernel_copies)
      launch_copy_rows(src, sp, dst, dp, rb, rows, cs_);
    else
      PCONV_HIP_CHECK(hipMemcpy2DAsync(dst, dp, src, sp, rb, rows, kind, cs_));
    packed += rb * rows;
  }
}

// A table goes to the device out of pinned words that are rewritten only after
// the event behind the previous copy out of them, and is copied ON THE COMPUTE
// STREAM.  One device region is enough: the stream is in order, so the copy
// lands after every launch that was enqueued with the previous table has
// finished, and before every launch enqueued after it starts.
void BatchEngine::stage(StagedTable& t, const char* what, const void* entries, size_t entry_bytes, size_t n) {
  const size_t bytes = round_up<size_t>(entry_bytes * static_cast<size_t>(capacity_), 16);
  if (!t.dev.data()) {
    PCONV_CHECK(!stream_capturing(cs_),
                std::string("BatchEngine: the ") + what + " table cannot be allocated on a capturing stream");
    t.dev = DeviceBuffer(bytes);
    t.pin = PinnedBuffer(bytes);
    std::memset(t.pin.data(), 0, bytes);
    t.ev = Event::create();
  } else {
    t.ev.sync();  // the previous copy out of the pinned words has completed
  }
  std::memcpy(t.pin.data(), entries, entry_bytes * n);
  copy_words(t.dev.data(), t.pin.data(), bytes, hipMemcpyHostToDevice);
  t.ev.record(cs_);
}

void BatchEngine::upload_active(const std::vector<int32_t>& table) {
  PCONV_CHECK(!table.empty() && static_cast<int>(table.size()) <= capacity_,
              "BatchEngine: an active-image table must hold 1 to `capacity` entries");
  stage(active_, "active-image", table.data(), sizeof(int32_t), table.size());
  active_host_ = table;
}

void BatchEngine::upload(const uint8_t* p, int n, bool device) {
  sizes_.clear();  // back to uniform launches
  dims_host_.clear();
  orig_n_ = 0;  // a snapshot describes the frames before this upload
  check_n("BatchEngine::upload", n);
  PCONV_CHECK(p != nullptr || n == 0, "BatchEngine::upload: null source");
  copy_images(true, const_cast<uint8_t*>(p), n, nullptr, device);
}

void BatchEngine::download(uint8_t* p, int n, bool device) {
  check_n("BatchEngine::download", n);
  PCONV_CHECK(p != nullptr || n == 0, "BatchEngine::download: null destination");
  copy_images(false, p, n, nullptr, device);
}

void BatchEngine::upload_sized(const uint8_t* p, const std::vector<ImageSize>& sizes, bool device) {
  std::vector<ImageDims> table = image_dims_table(geom_, capacity_, sizes);
  PCONV_CHECK(p != nullptr || sizes.empty(), "BatchEngine::upload_sized: null source");
  orig_n_ = 0;
  if (!sizes.empty()) {
    stage(dims_, "extents", table.data(), sizeof(ImageDims), table.size());
    // No frame is cleared: the kernels read nothing outside an image.
    copy_images(true, const_cast<uint8_t*>(p), static_cast<int>(table.size()), table.data(), device);
  }
  sizes_ = sizes;
  dims_host_ = std::move(table);
}

void BatchEngine::download_sized(uint8_t* p, bool device) {
  PCONV_CHECK(p != nullptr || sizes_.empty(), "BatchEngine::download_sized: null destination");
  copy_images(false, p, static_cast<int>(dims_host_.size()), dims_host_.data(), device);
}

// ---- decimated results --------------------------------------------------------
// ONE launch_decimate for all n images.  A uniform batch into device memory
// goes straight to the caller's buffer (tight rows, frames back to back: the
// kernel's byte stores take any alignment).  Everything else — host memory, and
// mixed sizes, whose packed images have a row pitch each — goes through staging
// frames of the decimated envelope, from which one pitched copy per image (the
// copies of copy_images) moves the image regions.

void BatchEngine::decimate_images(uint8_t* p, int n, int factor, bool device) {
  check_decimate(factor);
  if (n == 0) return;
  PCONV_CHECK(!stream_capturing(cs_), "BatchEngine: a decimated download is not captured into a hipGraph");
  const int64_t pb = geom_.pixel_bytes();
  const ImageGeom og = decimated_geom(geom_, factor);
  const int64_t orb = og.row_bytes(), oh = og.height;
  DecimateLaunch d;
  d.src = frame_at(cur_);
  d.src_pitch = lay_.pitch;
  d.row_bytes = lay_.row_bytes;
  d.rows = lay_.rows;
  d.pixel_bytes = static_cast<int>(pb);
  d.factor = factor;
  d.images = image_tables(n);
  d.src_stride = stride_;
  const ImageDims* extents = d.images.dims_host;  // mixed mode: the packed images have a row pitch each
  if (device && !extents) {
    d.dst = p;
    d.dst_pitch = orb;
    d.dst_stride = oh * orb;
    d.dst_bytes = n * oh * orb;
    launch_decimate(d, cs_);
    return;
  }
  const int64_t sp = round_up<int64_t>(orb, 16), sstride = oh * sp;
  const size_t need = static_cast<size_t>(sstride * capacity_);
  if (dec_stage_.size() < need) {
    PCONV_HIP_CHECK(hipStreamSynchronize(cs_));  // no earlier copy still reads the buffer that goes
    dec_stage_ = DeviceBuffer(need);
  }
  d.dst = dec_stage_.data();
  d.dst_pitch = sp;
  d.dst_stride = sstride;
  d.dst_bytes = static_cast<int64_t>(dec_stage_.size());
  launch_decimate(d, cs_);
  const hipMemcpyKind kind = device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  for (int b = 0; b < n; ++b) {
    const int64_t rb = extents ? decimated_extent(extents[b].row_bytes / pb, factor) * pb : orb;
    const int64_t rows = extents ? decimated_extent(extents[b].height, factor) : oh;
    const uint8_t* src = dec_stage_.data() + b * sstride;
    if (opt_.kernel_copies)
      launch_copy_rows(src, sp, p, rb, rb, rows, cs_);
    else
      PCONV_HIP_CHECK(hipMemcpy2DAsync(p, rb, src, sp, rb, rows, kind, cs_));
    p += rb * rows;
  }
}

void BatchEngine::download_decimated(uint8_t* p, int n, int factor, bool device) {
  check_n("BatchEngine::download_decimated", n);
  PCONV_CHECK(sizes_.empty(), "BatchEngine::download_decimated: the upload was mixed-size (download_sized_decimated)");
  PCONV_CHECK(p != nullptr || n == 0, "BatchEngine::download_decimated: null destination");
  if (factor == 1) return download(p, n, device);
  decimate_images(p, n, factor, device);
}

void BatchEngine::download_sized_decimated(uint8_t* p, int factor, bool device) {
  PCONV_CHECK(p != nullptr || sizes_.empty(), "BatchEngine::download_sized_decimated: null destination");
  if (factor == 1) return download_sized(p, device);
  decimate_images(p, static_cast<int>(dims_host_.size()), factor, device);
}

int64_t decimated_packed_bytes(const ImageGeom& env, const std::vector<ImageSize>& sizes, int factor) {
  int64_t total = 0;
  for (const auto& z : sizes)
    total += decimated_extent(z.width, factor) * decimated_extent(z.height, factor) * env.pixel_bytes();
  return total;
}

// ---- unsharp mask -------------------------------------------------------------
// The originals live in a third allocation laid out like the two frame sets
// (image b at b * stride_, rows at lay_.pitch), so the kernel takes one stride
// for all three pointers.  ONE launch each: the frames sit a whole number of
// pitches apart, so images [0, n) are one pitched run of rows for the copy
// (the ghost rows between them travel along), and the kernel takes `frames`.

void BatchEngine::snapshot_original(int n) {
  check_n("BatchEngine::snapshot_original", n);
  PCONV_CHECK(active_host_.empty(), "BatchEngine::snapshot_original: an active-image table is in force");
  PCONV_CHECK(!stream_capturing(cs_), "BatchEngine::snapshot_original: not captured into a hipGraph");
  orig_n_ = 0;
  if (n == 0) return;
  if (!orig_.data()) orig_ = DeviceBuffer(static_cast<size_t>(stride_ * capacity_));
  const int64_t rows = (n - 1) * (stride_ / lay_.pitch) + lay_.rows;
  launch_copy_rows(frame_at(cur_), lay_.pitch, orig_.data() + lay_.offset(0), lay_.pitch, lay_.row_bytes, rows, cs_);
  orig_n_ = n;
}

void BatchEngine::apply_unsharp(int k, int threshold, int n) {
  check_n("BatchEngine::apply_unsharp", n);
  check_unsharp(k, threshold, geom_.depth);
  PCONV_CHECK(active_host_.empty(), "BatchEngine::apply_unsharp: an active-image table is in force");
  PCONV_CHECK(!stream_capturing(cs_), "BatchEngine::apply_unsharp: not captured into a hipGraph");
  PCONV_CHECK(n == orig_n_, "BatchEngine::apply_unsharp: " + std::to_string(n) + " images, but the snapshot holds " +
                                std::to_string(orig_n_) + " (snapshot_original(n) after the upload, before run())");
  orig_n_ = 0;  // the frames are no blur of the snapshot any more
  if (n == 0) return;
  UnsharpLaunch u;
  u.orig = orig_.data() + lay_.offset(0);
  u.blur = u.dst = frame_at(cur_);  // in place on the newest frames
  u.orig_pitch = u.blur_pitch = u.dst_pitch = lay_.pitch;
  u.row_bytes = lay_.row_bytes;
  u.rows = lay_.rows;
  u.depth = geom_.depth;
  u.k = k;
  u.threshold = threshold;
  u.images = image_tables(n);
  u.orig_stride = u.blur_stride = u.dst_stride = stride_;
  launch_unsharp(u, cs_);
}

// Images [0, n) for a launch: the extents table in mixed mode, the table of
// open images while a compacting run_until_stable has retired some.
ImageTables BatchEngine::image_tables(int n) const {
  ImageTables t;
  t.frames = n;
  if (!sizes_.empty()) {
    t.dims = reinterpret_cast<const ImageDims*>(dims_.dev.data());
    t.dims_host = dims_host_.data();
  }
  if (!active_host_.empty()) {
    t.active = reinterpret_cast<const int32_t*>(active_.dev.data());
    t.active_host = active_host_.data();
    t.count = static_cast<int>(active_host_.size());
  }
  return t;
}

// What every temporal and residual launch over images [0, n) of the current
// frames shares: whole images, their tables, the frames' stride.
StencilLaunch BatchEngine::base_launch(int n) const {
  StencilLaunch a;
  a.src = frame_at(cur_);
  a.pitch = lay_.pitch;
  a.row_bytes = lay_.row_bytes;
  a.r0 = 0;
  a.r1 = lay_.rows;
  a.frame_lo = -lay_.halo;
  a.frame_hi = lay_.rows + lay_.halo;
  a.g_row0 = 0;
  a.height = geom_.height;
  a.border = opt_.border;
  a.depth = geom_.depth;
  static_cast<ImageTables&>(a.images) = image_tables(n);
  a.images.stride = stride_;
  return a;
}

void BatchEngine::run(int reps, int n) {
  TraceRange tr("pconv.batch.run");
  PCONV_CHECK(reps >= 0, "repetitions must be >= 0");
  check_n("BatchEngine::run", n);
  Band band;
  band.rows = geom_.height;
  PlanConfig c;
  c.fuse = supports_fusion(filter_, opt_.variant) ? opt_.fuse : 1;
  c.halo_depth = opt_.fuse;
  const std::vector<Phase> ph = plan_band(band, reps, c);
  stats_ = RunStats{};
  wall_t0_ = wall_seconds();
  if (opt_.timing) ev_t0_.record(cs_);
  if (n > 0) {
    // First use of a (geometry, steps, batch) tunes inside launch_stencil on
    // this very launch, frame[cur] -> frame[cur ^ 1] (BandEngine's rule: the
    // input is only read, every candidate writes the same bytes), and never on
    // a capturing stream.
    for (const auto& p : ph) {
      for (const auto& l : p.launches) {
        StencilLaunch a = base_launch(n);
        a.dst = frame_at(cur_ ^ 1);
        a.r0 = l.lo;
        a.r1 = l.hi;
        a.steps = l.steps;
        launch_stencil(filter_, geom_.channels, a, cs_, opt_.variant);
        ++stats_.launches;
        stats_.image_launches += a.images.images();
      }
      cur_ ^= 1;
    }
  }
  if (opt_.timing) {
    ev_t1_.record(cs_);
    timing_pending_ = true;
  }
}

// ---- fixed points (BandEngine's pattern, one counter per image) -----------

void BatchEngine::launch_batch_residual(int n) {
  launch_residual(filter_, geom_.channels, base_launch(n), reinterpret_cast<uint64_t*>(res_count_.data()), cs_);
}

void BatchEngine::enqueue_residual(int n) {
  TraceRange tr("pconv.batch.residual");
  // The host waits for the counts: a check has no place in a graph.
  PCONV_CHECK(!stream_capturing(cs_), "BatchEngine: a residual check cannot be enqueued on a capturing stream");
  const size_t bytes = round_up<size_t>(sizeof(uint64_t) * static_cast<size_t>(capacity_), 16);
  if (!res_count_.data()) {
    res_count_ = DeviceBuffer(bytes);
    res_host_ = PinnedBuffer(bytes);
    zero_words(res_count_.data(), bytes);
    res_ev_ = Event::create();
    res_seen_.assign(static_cast<size_t>(capacity_), 0);
  }
  // The device counters are never zeroed again: they run on, a check is the
  // per-image difference to the value the check before it read (the stream is
  // in order).  All `capacity` words are read back: those of images >= n have
  // not moved.
  launch_batch_residual(n);
  copy_words(res_host_.data(), res_count_.data(), bytes, hipMemcpyDeviceToHost);
  res_ev_.record(cs_);
}

std::vector<uint64_t> BatchEngine::finish_residual(int n) {
  res_ev_.sync();
  std::vector<uint64_t> out(static_cast<size_t>(n));
  for (int b = 0; b < n; ++b) {
    uint64_t total = 0;
    std::memcpy(&total, res_host_.data() + sizeof(total) * static_cast<size_t>(b), sizeof(total));
    out[b] = total - res_seen_[b];
    res_seen_[b] = total;
  }
  return out;
}

std::vector<uint64_t> BatchEngine::residual(int n) {
  check_n("BatchEngine::residual", n);
  if (n == 0) return {};
  enqueue_residual(n);
  std::vector<uint64_t> out = finish_residual(n);
  synchronize();
  return out;
}

std::vector<double> BatchEngine::time_residual(int launches, int n) {
  check_n("BatchEngine::time_residual", n);
  std::vector<double> ms;
  if (n == 0) return ms;
  (void)residual(n);  // the counters exist
  for (int i = 0; i < launches; ++i) {
    ev_t0_.record(cs_);
    launch_batch_residual(n);
    ev_t1_.record(cs_);
    PCONV_HIP_CHECK(hipStreamSynchronize(cs_));
    ms.push_back(Event::elapsed_ms(ev_t0_, ev_t1_));
  }
  (void)residual(n);  // (the next check's differences start behind these launches)
  return ms;
}

// Compaction (`compact`): an image whose count was zero at check j leaves the
// launches.  The chunk after that check is already in flight with it, so the
// first launches without it are check j + 1 and chunk j + 2.
//   Why no frame parity is kept per image: a retired image X satisfies
// step(X) = X in the frame check j read, and it takes part in at least one
// fused launch AFTER that check — the chunk in flight — which writes
// step^t(X) = X into the other ping-pong frame.  Both frames of a retired
// image therefore hold the same image bytes, whichever of them cur_ names when
// the loop ends: download / download_sized go on reading cur_ for every image,
// and a later plain run(reps, n) continues every image correctly.  The "at
// least one launch" is checked below for every image at the moment it is
// retired, and nothing is retired when the loop ends at the check (no chunk
// follows it).
std::vector<StableStats> BatchEngine::run_until_stable(int max_reps, int check_every, int n, bool compact) {
  PCONV_CHECK(max_reps >= 0, "repetitions must be >= 0");
  PCONV_CHECK(check_every >= 1, "check_every must be >= 1");
  check_n("BatchEngine::run_until_stable", n);
  std::vector<StableStats> st(static_cast<size_t>(n));
  if (n == 0) {
    stats_ = RunStats{};
    return st;
  }
  // The table lives for this call only, also when a launch throws.
  struct ClearActive {
    std::vector<int32_t>& t;
    ~ClearActive() { t.clear(); }
  } clear_active{active_host_};
  active_host_.clear();
  RunStats sum;
  const double w0 = wall_seconds();
  // Fused launches image b has taken part in, and that number when the latest
  // check was enqueued (the invariant above).
  std::vector<int64_t> launched(static_cast<size_t>(n), 0), at_check(static_cast<size_t>(n), 0);
  auto chunk = [&](int k) {
    run(k, n);
    sum.launches += stats_.launches;
    sum.image_launches += stats_.image_launches;
    if (active_host_.empty())
      for (auto& l : launched) l += stats_.launches;
    else
      for (const int32_t b : active_host_) launched[b] += stats_.launches;
  };
  auto check = [&] {
    at_check = launched;
    enqueue_residual(n);
  };
  int done = std::min(check_every, max_reps);
  int checks = 0, open = n;
  chunk(done);
  check();
  for (;;) {
    // The next chunk is enqueued BEFORE the host waits for this check's
    // counts, so the GPU never idles over the read-back.  If every count turns
    // out zero, the chunk in flight repeats the fixed points' bytes.
    const int next = std::min(check_every, max_reps - done);
    if (next > 0) chunk(next);
    // (a retired image's counter no longer moves: its difference reads zero)
    const std::vector<uint64_t> cnt = finish_residual(n);
    ++checks;
    bool retire = false;
    for (int b = 0; b < n; ++b) {
      StableStats& s = st[b];
      if (s.converged) {
        PCONV_CHECK(cnt[b] == 0, "BatchEngine::run_until_stable: image " + std::to_string(b) + " left its fixed point (" +
                                     std::to_string(cnt[b]) + " bytes change at check " + std::to_string(checks) + ")");
        continue;
      }
      s.residual = cnt[b];
      s.checks = checks;
      s.reps_done = done;
      s.converged = cnt[b] == 0;
      if (s.converged) {
        --open;
        retire = true;
      }
    }
    if (open == 0 || next == 0) break;
    if (compact && retire) {
      // The images this check found fixed leave the launches from here on:
      // the next check and the chunk after the one in flight.
      std::vector<int32_t> table;
      for (int b = 0; b < n; ++b) {
        if (!st[b].converged) {
          table.push_back(b);
          continue;
        }
        if (st[b].checks != checks) continue;  // retired at an earlier check
        PCONV_CHECK(launched[b] > at_check[b],
                    "BatchEngine::run_until_stable: image " + std::to_string(b) +
                        " would be retired without a fused launch since its zero check (its two frames could differ)");
      }
      upload_active(table);
    }
    done += next;
    check();
  }
  synchronize();
  sum.wall_ms = (wall_seconds() - w0) * 1e3;
  sum.loop_ms = sum.wall_ms;  // chunks and checks overlap: the loop is timed as a whole, on the host
  stats_ = sum;
  return st;
}

void BatchEngine::wait_stream(hipStream_t s) {
  ev_sync_.record(s);
  ev_sync_.wait_on(cs_);
}

void BatchEngine::signal_stream(hipStream_t s) {
  ev_sync_.record(cs_);
  ev_sync_.wait_on(s);
}

void BatchEngine::synchronize() {
  PCONV_HIP_CHECK(hipStreamSynchronize(cs_));
  if (timing_pending_) {
    stats_.loop_ms = Event::elapsed_ms(ev_t0_, ev_t1_);
    stats_.wall_ms = (wall_seconds() - wall_t0_) * 1e3;
    timing_pending_ = false;
  }
}

}  // namespace pconv
