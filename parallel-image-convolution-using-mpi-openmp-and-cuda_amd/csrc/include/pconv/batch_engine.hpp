// Batch engine: up to `capacity` whole images of ONE geometry resident on one
// GPU, advanced together — every launch carries the n frames as its image set
// (StencilLaunch::images, pconv/kernels.hpp), so a run of `reps` repetitions is
// ceil(reps / fuse) launches whatever n.
//
// Small images cannot fill 256 CUs one at a time (a launch of the temporal
// kernels costs its per-step latency, not its work: docs/PERFORMANCE.md §1.5);
// a batch widens the grid instead of lengthening the queue of launches.
//
// No bands, neighbours or transport: each image is the band {y0 = 0, rows = H}
// of BandEngine, and the plan is plan_band's for that band.
//
// Fixed points: residual(n) counts, per image and in ONE launch of the
// residual kernel, the bytes one more repetition would change;
// run_until_stable advances all n images in chunks with such a check after
// each and reports for every image what a single-image run of it would have
// reported.  Converged images keep advancing with the rest (they rewrite the
// same bytes) until the last image converges or max_reps is reached — unless
// the caller asks for compaction.
//
// Compaction (run_until_stable's `compact`, off by default): an image found
// fixed at check j is retired — from check j + 1 and chunk j + 2 on, the fused
// and the residual launches carry a table of the open images only
// (ImageSet::active) and their grids shrink to those images.  The chunk
// in flight while check j was read still holds the image, which is what makes
// both of its ping-pong frames equal (see run_until_stable in the .cpp), so
// results, downloads and later runs are those of compact = false, byte for
// byte.  RunStats::image_launches shows the work that was retired.  A
// compacted launch never starts first-use tuning: it runs the tuned entry of
// its own image count if one exists, else the latency model's tile.
//
// Mixed sizes: the engine's geometry is then an ENVELOPE.  upload_sized puts
// images of any sizes within it top-left into their frames and hands every
// launch a table of their extents (ImageSet::dims): each image is
// convolved as a lone image of its own size, in the same ceil(reps / fuse)
// launches.  No frame is cleared in between — the kernels read nothing outside
// an image, so a larger image's stale bytes never leak.  The mode lasts until
// the next plain upload().
//
// Out of scope here (see docs/ARCHITECTURE.md §5): hipGraph capture, more than
// one GPU, a device-side rebuild of the active-image table (it would remove
// the one-chunk lag of compaction); and for mixed sizes and compaction the
// CLI, the service and the pipelines.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <vector>

#include "pconv/device.hpp"
#include "pconv/engine.hpp"
#include "pconv/filter.hpp"
#include "pconv/image.hpp"
#include "pconv/kernels.hpp"

namespace pconv {

// One image of a mixed-size upload, in pixels.
struct ImageSize {
  int64_t width = 0;
  int64_t height = 0;
};

// The host half of upload_sized, free of any device call: the extents table of
// `sizes` inside the envelope `env` for an engine of `capacity` frames
// (throws when there are too many images or one does not fit), and the bytes
// of the packed buffer that holds them back to back with tight rows.
std::vector<ImageDims> image_dims_table(const ImageGeom& env, int capacity, const std::vector<ImageSize>& sizes);
int64_t packed_bytes(const ImageGeom& env, const std::vector<ImageSize>& sizes);
// Bytes of the same images decimated by `factor`, packed the same way.
int64_t decimated_packed_bytes(const ImageGeom& env, const std::vector<ImageSize>& sizes, int factor);

class BatchEngine {
 public:
  // Options read: device, fuse, variant, border, compute_stream, timing,
  // kernel_copies (the rest describe bands and pipelines).
  BatchEngine(const ImageGeom& geom, const Filter& filter, int capacity, const EngineOptions& opt);
  ~BatchEngine();

  const ImageGeom& geom() const { return geom_; }
  const FrameLayout& layout() const { return lay_; }
  const EngineOptions& options() const { return opt_; }
  int capacity() const { return capacity_; }
  // Bytes between image b's and image b + 1's frame: a whole number of
  // pitches >= the frame's bytes (a frame is whole pitches, so exactly that).
  int64_t batch_stride() const { return stride_; }
  hipStream_t compute_stream() const { return cs_; }
  // Frame `which` (0/1) of image 0 at (row 0, data column 0); cur() = the newest.
  uint8_t* frame_at(int which) const { return frame_[which & 1].data() + lay_.offset(0); }
  int cur() const { return cur_; }

  // Copy n <= capacity packed images (row pitch row_bytes, images back to
  // back) into the current frames / the newest frames out.  Async on the
  // compute stream; a host pointer should be pinned.  `device`: p is device
  // memory.
  void upload(const uint8_t* p, int n, bool device = false);
  void download(uint8_t* p, int n, bool device = false);
  // Mixed sizes: `p` holds sizes.size() <= capacity images back to back with
  // tight rows, image b as sizes[b].height rows of sizes[b].width x channels
  // bytes, each within the engine's geometry (the envelope).  One pitched 2-D
  // copy per image, and the extents table goes to the device on the same
  // stream.  From here on run / residual / run_until_stable / time_residual
  // take n == sizes.size() and treat every image as a lone one of its size;
  // download_sized returns the newest frames' image regions in the same
  // packing.  The next plain upload() ends the mode.
  void upload_sized(const uint8_t* p, const std::vector<ImageSize>& sizes, bool device = false);
  void download_sized(uint8_t* p, bool device = false);
  // Decimated results (kernels.hpp launch_decimate, ONE launch for all images):
  // every factor-th pixel of every factor-th row of the newest frames.
  // download_decimated: n images of ceil(H / factor) x ceil(W / factor) pixels
  // back to back with tight rows.  download_sized_decimated: image b of the
  // current mixed-size upload as ceil(h_b / factor) rows of ceil(w_b / factor)
  // pixels, at offset sum_{i<b} out_h_i x out_w_i x pixel bytes.  The kernel
  // writes the caller's buffer where its layout allows (a uniform batch into
  // device memory), otherwise staging frames of the decimated envelope
  // (allocated on first use, never on a capturing stream) that one pitched
  // copy per image empties.  Factor 1 is download / download_sized.
  void download_decimated(uint8_t* p, int n, int factor, bool device = false);
  void download_sized_decimated(uint8_t* p, int factor, bool device = false);
  // Unsharp mask (kernels.hpp launch_unsharp) of images [0, n), ONE launch each:
  // snapshot_original(n) copies the current frames' rows into a third
  // allocation (first use, never on a capturing stream) after the upload and
  // before run(); apply_unsharp(k, threshold, n) then combines the newest
  // frames with them in place, image by image — a uniform batch through
  // `frames` and the stride, a mixed-size upload through its extents table —
  // so download / download_sized return the sharpened images.  Both refuse by
  // name while an active-image table is in force.
  void snapshot_original(int n);
  void apply_unsharp(int k, int threshold, int n);
  // Sizes of the current mixed-size upload (empty: uniform launches).
  const std::vector<ImageSize>& sizes() const { return sizes_; }
  // Enqueue `reps` repetitions of images [0, n) (async).
  void run(int reps, int n);

  // Per-image counts of the bytes one more repetition would change in the
  // newest frames of images [0, n): one residual launch.  Synchronises.
  std::vector<uint64_t> residual(int n);
  // Chunks of `check_every` repetitions of images [0, n) (the last one
  // shorter), a per-image residual check after each; ends when every image has
  // converged or at max_reps.  Entry b is what BandEngine::run_until_stable
  // returns for image b alone: an image whose count is zero for the first time
  // at check j is converged there (reps_done = the repetitions made by then,
  // checks = j, residual 0) and final — a later non-zero count for it is an
  // error; the others end with reps_done = max_reps, every check made and
  // their last count.  The frames hold max(reps made) repetitions, which for a
  // converged image are its fixed point's bytes.  last_stats() afterwards
  // carries the summed launches and the host-timed loop.
  //   compact: images found fixed are retired from the launches that follow
  // (the header comment); the returned entries and the frames' image bytes are
  // exactly those of compact = false, last_stats().image_launches is smaller.
  std::vector<StableStats> run_until_stable(int max_reps, int check_every, int n, bool compact = false);
  // Diagnostics: ms of each of `launches` residual launches over images [0, n)
  // of the current frames (stream events around the launch alone).
  std::vector<double> time_residual(int launches, int n);

  void wait_stream(hipStream_t s);
  void signal_stream(hipStream_t s);
  void synchronize();
  const RunStats& last_stats() const { return stats_; }

 private:
  // A table the launches read on the device: the pinned words it is copied out
  // of, the device region of `capacity` entries, and the event behind the
  // latest copy.  Allocated by the first stage(), never on a capturing stream.
  struct StagedTable {
    PinnedBuffer pin;
    DeviceBuffer dev;
    Event ev;
  };

  void check_n(const char* who, int n) const;
  // Flat copy / memset on the compute stream.
  void copy_words(uint8_t* dst, const uint8_t* src, size_t bytes, hipMemcpyKind kind);
  void zero_words(uint8_t* p, size_t bytes);
  // One pitched copy per image between `packed` and the current frames.
  void copy_images(bool to_frames, uint8_t* packed, int n, const ImageDims* extents, bool device);
  // The newest frames of images [0, n), decimated, into `packed` (in mixed
  // mode each at its own decimated extent).
  void decimate_images(uint8_t* packed, int n, int factor, bool device);
  DeviceBuffer dec_stage_;  // staging frames of the decimated envelope (first use, regrown)
  DeviceBuffer orig_;       // snapshot_original(): `capacity` frames laid out like frame_ (first use)
  int orig_n_ = 0;          // images the snapshot holds (0: none, or already consumed)
  // Rewrite `t` with n entries of entry_bytes each (`what` names it in errors).
  void stage(StagedTable& t, const char* what, const void* entries, size_t entry_bytes, size_t n);
  void upload_active(const std::vector<int32_t>& table);
  ImageTables image_tables(int n) const;
  StencilLaunch base_launch(int n) const;
  void launch_batch_residual(int n);
  void enqueue_residual(int n);
  std::vector<uint64_t> finish_residual(int n);

  ImageGeom geom_;
  Filter filter_;
  EngineOptions opt_;
  int capacity_ = 0;
  FrameLayout lay_;
  int64_t stride_ = 0;
  DeviceBuffer frame_[2];
  int cur_ = 0;
  DeviceBuffer res_count_;          // residual(): `capacity` 64-bit device counters (allocated on first use)
  PinnedBuffer res_host_;           // pinned words the running counts are read back into
  Event res_ev_;                    // the latest read-back has landed
  std::vector<uint64_t> res_seen_;  // the running counts at the latest check read
  // Mixed sizes: the extents of the current upload_sized (empty: uniform), as
  // given, as the host copy the guards read, and on the device.
  std::vector<ImageSize> sizes_;
  std::vector<ImageDims> dims_host_;
  StagedTable dims_;
  // Compaction: the open images of the run_until_stable in progress, in
  // increasing order (empty: every launch covers images [0, n)): the host
  // copy the guards read, and the device table.
  std::vector<int32_t> active_host_;
  StagedTable active_;
  Stream own_cs_;
  hipStream_t cs_ = nullptr;
  Event ev_t0_, ev_t1_, ev_sync_;
  RunStats stats_;
  double wall_t0_ = 0;
  bool timing_pending_ = false;
};

}  // namespace pconv
