// Host-side helpers shared by the kernel translation units: run-time value ->
// template argument dispatch, and the first-use tuner's measuring loop.
#pragma once

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstddef>
#include <type_traits>
#include <utility>
#include <vector>

#include <string>

#include "pconv/common.hpp"
#include "pconv/device.hpp"
#include "pconv/kernels.hpp"

namespace pconv {

// f(std::integral_constant<int, bytes per pixel>) for the channel layout.
template <class F>
decltype(auto) with_channels(Channels ch, F&& f) {
  switch (ch) {
    case Channels::Grey: return f(std::integral_constant<int, 1>{});
    case Channels::Rgb: return f(std::integral_constant<int, 3>{});
    case Channels::Rgba: break;
  }
  return f(std::integral_constant<int, 4>{});
}

// f(std::integral_constant<size_t, i>) for a run-time i < N; false (f not
// called) for any other i.  A kernel family's constexpr shape table goes
// through this: f is compiled for every row, so a row IS an instantiation, and
// a shape outside the table has nothing to dispatch to.
template <class F, size_t... I>
bool with_index(size_t i, F&& f, std::index_sequence<I...>) {
  return ((i == I && (f(std::integral_constant<size_t, I>{}), true)) || ...);
}
template <size_t N, class F>
bool with_index(size_t i, F&& f) {
  return with_index(i, f, std::make_index_sequence<N>{});
}

// Nothing may be timed (or synchronised) on a stream that is being captured
// into a graph: the engine tunes a step's launches before it captures them.
inline bool stream_capturing(hipStream_t s) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(s, &st) == hipSuccess && st != hipStreamCaptureStatusNone;
}

// Guards of an image batch (StencilLaunch::batch), shared by the launches that
// take one: the frames of a batch lie at a 16-byte aligned stride that holds a
// whole frame, so no two images' frames overlap.
inline void check_batch(const std::string& who, const StencilLaunch& a) {
  PCONV_CHECK(a.batch >= 1, who + ": batch must be >= 1");
  if (a.batch == 1) return;
  PCONV_CHECK(a.batch_stride % 16 == 0, who + ": batch_stride must be a multiple of 16");
  PCONV_CHECK(a.batch_stride >= (a.frame_hi - a.frame_lo) * a.pitch,
              who + ": batch_stride " + std::to_string(a.batch_stride) + " is smaller than a frame (" +
                  std::to_string((a.frame_hi - a.frame_lo) * a.pitch) + " bytes): frames would overlap");
}

// Frame of the k-th image of a launch's grid: k itself, or entry k of the
// active-image table (StencilLaunch::active; check_active comes first).
inline int frame_of(const StencilLaunch& a, int k) { return a.active_host ? a.active_host[k] : k; }

// Guards of an active-image table (StencilLaunch::active), shared by the
// launches that take one: the table comes with its host copy, holds `batch`
// strictly increasing frame indices inside [0, batch_frames) — no two grid
// slots name one frame — and the frames obey the stride rules of a batch
// whenever there is more than one of them, whatever the number of entries.
// The kernels clamp the device entries to batch_frames - 1 themselves, so a
// device table that differs from the host copy still stays in the allocation.
inline void check_active(const std::string& who, const StencilLaunch& a) {
  PCONV_CHECK((a.active == nullptr) == (a.active_host == nullptr),
              who + ": active and active_host must be given together (the device table and its host copy)");
  if (!a.active) return;
  PCONV_CHECK(a.batch >= 1, who + ": active needs batch >= 1 entries");
  PCONV_CHECK(a.batch <= a.batch_frames, who + ": active holds " + std::to_string(a.batch) +
                                             " entries, more than batch_frames " + std::to_string(a.batch_frames));
  for (int k = 0; k < a.batch; ++k) {
    const int32_t e = a.active_host[k];
    PCONV_CHECK(e >= 0 && e < a.batch_frames, who + ": active[" + std::to_string(k) + "] = " + std::to_string(e) +
                                                  " is outside [0, batch_frames " + std::to_string(a.batch_frames) + ")");
    PCONV_CHECK(k == 0 || e > a.active_host[k - 1],
                who + ": active[" + std::to_string(k) + "] = " + std::to_string(e) +
                    " does not exceed the entry before it (the table must be strictly increasing)");
  }
  if (a.batch_frames > 1) {
    StencilLaunch frames = a;  // the stride rules of batch_frames frames
    frames.batch = a.batch_frames;
    check_batch(who, frames);
  }
}

// Guards of a mixed-size batch (StencilLaunch::dims), shared by the launches
// that take one: the table comes with its host copy, the launch covers whole
// images, and every image is whole pixels inside the envelope.  `ch`: bytes
// per pixel.  The kernels clamp the device entries to the envelope themselves,
// so a device table that differs from the host copy still stays in the frame.
// The table is indexed by FRAME: with an active-image table it has
// batch_frames entries (check_active comes first), all of them checked.
inline void check_dims(const std::string& who, const StencilLaunch& a, int ch) {
  PCONV_CHECK((a.dims == nullptr) == (a.dims_host == nullptr),
              who + ": dims and dims_host must be given together (the device table and its host copy)");
  if (!a.dims) return;
  PCONV_CHECK(a.g_row0 == 0 && a.r0 == 0 && a.r1 == a.height,
              who + ": dims needs whole images (g_row0 = 0, r0 = 0, r1 = height)");
  const int entries = a.active_host ? a.batch_frames : a.batch;
  for (int b = 0; b < entries; ++b) {
    const ImageDims& d = a.dims_host[b];
    PCONV_CHECK(d.row_bytes >= ch && d.row_bytes <= a.row_bytes && d.row_bytes % ch == 0,
                who + ": dims[" + std::to_string(b) + "].row_bytes " + std::to_string(d.row_bytes) +
                    " is no whole number of pixels inside the envelope's " + std::to_string(a.row_bytes));
    PCONV_CHECK(d.height >= 1 && d.height <= a.height,
                who + ": dims[" + std::to_string(b) + "].height " + std::to_string(d.height) +
                    " is outside [1, the envelope's " + std::to_string(a.height) + "]");
  }
}

// Workgroups of a mixed-size launch that have output in their image, for a
// grid whose workgroup covers vbytes x vrows of output and packs `fold` column
// strips (2: the SWAR strip pairs).  The tuners key on it (0: no dims), so a
// uniform launch never shares a cache entry with a mixed one.  With an
// active-image table the count runs over the frames the table names.
inline int64_t live_workgroups(const StencilLaunch& a, int64_t vbytes, int64_t vrows, int fold) {
  if (!a.dims_host || vbytes <= 0 || vrows <= 0) return 0;
  int64_t live = 0;
  for (int b = 0; b < a.batch; ++b) {
    const ImageDims& d = a.dims_host[frame_of(a, b)];
    const int64_t strips = ceil_div<int64_t>(d.row_bytes, vbytes);
    // strip pair `col` holds strips col and col + pair_stride: it is live when its strip A is
    const int64_t pair_stride = (ceil_div<int64_t>(a.row_bytes, vbytes) + fold - 1) / fold;
    live += std::min(strips, pair_stride) * ceil_div<int64_t>(d.height, vrows);
  }
  return live;
}

constexpr int kTuneRepeats = 3;
constexpr int kTunePasses = 2;

// Index of the fastest of n candidates (the first of equals); launch(i)
// enqueues candidate i on `stream`.  The candidates run the REAL launch (same
// src -> dst, so the repeats are harmless: every run writes the same bytes).
// Two interleaved passes, each candidate's best kept: a single pass in a
// fixed order mis-ranked large launches (the first candidates ran while
// clocks and caches were still settling; 32768^2 grey picked a shape 7 %
// slower than the best).
template <class Launch>
size_t fastest_candidate(size_t n, hipStream_t stream, Launch&& launch) {
  if (n <= 1) return 0;
  Event e0 = Event::create(true), e1 = Event::create(true);
  std::vector<float> t(n, 1e30f);
  for (int pass = 0; pass < kTunePasses; ++pass) {
    for (size_t i = 0; i < n; ++i) {
      if (pass == 0) launch(i);  // warm (code object, caches)
      e0.record(stream);
      for (int r = 0; r < kTuneRepeats; ++r) launch(i);
      e1.record(stream);
      PCONV_HIP_CHECK(hipEventSynchronize(e1.get()));
      t[i] = std::min(t[i], Event::elapsed_ms(e0, e1));
    }
  }
  return static_cast<size_t>(std::min_element(t.begin(), t.end()) - t.begin());
}

}  // namespace pconv
