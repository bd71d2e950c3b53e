// Host side of StencilLaunch::images (ImageSet, pconv/kernels.hpp), shared by
// the kernel translation units: the launch guards, the four kernel arguments
// every batch-capable kernel takes, and the tuners' live-workgroup count.
#pragma once

#include <algorithm>
#include <cstdint>
#include <initializer_list>
#include <string>
#include <utility>

#include "pconv/common.hpp"
#include "pconv/kernels.hpp"

namespace pconv {

// At least one image in the grid, and frames that do not overlap: more than
// one frame lies at a 16-byte aligned stride that holds a whole frame —
// whatever the number of images an active-image table leaves in the grid.
inline void check_batch(const std::string& who, const StencilLaunch& a) {
  const ImageSet& s = a.images;
  PCONV_CHECK(s.images() >= 1, who + ": batch must be >= 1");
  if (s.frames <= 1) return;
  PCONV_CHECK(s.stride % 16 == 0, who + ": batch_stride must be a multiple of 16");
  PCONV_CHECK(s.stride >= (a.frame_hi - a.frame_lo) * a.pitch,
              who + ": batch_stride " + std::to_string(s.stride) + " is smaller than a frame (" +
                  std::to_string((a.frame_hi - a.frame_lo) * a.pitch) + " bytes): frames would overlap");
}

// The active-image table comes with its host copy and holds `count` strictly
// increasing frame indices inside [0, frames): no two grid slots name one
// frame.  (The frames' stride rules are check_batch's.)
inline void check_active(const std::string& who, const StencilLaunch& a) {
  const ImageSet& s = a.images;
  PCONV_CHECK((s.active == nullptr) == (s.active_host == nullptr),
              who + ": active and active_host must be given together (the device table and its host copy)");
  if (!s.active) return;
  PCONV_CHECK(s.count >= 1, who + ": active needs batch >= 1 entries");
  PCONV_CHECK(s.count <= s.frames, who + ": active holds " + std::to_string(s.count) +
                                       " entries, more than batch_frames " + std::to_string(s.frames));
  for (int k = 0; k < s.count; ++k) {
    const int32_t e = s.active_host[k];
    PCONV_CHECK(e >= 0 && e < s.frames, who + ": active[" + std::to_string(k) + "] = " + std::to_string(e) +
                                            " is outside [0, batch_frames " + std::to_string(s.frames) + ")");
    PCONV_CHECK(k == 0 || e > s.active_host[k - 1],
                who + ": active[" + std::to_string(k) + "] = " + std::to_string(e) +
                    " does not exceed the entry before it (the table must be strictly increasing)");
  }
}

// The extents table comes with its host copy, the launch covers whole images,
// and every frame's image — named by an active-image table or not — is whole
// pixels inside the envelope.  `ch`: bytes per pixel.
inline void check_dims(const std::string& who, const StencilLaunch& a, int ch) {
  const ImageSet& s = a.images;
  PCONV_CHECK((s.dims == nullptr) == (s.dims_host == nullptr),
              who + ": dims and dims_host must be given together (the device table and its host copy)");
  if (!s.dims) return;
  PCONV_CHECK(a.g_row0 == 0 && a.r0 == 0 && a.r1 == a.height,
              who + ": dims needs whole images (g_row0 = 0, r0 = 0, r1 = height)");
  for (int b = 0; b < s.dims_entries(); ++b) {
    const ImageDims& d = s.dims_host[b];
    PCONV_CHECK(d.row_bytes >= ch && d.row_bytes <= a.row_bytes && d.row_bytes % ch == 0,
                who + ": dims[" + std::to_string(b) + "].row_bytes " + std::to_string(d.row_bytes) +
                    " is no whole number of pixels inside the envelope's " + std::to_string(a.row_bytes));
    PCONV_CHECK(d.height >= 1 && d.height <= a.height,
                who + ": dims[" + std::to_string(b) + "].height " + std::to_string(d.height) +
                    " is outside [1, the envelope's " + std::to_string(a.height) + "]");
  }
}

// All guards of a launch's image set, in the one order every entry point
// reports them: the frames (check_batch), then the table that picks among them
// (check_active; from here on its entries may be read), then the extents
// (check_dims).  `a` is the launch AS GIVEN, before its rows are clipped to
// the global image: check_dims insists on whole images.  Called once per
// public entry point (launch_stencil, launch_float_temporal, launch_residual).
inline void check_image_set(const std::string& who, const StencilLaunch& a, int ch) {
  check_batch(who, a);
  check_active(who, a);
  check_dims(who, a, ch);
}

// launch_float_temporal for a launch whose image set launch_stencil has
// checked already (kernels/stencil_float.hip).
void launch_float_temporal_checked(const Filter& f, Channels ch, const StencilLaunch& a, hipStream_t stream);

// What only the temporal kernels implement, asked of the single-step variant
// named `variant`: "<who>: <name> not supported by kernel '<variant>' (temporal
// and float_temporal only)" for the first feature of the list that is present.
inline void check_temporal_only(const std::string& who, const char* variant,
                                std::initializer_list<std::pair<std::string, bool>> features) {
  for (const auto& f : features)
    PCONV_CHECK(!f.second, who + ": " + f.first + " not supported by kernel '" + variant +
                               "' (temporal and float_temporal only)");
}

// The image-set arguments of k_swar, k_swar_pf, k_float_temporal and
// k_residual, in the kernels' order.  A lone frame passes stride 0 (the
// kernels then add nothing to the base pointers); last_frame is what the
// kernels clamp a table's entries to and 0 without a table.
struct BatchKernelArgs {
  int64_t stride;
  const ImageDims* dims;
  const int32_t* active;
  unsigned last_frame;
};
inline BatchKernelArgs batch_kernel_args(const StencilLaunch& a) {
  const ImageSet& s = a.images;
  return {s.frames > 1 || s.has_table() ? s.stride : int64_t(0), s.dims, s.active,
          s.has_table() ? static_cast<unsigned>(s.frames - 1) : 0u};
}

// Workgroups of a mixed-size launch that have output in their image, for a
// grid whose workgroup covers vbytes x vrows of output and packs `fold` column
// strips (2: the SWAR strip pairs).  The tuners key on it (0: no dims), so a
// uniform launch never shares a cache entry with a mixed one.  The count runs
// over the grid's images: with an active-image table, the frames it names.
inline int64_t live_workgroups(const StencilLaunch& a, int64_t vbytes, int64_t vrows, int fold) {
  const ImageSet& s = a.images;
  if (!s.dims_host || vbytes <= 0 || vrows <= 0) return 0;
  int64_t live = 0;
  for (int k = 0; k < s.images(); ++k) {
    const ImageDims& d = s.dims_host[s.frame_of(k)];
    const int64_t strips = ceil_div<int64_t>(d.row_bytes, vbytes);
    // strip pair `col` holds strips col and col + pair_stride: it is live when its strip A is
    const int64_t pair_stride = (ceil_div<int64_t>(a.row_bytes, vbytes) + fold - 1) / fold;
    live += std::min(strips, pair_stride) * ceil_div<int64_t>(d.height, vrows);
  }
  return live;
}

}  // namespace pconv
