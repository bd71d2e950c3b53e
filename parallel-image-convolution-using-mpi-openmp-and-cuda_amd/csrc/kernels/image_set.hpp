// Host side of a launch's images (ImageTables and ImageSet, pconv/kernels.hpp),
// shared by the kernel translation units: the launch guards, the four kernel
// arguments every batch-capable temporal kernel takes, and the tuners'
// live-workgroup count.  No HIP call and no device code: the guards also run
// stand-alone (tests/cpp/test_ragged_native.cpp).
#pragma once

#include <algorithm>
#include <cstdint>
#include <initializer_list>
#include <string>
#include <utility>

#include "pconv/common.hpp"
#include "pconv/kernels.hpp"

namespace pconv {

// Frames `stride` bytes apart (`name`: the stride's field) do not overlap: the
// stride holds `frame` ("a frame", "an output frame"), `frame_bytes` bytes.
inline void check_frames_apart(const std::string& who, const char* name, int64_t stride, const char* frame,
                               int64_t frame_bytes) {
  PCONV_CHECK(stride >= frame_bytes, who + ": " + name + " " + std::to_string(stride) + " is smaller than " + frame +
                                         " (" + std::to_string(frame_bytes) + " bytes): frames would overlap");
}

// At least one image in the grid, and frames that do not overlap: more than
// one frame lies at a 16-byte aligned stride that holds a whole frame —
// whatever the number of images an active-image table leaves in the grid.
inline void check_batch(const std::string& who, const StencilLaunch& a) {
  const ImageSet& s = a.images;
  PCONV_CHECK(s.images() >= 1, who + ": batch must be >= 1");
  if (s.frames <= 1) return;
  PCONV_CHECK(s.stride % 16 == 0, who + ": batch_stride must be a multiple of 16");
  check_frames_apart(who, "batch_stride", s.stride, "a frame", (a.frame_hi - a.frame_lo) * a.pitch);
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

// A launch that covers every frame takes no active-image table; `verb`: what
// it does to each ("decimated", "sharpened").
inline void check_no_active(const std::string& who, const ImageTables& s, const char* verb) {
  PCONV_CHECK(!s.has_table(),
              who + ": an active table is not supported (every frame of the set is " + verb + ")");
}

// The extents table comes with its host copy, the launch covers whole images
// (`whole`; `whole_rule` names what that asks of this launch), and every
// frame's image — named by an active-image table or not — is a whole number
// of `unit`-byte `noun` ("pixels", "samples") inside the envelope of
// row_bytes x rows.
inline void check_extents(const std::string& who, const ImageTables& s, int64_t row_bytes, int64_t rows, int unit,
                          const char* noun, bool whole = true, const char* whole_rule = "") {
  PCONV_CHECK((s.dims == nullptr) == (s.dims_host == nullptr),
              who + ": dims and dims_host must be given together (the device table and its host copy)");
  if (!s.dims) return;
  PCONV_CHECK(whole, who + ": dims needs whole images (" + whole_rule + ")");
  for (int b = 0; b < s.dims_entries(); ++b) {
    const ImageDims& d = s.dims_host[b];
    PCONV_CHECK(d.row_bytes >= unit && d.row_bytes <= row_bytes && d.row_bytes % unit == 0,
                who + ": dims[" + std::to_string(b) + "].row_bytes " + std::to_string(d.row_bytes) +
                    " is no whole number of " + noun + " inside the envelope's " + std::to_string(row_bytes));
    PCONV_CHECK(d.height >= 1 && d.height <= rows,
                who + ": dims[" + std::to_string(b) + "].height " + std::to_string(d.height) +
                    " is outside [1, the envelope's " + std::to_string(rows) + "]");
  }
}

// check_extents for a temporal or residual launch.  `ch`: bytes per pixel.
inline void check_dims(const std::string& who, const StencilLaunch& a, int ch) {
  check_extents(who, a.images, a.row_bytes, a.height, ch, "pixels", a.g_row0 == 0 && a.r0 == 0 && a.r1 == a.height,
                "g_row0 = 0, r0 = 0, r1 = height");
}

// A flat, image-major grid of `images` x (bx x by) workgroups fits one launch.
inline void check_flat_grid(const std::string& who, int64_t bx, int64_t by, int64_t images) {
  PCONV_CHECK(bx * by < (int64_t(1) << 31) && bx * by * images < (int64_t(1) << 31),
              who + ": too many workgroups for one grid (images x blocks per image)");
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
