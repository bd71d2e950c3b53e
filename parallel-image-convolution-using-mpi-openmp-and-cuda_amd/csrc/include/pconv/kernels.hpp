// Device stencil kernels (CDNA4 / gfx950) — host-side launch interface.
//
// Reference kernels: kernelConvolutionforGrey / kernelConvolutionforRGB
// (cuda/cuda_convolution.cu:9-47): one thread per pixel with lanes walking
// down ROWS (uncoalesced), FP64 /16.0, border ring never written, RGB grid 3x
// too wide with out-of-bounds accesses.
//
// pconv kernels treat a row as a byte vector (RGB = 3W bytes, horizontal tap
// stride = CH bytes), so one template serves grey/RGB/RGBA:
//   * lanes walk along a row, 16 bytes per lane (dwordx4 loads/stores);
//   * the gaussian runs in packed 16-bit integer SIMD (v_perm_b32 byte
//     unpack, v_pk_add_u16 / v_pk_mad_u16, shift, v_perm_b32 repack), exactly
//     reproducing the float32 reference;
//   * each lane marches down RPT rows keeping the horizontal sums of the last
//     two rows in registers (every input row is loaded and unpacked once);
//   * the temporal-blocked SWAR kernel fuses `steps` repetitions in one
//     launch (kernels/stencil_swar.hip).
// The frame's zero pad (image.hpp) provides the boundary; no edge branches.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <utility>
#include <vector>

#include "pconv/filter.hpp"
#include "pconv/image.hpp"

namespace pconv {

// Extent of one image of a mixed-size batch inside its frame (device table of
// the temporal and residual kernels, host copy for the guards): 8 bytes.
struct ImageDims {
  int32_t row_bytes;
  int32_t height;
};

struct StencilLaunch {
  const uint8_t* src = nullptr;  // frame: owned row 0, data column 0
  uint8_t* dst = nullptr;        // same layout as src
  int64_t pitch = 0;
  int64_t row_bytes = 0;
  int64_t r0 = 0, r1 = 0;        // output rows [r0, r1) in frame-local numbering
  int64_t frame_lo = 0;          // first readable frame row (= -halo)
  int64_t frame_hi = 0;          // one past the last readable frame row (= rows + halo)
  int steps = 1;                 // fused repetitions (temporal blocking) in this launch
  int64_t g_row0 = 0;            // global image row of frame row 0
  int64_t height = 0;            // global image height (rows outside are zero each step)
  // Rule at the global image's edges.  Replicate is built into the temporal
  // kernels only (they apply it at every fused step): Auto routes every step
  // count to them, the single-step variants reject it.
  Border border = Border::Zero;
  // Image batch (temporal kernels and the residual kernel): `batch` independent images of this
  // geometry advance in the one launch.  Every other field describes ONE image
  // and applies to each; image b's frame lies b * batch_stride bytes after
  // image 0's, in src and dst alike (ignored when batch == 1).  Images never
  // read each other's rows: the batch only moves the base pointers.
  int batch = 1;
  int64_t batch_stride = 0;
  // Mixed sizes (temporal kernels and the residual kernel): every field above
  // is then the ENVELOPE all frames share, and image b occupies rows
  // [0, dims[b].height) and bytes [0, dims[b].row_bytes) of its frame, top-left
  // aligned.  It is convolved exactly as a lone image of that size under
  // either border: whatever the rest of its frame holds (pad columns, ghost
  // rows, a larger image's stale bytes) reads as out-of-image, and nothing of
  // the destination frame outside the image is written.  `dims` is device
  // memory of `batch` entries (the kernels clamp each entry to the envelope),
  // `dims_host` the host copy of the same entries the guards read; both or
  // neither.  Null: every image is the envelope.  Whole images only
  // (g_row0 = 0, r0 = 0, r1 = height); batch = 1 is allowed.
  const ImageDims* dims = nullptr;
  const ImageDims* dims_host = nullptr;
  // Active images (temporal kernels and the residual kernel): a launch over
  // SOME of the `batch_frames` frames that lie batch_stride apart.  `batch` is
  // then the number of table entries and the grid is that many images wide;
  // entry k is the frame index of the grid's k-th image, whose frame lies
  // active[k] * batch_stride after frame 0 (in src and dst alike; the residual
  // kernel adds to counter[active[k]]).  Frames the table does not name are
  // neither read nor written, and their counters are not touched.  The entries
  // are strictly increasing inside [0, batch_frames).  `active` is device
  // memory (the kernels clamp each entry to batch_frames - 1), `active_host`
  // the host copy the guards read; both or neither.  `dims` stays indexed by
  // FRAME: with a table it has batch_frames entries.  Null: image k is frame k
  // and batch_frames is ignored.  A launch with a table runs its model's tile
  // (or the tuned entry of its own key, if one exists) and never starts
  // first-use tuning.
  const int32_t* active = nullptr;
  const int32_t* active_host = nullptr;
  int batch_frames = 1;
};

enum class KernelVariant : int {
  Auto = 0,      // pick by filter / steps
  Binomial = 1,  // packed-u16 gaussian, 1 step per launch
  Temporal = 2,  // SWAR-32 gaussian, `steps` fused in registers (production)
  Int9 = 3,      // generic int-exact 9-tap
  Float9 = 4,    // generic float32 9-tap (reference rounding)
  FloatTemporal = 6,  // any 3x3 filter, float32 reference rounding, `steps` fused in registers
};

const char* kernel_variant_name(KernelVariant v);

// Largest `steps` the temporal kernel accepts.
constexpr int kMaxFusedSteps = 16;

// Enqueue one stencil launch on `stream`.  Validates the geometry against the
// frame before launching (no out-of-frame access is possible).
void launch_stencil(const Filter& f, Channels ch, const StencilLaunch& a, hipStream_t stream,
                    KernelVariant v = KernelVariant::Auto);
// Settle per-launch choices (SWAR tile-shape tuning) for a launch that will be
// enqueued later — e.g. inside a graph capture, where nothing may be timed.
void prepare_stencil(const Filter& f, Channels ch, const StencilLaunch& a, hipStream_t stream,
                     KernelVariant v = KernelVariant::Auto);

// `steps` repetitions of ANY 3x3 filter in the reference's float32 semantics
// in one launch (kernels/stencil_float.hip): box/9, edge/28, custom filters.
void launch_float_temporal(const Filter& f, Channels ch, const StencilLaunch& a, hipStream_t stream);
// Tune the float kernel's tile shape for this launch geometry now (before a
// graph capture).
void prepare_float_temporal(const Filter& f, Channels ch, const StencilLaunch& a, hipStream_t stream);

// Residual of the iterated map at the frame `a.src` (kernels/residual.hip):
// one repetition of `f` under `a.border` is evaluated in registers for rows
// [a.r0, a.r1) and the bytes of [0, row_bytes) with step(x) != x are counted.
// Nothing is stored but the count, ADDED to *counter (device memory, zeroed by
// the caller): zero means the rows are a fixed point of the repetition.  Reads
// src, pitch, row_bytes, r0, r1, frame_lo, frame_hi, g_row0, height, border,
// batch and batch_stride (dst and steps are ignored); the rows are clipped to
// the global image and validated against the frame like a one-step
// launch_stencil.
// Image batch: `counter` points at a.batch consecutive 64-bit counters and
// image b's count (its frame b * batch_stride bytes after image 0's) is ADDED
// to counter[b], all in the one launch; no counter beyond a.batch is touched.
// The batch guards are launch_stencil's (check_batch), every geometry guard
// holds per image, and batch x workgroups per image must stay below 2^31.
// With an active-image table (a.active) `counter` points at a.batch_frames
// counters, the grid's k-th image adds to counter[active[k]], and the counters
// of frames the table does not name are not touched.
void launch_residual(const Filter& f, Channels ch, const StencilLaunch& a, uint64_t* counter, hipStream_t stream);
// Rows one workgroup of the residual kernel covers (tests place image heights around it).
constexpr int kResidualBlockRows = 32;

// Whether `v` (or Auto) can fuse `steps` > 1 for this filter.
bool supports_fusion(const Filter& f, KernelVariant v);

// Default repetitions per launch for a band frame of `frame_bytes`: 1 without
// fusion; 12 for grey frames of 256 MiB and more (far beyond the Infinity
// Cache: 32768^2 grey 113.2-116.2 us/rep at 12 vs 116.9-121.1 at 8 over four
// boxes, 16384^2 30.6 vs 32.2; profiles/r02/tile_shapes.md,
// prefetch_kernel.md); 8 everywhere else (RGB's 3x wider horizontal halo makes
// deeper fusion slower; 1920x2520 RGB 3.5 us/rep at 8 vs 4.0 at 6, 8192^2 RGB
// within 2 % either way).  Other filters (float temporal kernel): 4.
int auto_fuse(const Filter& f, KernelVariant v, int64_t frame_bytes, int channels = 0);

// Row copy by the CUs: `rows` rows of `row_bytes` from src (row pitch sp) to
// dst (row pitch dp); either side may be pinned host memory (the CUs move the
// bytes over PCIe) or device memory.  No SDMA engine and no runtime blit
// program is involved — a one-shot process saves their first-use set-up
// (~8 ms per SDMA direction and the blit code object, profiles/r02/), at
// 44-53 GB/s instead of SDMA's 54 (tools/ubench/copy_bw.hip).
// max_blocks > 0 caps the grid (a copy beside stencil launches leaves them CUs).
void launch_copy_rows(const uint8_t* src, int64_t sp, uint8_t* dst, int64_t dp, int64_t row_bytes, int64_t rows,
                      hipStream_t stream, int max_blocks = 0);
// Zero `bytes` (a multiple of 16, 16-byte aligned) with a kernel of this module.
void launch_fill_zero(uint8_t* p, int64_t bytes, hipStream_t stream);
// Load the code object of the temporal / copy kernels now (a one-shot process
// calls it from a helper thread while it creates its first hardware queue).
void preload_kernel_module();

// ---- Tile shapes and their first-use tuning, for both temporal kernels ----
// Each family's shapes are one constexpr table in its translation unit; the
// lists below, the launch dispatch and the tuners' candidates all come from it.

// Tile of the SWAR kernel: lw bytes per lane per strip (4 or 8), m rows per
// wave, nw waves stacked vertically per workgroup.
struct SwarShape {
  int lw = 8, m = 8, nw = 8;
};
// Tile of the float temporal kernel: m rows per wave (8 bytes per lane), nw waves.
struct FloatShape {
  int m, nw;
};
// The instantiated shapes: the SWAR tile kernel's, those of them the buffer-op
// kernel k_swar_pf has too, and the float kernel's (largest tile first).
std::vector<SwarShape> swar_shapes();
std::vector<SwarShape> swar_prefetch_shapes();
std::vector<FloatShape> float_shapes();

// Empirical tile-shape tuning on / off (off: the latency model's pick);
// returns the previous setting.  A one-shot process turns it off: timing a
// dozen candidates costs more than the loop they would speed up.
bool set_shape_tuning(bool on);
bool shape_tuning_enabled();
// How many of the model's best SWAR shapes the tuner times (default 6).
void set_tune_candidates(int n);
// Force a tile shape.  SWAR: lw = 0 restores the model, an unknown shape is an
// error.  Float: m = 0 restores the model / tuner, an unknown shape is ignored.
void set_swar_shape(int lw, int m, int nw);
void set_float_shape(int m, int nw);
// Forget the tuned shapes: of both kernels, of the float kernel alone.
void clear_swar_tuning();
void clear_float_tuning();
// Tuned SWAR entries: ({channels, steps, rows, row_bytes, step_form, kernel, batch, live}, shape); kernel 0: the
// tile kernel k_swar, 1: the buffer-op tile kernel k_swar_pf; live: the workgroups of a mixed-size launch
// (StencilLaunch::dims) that have output in their image, 0 for a uniform launch.
std::vector<std::pair<std::vector<int64_t>, SwarShape>> swar_tuned();

}  // namespace pconv
