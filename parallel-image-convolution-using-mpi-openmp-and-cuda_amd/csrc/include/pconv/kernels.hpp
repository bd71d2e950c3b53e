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
// the kernels, host copy for the guards): 8 bytes.
struct ImageDims {
  int32_t row_bytes;
  int32_t height;
};

// The images of one launch: which frames exist, which of them the grid covers,
// and how much of each frame is image.  Every other field of a launch struct
// describes ONE frame and applies to each.  ImageTables is the part every
// launch over frames shares (the pointwise launches carry it as it is, beside a
// stride per operand); ImageSet adds the one stride of the temporal and
// residual kernels.
//   frames: frames of the launch's geometry, at the launch's stride(s).
//   active / active_host / count: optional table of `count` strictly increasing
// frame indices inside [0, frames).  With it the grid is `count` images wide
// and its k-th image is frame active[k]; frames the table does not name are
// neither read nor written, and their counters are not touched.  Without it
// the grid covers every frame in order (`count` is not read).  A launch with a
// table runs its model's tile (or the tuned entry of its own key, if one
// exists) and never starts first-use tuning.
//   dims / dims_host: optional table of `frames` extents, indexed by FRAME.
// With it the launch's geometry is the ENVELOPE all frames share and frame b's
// image occupies rows [0, dims[b].height) and bytes [0, dims[b].row_bytes),
// top-left aligned.  It is convolved exactly as a lone image of that size
// under either border: whatever the rest of its frame holds reads as
// out-of-image, and nothing of the destination frame outside the image is
// written.  Whole images only (g_row0 = 0, r0 = 0, r1 = height).
//   Each table is device memory the kernels read (they clamp every entry, to
// frames - 1 and to the envelope, so a wrong table stays inside the
// allocation) plus the host copy of the same entries the guards and tuners
// read; both pointers or neither.
struct ImageTables {
  int frames = 1;
  const int32_t* active = nullptr;
  const int32_t* active_host = nullptr;
  int count = 0;
  const ImageDims* dims = nullptr;
  const ImageDims* dims_host = nullptr;

  bool has_table() const { return active || active_host; }
  bool has_dims() const { return dims || dims_host; }
  // Images in the grid, and the frame of its k-th image (after the guards).
  int images() const { return has_table() ? count : frames; }
  int frame_of(int k) const { return active_host ? active_host[k] : k; }
  // Entries of dims / dims_host.
  int dims_entries() const { return frames; }
};

//   stride: the frames lie `stride` bytes apart, in src and dst alike (the
// residual kernel's counters number the same); frame b starts b * stride after
// frame 0.  More than one frame needs a 16-byte aligned stride that holds a
// whole frame.  Images never read each other's rows: the set only moves the
// base pointers.
struct ImageSet : ImageTables {
  int64_t stride = 0;
  // One plain image: nothing here that only the temporal kernels read.
  bool single() const { return frames <= 1 && !has_table() && !has_dims(); }
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
  // Bits per sample, 8 | 16.  16: rows hold unsigned 16-bit samples in host
  // byte order, a pixel is 2 x channels bytes, row_bytes and every
  // ImageDims::row_bytes are whole pixels; the gaussian only, on the 16-bit
  // temporal kernel (kernels/stencil_swar16.hip) for every step count.
  int depth = 8;
  ImageSet images;
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
// Nothing is stored but the count, ADDED to a counter (device memory, zeroed by
// the caller): zero means the rows are a fixed point of the repetition.  Reads
// src, pitch, row_bytes, r0, r1, frame_lo, frame_hi, g_row0, height, border
// and images (dst and steps are ignored); the rows are clipped to the global
// image and validated against the frame like a one-step launch_stencil.
// `counter` points at a.images.frames consecutive 64-bit counters: the count of
// every image of the grid is ADDED to its FRAME's counter, all in the one
// launch, and no other counter is touched.  The image-set guards are
// launch_stencil's, every geometry guard holds per image, and images x
// workgroups per image must stay below 2^31.
void launch_residual(const Filter& f, Channels ch, const StencilLaunch& a, uint64_t* counter, hipStream_t stream);
// Rows one workgroup of the residual kernel covers (tests place image heights around it).
constexpr int kResidualBlockRows = 32;

// Decimation (kernels/decimate.hip): out[Y][X] = frame[first + Y * s][X * s],
// whole pixels of `pixel_bytes` (channels x depth / 8: 1, 2, 3, 4, 6 or 8),
// phase 0.  Frame row r is kept when (g_row0 + r) % s == 0, so the bands of an
// image select by GLOBAL row; columns are never split.  The output of a frame
// of `rows` x `row_bytes` has ceil((rows - first) / s) rows of
// ceil(row_bytes / pixel_bytes / s) pixels and sits top-left in its
// destination frame; no other destination byte is written, no source byte
// outside [0, row_bytes) of the rows is read, and only selected source rows are
// addressed at all.
//   src / src_pitch / row_bytes / rows / g_row0: one pitched source frame, src
// at (row 0, data column 0).  dst / dst_pitch: one pitched destination;
// dst_bytes: the size of what dst points into, which the guards hold every
// frame's output against.
//   images / src_stride / dst_stride: the frames (ImageTables above), source
// frames src_stride bytes apart going to destination frames dst_stride apart,
// all in one launch.  images.dims holds SOURCE extents (the geometry above is
// then the envelope, g_row0 = 0); image b's output extent is the ceil of its
// own extent, derived in the kernel.  An active table is refused by name: a
// decimation covers every frame.
// The source base, pitch and stride must be multiples of the load width (4 for
// 4- and 8-byte pixels, 2 for 2 and 6); a destination whose base, pitch and
// stride are multiples of 4 gets dword stores, any other byte stores.
// Every guard is named "launch_decimate: ..."; a refused launch writes nothing.
struct DecimateLaunch {
  const uint8_t* src = nullptr;
  int64_t src_pitch = 0;
  int64_t row_bytes = 0;
  int64_t rows = 0;
  int64_t g_row0 = 0;
  uint8_t* dst = nullptr;
  int64_t dst_pitch = 0;
  int64_t dst_bytes = 0;
  int pixel_bytes = 1;
  int factor = 1;
  ImageTables images;
  int64_t src_stride = 0;
  int64_t dst_stride = 0;
};
void launch_decimate(const DecimateLaunch& a, hipStream_t stream);
// Output rows one workgroup of k_decimate covers (tests place heights around
// it); the factor's range and decimated_extent are image.hpp's.
constexpr int kDecimateBlockRows = 16;

// Unsharp mask (kernels/unsharp.hip): per sample, with x from `orig`, b from
// `blur`, d = x - b and max = 255 (depth 8) or 65535 (depth 16, host byte order),
//   dst = x                                           if |d| < threshold
//   dst = clamp((x (16 + k) - b k + 8) >> 4, 0, max)  otherwise
// (arithmetic shift, 32-bit integers): x + (k / 16)(x - b), rounded to nearest.
// Only [0, row_bytes) of rows [0, rows) of a destination frame is written; the
// row's last lane LOADS up to round_up(row_bytes, 16) of both sources, which
// the guards keep inside every pitch.
//   orig / orig_pitch, blur / blur_pitch, dst / dst_pitch: three pitched frames
// of `rows` x `row_bytes`, each pointer at (row 0, data column 0).  dst == blur
// with equal pitch and stride is in place (a lane reads its bytes before it
// writes them); any other overlap of dst with orig or blur is refused.
//   depth: 8 | 16 (row_bytes a whole number of samples).  k: amount x 16, in
// [1, 255].  threshold: in [0, max].
//   images / orig_stride / blur_stride / dst_stride: the frames (ImageTables
// above) at those strides (each >= a frame), all in one launch.  With
// images.dims the geometry above is the envelope.  An active table is refused
// by name: every frame is sharpened.
// Every base, pitch and stride must be a multiple of 16 and every pitch
// >= round_up(row_bytes, 16).
// Every guard is named "launch_unsharp: ..."; a refused launch writes nothing.
struct UnsharpLaunch {
  const uint8_t* orig = nullptr;
  int64_t orig_pitch = 0;
  const uint8_t* blur = nullptr;
  int64_t blur_pitch = 0;
  uint8_t* dst = nullptr;
  int64_t dst_pitch = 0;
  int64_t row_bytes = 0;
  int64_t rows = 0;
  int depth = 8;
  int k = 16;
  int threshold = 0;
  ImageTables images;
  int64_t orig_stride = 0;
  int64_t blur_stride = 0;
  int64_t dst_stride = 0;
};
void launch_unsharp(const UnsharpLaunch& a, hipStream_t stream);
// Rows one workgroup of k_unsharp covers (tests place heights around it).
constexpr int kUnsharpBlockRows = 16;

// Whether `v` (or Auto) can fuse `steps` > 1 for this filter.
bool supports_fusion(const Filter& f, KernelVariant v);

// Default repetitions per launch for a band frame of `frame_bytes`: 1 without
// fusion; 12 for grey frames of 256 MiB and more (far beyond the Infinity
// Cache: 32768^2 grey 113.2-116.2 us/rep at 12 vs 116.9-121.1 at 8 over four
// boxes, 16384^2 30.6 vs 32.2; profiles/r02/tile_shapes.md,
// prefetch_kernel.md); 8 everywhere else (RGB's 3x wider horizontal halo makes
// deeper fusion slower; 1920x2520 RGB 3.5 us/rep at 8 vs 4.0 at 6, 8192^2 RGB
// within 2 % either way).  Other filters (float temporal kernel): 4.
// Depth 16 (the 16-bit gaussian kernel): 8 (docs/PERFORMANCE.md 3.7).
int auto_fuse(const Filter& f, KernelVariant v, int64_t frame_bytes, int channels = 0, int depth = 8);

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
// (ImageSet::dims) that have output in their image, 0 for a uniform launch.
std::vector<std::pair<std::vector<int64_t>, SwarShape>> swar_tuned();
// Tuned float entries: ({channels, uniform, steps, rows, row_bytes, batch, live}, shape); uniform 1: nine equal taps.
std::vector<std::pair<std::vector<int64_t>, FloatShape>> float_tuned();
// What ran (read-only, process-wide; tests assert that a forced kernel, shape
// and form are what a launch took after tuned_choice's fallbacks): the most
// recent launch issued to k_swar (kern 0) or k_swar_pf (kern 1), the tuner's
// timed candidates included, and the most recent one issued to
// k_float_temporal.  Before the first such launch: kern -1 / shape {0, 0}.
struct SwarLaunchInfo {
  int kern = -1;
  SwarShape shape{0, 0, 0};
  int form = -1;
};
SwarLaunchInfo last_swar_launch();
FloatShape last_float_launch();

// The 16-bit gaussian kernel's family (kernels/stencil_swar16.hip): lw is the
// SAMPLES per lane (4 or 8: 8- or 16-byte lane loads), one column strip per
// lane.  Its shapes (largest tile first), the override (lw = 0: back to the
// pick / tuner; an unknown shape is an error) and its tuned entries:
// ({channels, steps, rows, row_bytes, step_form, batch, live}, shape).
// clear_swar_tuning() forgets them too; swar_tuned() never lists them.
std::vector<SwarShape> swar16_shapes();
void set_swar16_shape(int lw, int m, int nw);
std::vector<std::pair<std::vector<int64_t>, SwarShape>> swar16_tuned();

}  // namespace pconv
