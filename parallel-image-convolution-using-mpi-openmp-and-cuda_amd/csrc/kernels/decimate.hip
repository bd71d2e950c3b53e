// Decimation kernel (gfx950): every s-th pixel of every s-th row of a frame,
// packed into a pitched destination.  See launch_decimate in
// include/pconv/kernels.hpp.
//
// The reference has no subsampled output; a user of it downloads every blurred
// byte and slices on the host.  Here the slicing runs on the device, so that a
// host copy (or the next pyramid level) moves out_h x out_w pixels instead of
// H x W.
//
// ONLY SELECTED SOURCE ROWS ARE EVER ADDRESSED.  Output row Y reads source row
// first + Y * s and nothing else: the s - 1 rows in between cost no load, no
// address and no cache line.  That, not the arithmetic, is the point of the
// kernel: at factor s it touches 1 / s of the frame's rows (and, for pixels
// narrower than a cache line's 1 / s, still most lines of those rows).
//
// Lanes run along the OUTPUT row and own 4 consecutive output bytes.  Output
// byte j is byte j % PB of output pixel j / PB, which is source pixel
// (j / PB) * s: source byte (j / PB) * s * PB + j % PB.  PB (bytes per pixel)
// is a template argument, so both divisions are by constants; s is a run-time
// scalar.  The source is read in the widest unit a pixel allows — a dword for
// PB 4 and for each half of PB 8, a ushort for PB 2 and 6, bytes for PB 1 and
// 3 — and the lane's 4 bytes leave as ONE dword store where the destination
// allows it (ALIGNED, chosen on the host: base, pitch and frame stride are
// multiples of 4) and all 4 lie inside the row; the row's tail and every
// unaligned destination take byte stores.
//
// A workgroup is 64 lanes x 4 waves; each wave marches down kRowsPerWave
// output rows, so a workgroup covers 256 output bytes x kDecimateBlockRows
// rows.  The grid is flat and image-major (image_block in image_grid.hpp).
// With an extents table (SOURCE extents) the image's own output extent is
// derived here as the ceil of its own size, and a workgroup of the envelope's
// grid with no output in its image leaves before its first load.
//
// Nothing outside [0, out_row_bytes) of rows [0, out_h) of a destination frame
// is written and nothing outside [0, row_bytes) of the image's rows is read:
// pads, ghost rows and the rest of an envelope frame keep their bytes.
#include <hip/hip_runtime.h>

#include <string>

#include "pconv/device.hpp"
#include "pconv/kernels.hpp"
#include "image_grid.hpp"
#include "image_set.hpp"

namespace pconv {
namespace {

constexpr int kRowsPerWave = kDecimateBlockRows / 4;  // 4 waves stacked vertically per workgroup
constexpr int kBlockBytes = 64 * 4;                   // output bytes of a row one workgroup covers

// Bytes of the widest load that never straddles a pixel.
template <int PB>
struct LoadUnit {
  static constexpr int value = PB % 4 == 0 ? 4 : PB % 2 == 0 ? 2 : 1;
};

template <int U>
__device__ __forceinline__ uint32_t load_unit(const uint8_t* p) {
  if (U == 4) return *reinterpret_cast<const uint32_t*>(p);
  if (U == 2) return *reinterpret_cast<const uint16_t*>(p);
  return *p;
}

template <int PB, bool ALIGNED>
__global__ __launch_bounds__(256) void k_decimate(const uint8_t* __restrict__ src, int64_t src_pitch, int row_bytes,
                                                  int rows, int first, uint8_t* __restrict__ dst, int64_t dst_pitch,
                                                  int factor, int blocks_x, int blocks_per_image, int64_t src_stride,
                                                  int64_t dst_stride, const ImageDims* __restrict__ dims) {
  constexpr int U = LoadUnit<PB>::value;
  const auto [img, bx, by] = image_block(blocks_x, blocks_per_image);
  src += static_cast<int64_t>(img) * src_stride;
  dst += static_cast<int64_t>(img) * dst_stride;
  // Mixed sizes: the image's own extent replaces the envelope's (one scalar
  // load; whole images, so first = 0).
  if (dims != nullptr) {
    const ImageDims d = clamp_extent(dims[img], row_bytes, rows);
    row_bytes = d.row_bytes;
    rows = d.height;
  }
  // Output extent: the ceil of the image's own extent (in pixels, in rows).
  const int out_rb = ((row_bytes / PB + factor - 1) / factor) * PB;
  const int out_h = rows > first ? (rows - first + factor - 1) / factor : 0;
  if (bx * kBlockBytes >= out_rb || by * kDecimateBlockRows >= out_h) return;  // before the first load

  const int j0 = (bx * 64 + static_cast<int>(threadIdx.x)) * 4;
  if (j0 >= out_rb) return;
  // Source byte of each unit of the lane's 4 output bytes (the same for every row).
  int sb[4 / U];
#pragma unroll
  for (int u = 0; u < 4 / U; ++u) {
    const int j = j0 + u * U;
    sb[u] = (j / PB) * factor * PB + j % PB;
  }
  const int live = min(4, out_rb - j0);  // output bytes of this lane inside the row (whole units)
  const int y0 = (by * 4 + static_cast<int>(threadIdx.y)) * kRowsPerWave;
#pragma unroll
  for (int i = 0; i < kRowsPerWave; ++i) {
    const int y = y0 + i;
    if (y >= out_h) break;
    // the one source row this output row reads: 64-bit row offsets
    const uint8_t* s = src + (static_cast<int64_t>(first) + static_cast<int64_t>(y) * factor) * src_pitch;
    uint8_t* d = dst + static_cast<int64_t>(y) * dst_pitch + j0;
    uint32_t v = 0;
#pragma unroll
    for (int u = 0; u < 4 / U; ++u)
      if (u * U < live) v |= load_unit<U>(s + sb[u]) << (8 * u * U);
    if (ALIGNED && live == 4) {
      *reinterpret_cast<uint32_t*>(d) = v;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < live) d[k] = static_cast<uint8_t>(v >> (8 * k));
    }
  }
}

template <int PB>
void launch_pb(const DecimateLaunch& a, int first, int64_t bx, int64_t by, bool aligned, hipStream_t s) {
  const int frames = a.images.frames;
  const dim3 grid(static_cast<unsigned>(bx * by * frames)), block(64, 4);
  const int rb = static_cast<int>(a.row_bytes), rows = static_cast<int>(a.rows);
  const int64_t ss = frames > 1 ? a.src_stride : 0, ds = frames > 1 ? a.dst_stride : 0;
  if (aligned)
    k_decimate<PB, true><<<grid, block, 0, s>>>(a.src, a.src_pitch, rb, rows, first, a.dst, a.dst_pitch, a.factor,
                                                static_cast<int>(bx), static_cast<int>(bx * by), ss, ds,
                                                a.images.dims);
  else
    k_decimate<PB, false><<<grid, block, 0, s>>>(a.src, a.src_pitch, rb, rows, first, a.dst, a.dst_pitch, a.factor,
                                                 static_cast<int>(bx), static_cast<int>(bx * by), ss, ds,
                                                 a.images.dims);
}

}  // namespace

void launch_decimate(const DecimateLaunch& a, hipStream_t stream) {
  const std::string who = "launch_decimate";
  const auto num = [](int64_t v) { return std::to_string(v); };
  PCONV_CHECK(a.factor >= 1 && a.factor <= kMaxDecimate,
              who + ": factor " + num(a.factor) + " is outside [1, " + num(kMaxDecimate) + "]");
  const int pb = a.pixel_bytes;
  PCONV_CHECK(pb == 1 || pb == 2 || pb == 3 || pb == 4 || pb == 6 || pb == 8,
              who + ": pixel_bytes " + num(pb) + " is none of 1, 2, 3, 4, 6, 8");
  check_no_active(who, a.images, "decimated");
  PCONV_CHECK(a.src != nullptr && a.dst != nullptr, who + ": null frame pointer");
  const int frames = a.images.frames;
  PCONV_CHECK(frames >= 1, who + ": frames must be >= 1");
  PCONV_CHECK(a.rows >= 1 && a.row_bytes >= pb, who + ": empty source frame");
  PCONV_CHECK(a.row_bytes % pb == 0, who + ": row bytes " + num(a.row_bytes) + " are no whole pixels of " + num(pb) +
                                         " bytes");
  PCONV_CHECK(a.row_bytes <= a.src_pitch, who + ": row bytes " + num(a.row_bytes) + " exceed the source pitch " +
                                              num(a.src_pitch));
  PCONV_CHECK(a.g_row0 >= 0, who + ": g_row0 must be >= 0");
  PCONV_CHECK(a.row_bytes < (int64_t(1) << 31) - 1024 && a.rows < (int64_t(1) << 31) - 64,
              who + ": geometry exceeds 32-bit kernel indices");
  // The loads' width: a dword for PB 4 / 8, a ushort for PB 2 / 6.
  const int unit = pb % 4 == 0 ? 4 : pb % 2 == 0 ? 2 : 1;
  PCONV_CHECK(reinterpret_cast<uintptr_t>(a.src) % unit == 0 && a.src_pitch % unit == 0 &&
                  (frames <= 1 || a.src_stride % unit == 0),
              who + ": source base, pitch and stride must be multiples of " + num(unit) + " for " + num(pb) +
                  "-byte pixels");
  check_extents(who, a.images, a.row_bytes, a.rows, pb, "pixels", a.g_row0 == 0, "g_row0 = 0");
  // Frame row r is kept when (g_row0 + r) % factor == 0: the first such row,
  // and the envelope's output extent (every image's own lies inside it).
  const int64_t first = (a.factor - a.g_row0 % a.factor) % a.factor;
  const int64_t out_h = a.rows > first ? decimated_extent(a.rows - first, a.factor) : 0;
  const int64_t out_rb = decimated_extent(a.row_bytes / pb, a.factor) * pb;
  PCONV_CHECK(a.dst_pitch >= out_rb, who + ": destination pitch " + num(a.dst_pitch) +
                                         " is smaller than an output row (" + num(out_rb) + " bytes)");
  const int64_t frame_extent = out_h > 0 ? (out_h - 1) * a.dst_pitch + out_rb : 0;
  if (frames > 1) {
    check_frames_apart(who, "src_stride", a.src_stride, "a source frame", (a.rows - 1) * a.src_pitch + a.row_bytes);
    check_frames_apart(who, "dst_stride", a.dst_stride, "an output frame", frame_extent);
    PCONV_CHECK(frames * a.dst_stride <= a.dst_bytes,
                who + ": " + num(frames) + " frames at dst_stride " + num(a.dst_stride) + " exceed dst_bytes " +
                    num(a.dst_bytes));
  }
  PCONV_CHECK((frames - 1) * (frames > 1 ? a.dst_stride : 0) + frame_extent <= a.dst_bytes,
              who + ": the output (" + num(out_h) + " rows of " + num(out_rb) + " bytes at pitch " +
                  num(a.dst_pitch) + ") exceeds dst_bytes " + num(a.dst_bytes));
  if (out_h == 0) return;  // a band without a selected row
  const int64_t bx = ceil_div<int64_t>(out_rb, kBlockBytes), by = ceil_div<int64_t>(out_h, kDecimateBlockRows);
  check_flat_grid(who, bx, by, frames);
  const bool aligned = reinterpret_cast<uintptr_t>(a.dst) % 4 == 0 && a.dst_pitch % 4 == 0 &&
                       (frames <= 1 || a.dst_stride % 4 == 0);
  const int f = static_cast<int>(first);
  switch (pb) {
    case 1: launch_pb<1>(a, f, bx, by, aligned, stream); break;
    case 2: launch_pb<2>(a, f, bx, by, aligned, stream); break;
    case 3: launch_pb<3>(a, f, bx, by, aligned, stream); break;
    case 4: launch_pb<4>(a, f, bx, by, aligned, stream); break;
    case 6: launch_pb<6>(a, f, bx, by, aligned, stream); break;
    default: launch_pb<8>(a, f, bx, by, aligned, stream); break;
  }
  PCONV_HIP_CHECK(hipGetLastError());
}

}  // namespace pconv
