// Unsharp mask kernel (gfx950): out = x + amount * (x - blur(x)), per sample,
// in exact integers.  See launch_unsharp in include/pconv/kernels.hpp.
//
// The reference only ever blurs; a user of it who wants the sharpened image
// downloads the blurred frame and combines it with the original in three host
// passes.  Here the original stays on the device and the combination is one
// pointwise pass over the frame.
//
//   d = x - b
//   out = x                                            if |d| < t
//   out = clamp((x (16 + k) - b k + 8) >> 4, 0, max)   otherwise
//
// with k = amount x 16 in [1, 255], t in [0, max], max = 255 (depth 8) or 65535
// (depth 16, samples in host byte order).  The shift is arithmetic (floor), so
// a negative numerator gives <= -1 and clamps to 0; |numerator| < 2^25, plain
// 32-bit integers.  Every sample alike, an RGBA image's fourth channel included.
//
// The kernel is element-wise and memory-bound: two reads and one write per
// byte.  A lane owns 16 consecutive row bytes: ONE 16-byte load of the
// original, one of the blurred frame, one 16-byte store.  A workgroup is 64
// lanes x 4 waves and covers 1024 row bytes x kUnsharpBlockRows rows; each
// wave marches down kRowsPerWave rows, all of whose loads are issued before the
// first store.  The grid is flat and image-major (image_block in
// image_grid.hpp); with an extents table a workgroup with no byte of its image
// leaves before its first load.
//
// The lane that holds the row's end loads its 16 bytes like every other (the
// guards keep round_up(row_bytes, 16) inside every pitch) and stores only the
// bytes below row_bytes, one by one.  Nothing outside [0, row_bytes) of rows
// [0, rows) of a destination frame is ever written: pads, ghost rows and the
// rest of an envelope frame keep their bytes — the zero border of the fused
// kernels depends on it.
//
// dst may be blur (in place): a lane reads exactly the bytes it writes, and
// reads them first.
#include <hip/hip_runtime.h>

#include <string>

#include "pconv/device.hpp"
#include "pconv/kernels.hpp"
#include "image_grid.hpp"
#include "image_set.hpp"

namespace pconv {
namespace {

constexpr int kRowsPerWave = kUnsharpBlockRows / 4;  // 4 waves stacked vertically per workgroup
constexpr int kLaneBytes = 16;                       // row bytes one lane owns
constexpr int kBlockBytes = 64 * kLaneBytes;         // row bytes one workgroup covers

__device__ __forceinline__ int sharpen(int x, int b, int k, int t, int mx) {
  const int d = x - b;
  const int r = min(max((x * (16 + k) - b * k + 8) >> 4, 0), mx);
  return abs(d) < t ? x : r;
}

// One dword of samples: four of 8 bits or two of 16.
template <int DEPTH>
__device__ __forceinline__ uint32_t sharpen_word(uint32_t x, uint32_t b, int k, int t) {
  constexpr int mx = (1 << DEPTH) - 1;
  uint32_t out = 0;
#pragma unroll
  for (int s = 0; s < 32; s += DEPTH)
    out |= static_cast<uint32_t>(sharpen(static_cast<int>((x >> s) & mx), static_cast<int>((b >> s) & mx), k, t, mx))
           << s;
  return out;
}

template <int DEPTH>
__global__ __launch_bounds__(256) void k_unsharp(const uint8_t* __restrict__ orig, int64_t orig_pitch,
                                                 const uint8_t* blur, int64_t blur_pitch, uint8_t* dst,
                                                 int64_t dst_pitch, int row_bytes, int rows, int k, int t,
                                                 int blocks_x, int blocks_per_image, int64_t orig_stride,
                                                 int64_t blur_stride, int64_t dst_stride,
                                                 const ImageDims* __restrict__ dims) {
  const auto [img, bx, by] = image_block(blocks_x, blocks_per_image);
  orig += static_cast<int64_t>(img) * orig_stride;
  blur += static_cast<int64_t>(img) * blur_stride;
  dst += static_cast<int64_t>(img) * dst_stride;
  // Mixed sizes: the image's own extent replaces the envelope's (one scalar load).
  if (dims != nullptr) {
    const ImageDims d = clamp_extent(dims[img], row_bytes, rows);
    row_bytes = d.row_bytes;
    rows = d.height;
  }
  if (bx * kBlockBytes >= row_bytes || by * kUnsharpBlockRows >= rows) return;  // before the first load

  const int x0 = (bx * 64 + static_cast<int>(threadIdx.x)) * kLaneBytes;
  if (x0 >= row_bytes) return;
  const int live = min(kLaneBytes, row_bytes - x0);  // bytes of this lane inside the row (whole samples)
  const int y0 = (by * 4 + static_cast<int>(threadIdx.y)) * kRowsPerWave;
  // Every load of the wave's rows first (also what makes in place safe: a lane
  // has read its bytes before it writes them), then the arithmetic and stores.
  uint4 xo[kRowsPerWave], xb[kRowsPerWave];
#pragma unroll
  for (int i = 0; i < kRowsPerWave; ++i) {
    const int64_t y = y0 + i;
    if (y < rows) {
      xo[i] = *reinterpret_cast<const uint4*>(orig + y * orig_pitch + x0);
      xb[i] = *reinterpret_cast<const uint4*>(blur + y * blur_pitch + x0);
    }
  }
#pragma unroll
  for (int i = 0; i < kRowsPerWave; ++i) {
    const int64_t y = y0 + i;
    if (y >= rows) break;
    uint4 v;
    v.x = sharpen_word<DEPTH>(xo[i].x, xb[i].x, k, t);
    v.y = sharpen_word<DEPTH>(xo[i].y, xb[i].y, k, t);
    v.z = sharpen_word<DEPTH>(xo[i].z, xb[i].z, k, t);
    v.w = sharpen_word<DEPTH>(xo[i].w, xb[i].w, k, t);
    uint8_t* d = dst + y * dst_pitch + x0;
    if (live == kLaneBytes) {
      *reinterpret_cast<uint4*>(d) = v;
    } else {
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < kLaneBytes; ++j)
        if (j < live) d[j] = static_cast<uint8_t>(w[j / 4] >> (8 * (j % 4)));
    }
  }
}

}  // namespace

void launch_unsharp(const UnsharpLaunch& a, hipStream_t stream) {
  const std::string who = "launch_unsharp";
  const auto num = [](int64_t v) { return std::to_string(v); };
  const auto addr = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
  PCONV_CHECK(a.depth == 8 || a.depth == 16, who + ": depth " + num(a.depth) + " is neither 8 nor 16");
  const int sb = a.depth / 8, mx = (1 << a.depth) - 1;
  PCONV_CHECK(a.k >= 1 && a.k <= 255, who + ": k " + num(a.k) + " is outside [1, 255] (amount x 16)");
  PCONV_CHECK(a.threshold >= 0 && a.threshold <= mx,
              who + ": threshold " + num(a.threshold) + " is outside [0, " + num(mx) + "]");
  check_no_active(who, a.images, "sharpened");
  PCONV_CHECK(a.orig != nullptr && a.blur != nullptr && a.dst != nullptr, who + ": null frame pointer");
  const int frames = a.images.frames;
  PCONV_CHECK(frames >= 1, who + ": frames must be >= 1");
  PCONV_CHECK(a.rows >= 1 && a.row_bytes >= sb, who + ": empty frame");
  PCONV_CHECK(a.row_bytes % sb == 0,
              who + ": row bytes " + num(a.row_bytes) + " are no whole samples of " + num(sb) + " bytes");
  PCONV_CHECK(a.row_bytes < (int64_t(1) << 31) - kBlockBytes && a.rows < (int64_t(1) << 31) - 64,
              who + ": geometry exceeds 32-bit kernel indices");
  const bool many = frames > 1;
  PCONV_CHECK(addr(a.orig) % 16 == 0 && addr(a.blur) % 16 == 0 && addr(a.dst) % 16 == 0 && a.orig_pitch % 16 == 0 &&
                  a.blur_pitch % 16 == 0 && a.dst_pitch % 16 == 0 &&
                  (!many || (a.orig_stride % 16 == 0 && a.blur_stride % 16 == 0 && a.dst_stride % 16 == 0)),
              who + ": every base, pitch and stride must be a multiple of 16 (the lanes' 16-byte accesses)");
  // The row's last lane loads (never stores) up to round_up(row_bytes, 16).
  const int64_t reach = round_up<int64_t>(a.row_bytes, 16);
  PCONV_CHECK(a.orig_pitch >= reach && a.blur_pitch >= reach && a.dst_pitch >= reach,
              who + ": a pitch is smaller than the row bytes rounded up to 16 (" + num(reach) + ")");
  const auto frame_bytes = [&](int64_t pitch) { return (a.rows - 1) * pitch + reach; };
  if (many) {
    check_frames_apart(who, "orig_stride", a.orig_stride, "a frame", frame_bytes(a.orig_pitch));
    check_frames_apart(who, "blur_stride", a.blur_stride, "a frame", frame_bytes(a.blur_pitch));
    check_frames_apart(who, "dst_stride", a.dst_stride, "a frame", frame_bytes(a.dst_pitch));
  }
  check_extents(who, a.images, a.row_bytes, a.rows, sb, "samples");
  const int64_t bx = ceil_div<int64_t>(a.row_bytes, kBlockBytes), by = ceil_div<int64_t>(a.rows, kUnsharpBlockRows);
  check_flat_grid(who, bx, by, frames);
  // dst == blur at the same pitch and stride is in place; any other overlap of
  // the destination with a source is refused (byte ranges of all frames).
  const auto span = [&](int64_t pitch, int64_t stride) {
    return static_cast<uintptr_t>((many ? (frames - 1) * stride : 0) + frame_bytes(pitch));
  };
  const auto overlap = [&](const uint8_t* p, uintptr_t pn, const uint8_t* q, uintptr_t qn) {
    return addr(p) < addr(q) + qn && addr(q) < addr(p) + pn;
  };
  const uintptr_t dn = span(a.dst_pitch, a.dst_stride);
  const bool in_place = a.dst == a.blur && a.dst_pitch == a.blur_pitch && (!many || a.dst_stride == a.blur_stride);
  PCONV_CHECK(in_place || !overlap(a.dst, dn, a.blur, span(a.blur_pitch, a.blur_stride)),
              who + ": dst overlaps blur (in place needs dst == blur with equal pitch and stride)");
  PCONV_CHECK(!overlap(a.dst, dn, a.orig, span(a.orig_pitch, a.orig_stride)), who + ": dst overlaps orig");
  const dim3 grid(static_cast<unsigned>(bx * by * frames)), block(64, 4);
  const int rb = static_cast<int>(a.row_bytes), rows = static_cast<int>(a.rows);
  const int64_t os = many ? a.orig_stride : 0, bs = many ? a.blur_stride : 0, ds = many ? a.dst_stride : 0;
  if (a.depth == 8)
    k_unsharp<8><<<grid, block, 0, stream>>>(a.orig, a.orig_pitch, a.blur, a.blur_pitch, a.dst, a.dst_pitch, rb, rows,
                                             a.k, a.threshold, static_cast<int>(bx), static_cast<int>(bx * by), os, bs,
                                             ds, a.images.dims);
  else
    k_unsharp<16><<<grid, block, 0, stream>>>(a.orig, a.orig_pitch, a.blur, a.blur_pitch, a.dst, a.dst_pitch, rb, rows,
                                              a.k, a.threshold, static_cast<int>(bx), static_cast<int>(bx * by), os, bs,
                                              ds, a.images.dims);
  PCONV_HIP_CHECK(hipGetLastError());
}

}  // namespace pconv
