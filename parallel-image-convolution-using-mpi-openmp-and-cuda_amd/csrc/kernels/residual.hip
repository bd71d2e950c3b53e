// Residual kernel (gfx950): how many bytes of a frame one more repetition
// would change.  See launch_residual in include/pconv/kernels.hpp.
//
// The reference has no convergence check (its MPI family usually ends the
// loop on an MPI_Allreduce of a per-rank change count); here the count comes
// from ONE read of the current frame: a lane owns 16 consecutive row bytes
// (one dwordx4 load plus the dwords on either side for the +/-CH taps),
// marches down kRpt rows keeping the three-row window in registers, evaluates
// step(x) per byte in the project's arithmetic — (sum tap*p) >> shift for
// int-exact filters, float32 multiply-then-add in row-major tap order
// otherwise (nine_tap.hpp, shared with k_generic9) — and counts the bytes that
// differ from x.  No pixel is stored.  Counts are summed in the wave, then across the
// workgroup's four waves through LDS, and one 64-bit atomic add per workgroup
// (none when its count is zero) lands on the device counter.
//
// An image batch (StencilLaunch::images) is a run-time argument, as in the
// temporal kernels: the grid is flat and image-major (image_block in
// image_grid.hpp).  A workgroup's image does two things only: it moves the
// frame pointer by img * batch_stride and it picks the counter the workgroup's
// atomic add lands on, counter[img].  One image is the same instantiations on
// the same grid, adding to counter[0].
//
// Borders are applied to the registers, not read from the frame: rows outside
// the global image are zeros (Zero) or the image's first / last row
// (Replicate); the bytes left of column 0 and right of the row's last byte
// are zeros or byte c of the first / last pixel.  The kernel therefore
// depends neither on ghost rows beyond the image edge nor on the pad columns.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "pconv/device.hpp"
#include "pconv/kernels.hpp"
#include "image_grid.hpp"
#include "image_set.hpp"
#include "nine_tap.hpp"
#include "tuning.hpp"

namespace pconv {
namespace {

constexpr int kRpt = kResidualBlockRows / 4;  // rows per lane; 4 waves stacked vertically per workgroup

// Mask of the bytes of window dword i (positions 4i-4 .. 4i-1) that lie below position n.
__device__ __forceinline__ u32 below(int i, int n) { return low_bytes(n, 4 * i - 4); }

// One frame row with the border rule applied.  `r` is the frame row, [lo, hi)
// the frame rows inside the global image, x the lane's first byte, valid =
// row_bytes - x (>= 1).
template <int CH, bool REP>
__device__ __forceinline__ Row24 load_row(const uint8_t* __restrict__ src, int64_t pitch, int x, int valid, int r,
                                          int lo, int hi) {
  Row24 o;
  if (REP) {
    r = min(max(r, lo), hi - 1);
  } else if (r < lo || r >= hi) {
#pragma unroll
    for (int i = 0; i < 6; ++i) o.w[i] = 0;
    return o;
  }
  const uint8_t* p = src + static_cast<int64_t>(r) * pitch + x;
  const uint4 v = *reinterpret_cast<const uint4*>(p);
  o.w[0] = *reinterpret_cast<const u32*>(p - 4);
  o.w[1] = v.x;
  o.w[2] = v.y;
  o.w[3] = v.z;
  o.w[4] = v.w;
  o.w[5] = *reinterpret_cast<const u32*>(p + 16);
  if (valid < 20) {
    // The row ends inside this window: positions >= valid become zero, or the
    // byte CH positions to their left (the same channel of the last pixel —
    // the whole window shifted by CH bytes, taken where the row has ended).
    u32 s[6];
#pragma unroll
    for (int i = 0; i < 6; ++i)
      s[i] = REP ? __builtin_amdgcn_alignbyte(o.w[i], i > 0 ? o.w[i - 1] : 0u, 4 - CH) : 0u;
#pragma unroll
    for (int i = 1; i < 6; ++i) {
      const u32 m = below(i, valid);
      o.w[i] = (o.w[i] & m) | (s[i] & ~m);
    }
  }
  // Left of column 0: zero, or the first pixel's bytes moved CH positions down.
  if (x == 0) o.w[0] = REP ? o.w[1] << (8 * (4 - CH)) : 0u;
  return o;
}

// Bytes j < valid of the middle row that one repetition changes.
template <int CH, bool FLOAT>
__device__ __forceinline__ u32 changed(const Row24& a, const Row24& b, const Row24& c, const Taps9& tp, int valid) {
  u32 n = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    u32 v;
    PCONV_NINE_TAP(v, a.w, b.w, c.w, tp, j)
    n += (j < valid && v != byte_at(b.w, j)) ? 1u : 0u;
  }
  return n;
}

// Workgroup = 64 lanes along the row x 4 waves down the rows; workgroups in a
// flat grid, the row's chunks fastest, then the image's block rows, then the
// images of the batch.
template <int CH, bool FLOAT, bool REP>
__global__ __launch_bounds__(256) void k_residual(const uint8_t* __restrict__ src, int64_t pitch, int row_bytes,
                                                  int r0, int r1, Taps9 tp, int img_lo, int img_hi, int blocks_x,
                                                  int blocks_per_image, int64_t batch_stride,
                                                  unsigned long long* __restrict__ counter,
                                                  const ImageDims* __restrict__ dims,
                                                  const int32_t* __restrict__ active, unsigned last_frame) {
  __shared__ u32 part[4];
  // The image only moves the frame pointer and picks the counter.  Active
  // images: the grid's slot names its frame through the table (one scalar
  // load; the unsigned min keeps a wrong table inside the batch_frames frames
  // and counters); from there on img is a frame index.
  const ImageBlock wg = image_block(blocks_x, blocks_per_image);
  const int bx = wg.bx, by = wg.by;
  unsigned img = wg.img;
  if (active != nullptr) img = min(static_cast<unsigned>(active[img]), last_frame);
  src += static_cast<int64_t>(img) * batch_stride;
  // Mixed sizes: the image's own extent replaces the envelope's (one scalar
  // load; img is workgroup-uniform; whole images, so r0 = img_lo = 0 and
  // img_hi = r1).  A workgroup of the envelope's grid with no byte of this
  // image adds nothing: gone before its first load and the barrier, no atomic.
  if (dims != nullptr) {
    const ImageDims d = clamp_extent(dims[img], row_bytes, r1);
    row_bytes = d.row_bytes;
    img_hi = min(d.height, img_hi);
    r1 = d.height;
    if (bx * 1024 >= row_bytes || r0 + by * 4 * kRpt >= r1) return;
  }
  const int x = (bx * 64 + static_cast<int>(threadIdx.x)) * 16;
  const int rs = r0 + (by * 4 + static_cast<int>(threadIdx.y)) * kRpt;
  u32 cnt = 0;
  if (x < row_bytes && rs < r1) {
    const int n = min(kRpt, r1 - rs);
    const int valid = row_bytes - x;
    Row24 a = load_row<CH, REP>(src, pitch, x, valid, rs - 1, img_lo, img_hi);
    Row24 b = load_row<CH, REP>(src, pitch, x, valid, rs, img_lo, img_hi);
#pragma unroll
    for (int i = 0; i < kRpt; ++i) {
      if (i >= n) break;
      const Row24 c = load_row<CH, REP>(src, pitch, x, valid, rs + i + 1, img_lo, img_hi);
      cnt += changed<CH, FLOAT>(a, b, c, tp, valid);
      a = b;
      b = c;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
  if (threadIdx.x == 0) part[threadIdx.y] = cnt;
  __syncthreads();
  if (threadIdx.x == 0 && threadIdx.y == 0) {
    const u32 total = part[0] + part[1] + part[2] + part[3];
    if (total != 0) atomicAdd(counter + img, static_cast<unsigned long long>(total));
  }
}

// f(std::bool_constant<b>) for a run-time b.
template <class F>
void with_bool(bool b, F&& f) {
  b ? f(std::true_type{}) : f(std::false_type{});
}

template <int CH>
void launch_ch(const Filter& f, const StencilLaunch& a, uint64_t* counter, hipStream_t s) {
  const int64_t rows = a.r1 - a.r0;
  const auto [lo, hi] = image_rows_in_frame(a);
  const int64_t bx = ceil_div<int64_t>(ceil_div<int64_t>(a.row_bytes, 16), 64);
  const int64_t by = ceil_div<int64_t>(rows, kResidualBlockRows);
  const int images = a.images.images();
  check_flat_grid("launch_residual", bx, by, images);
  const Taps9 tp = make_taps9(f);
  const dim3 grid(static_cast<unsigned>(bx * by * images)), block(64, 4);
  auto* ctr = reinterpret_cast<unsigned long long*>(counter);
  const int rb = static_cast<int>(a.row_bytes), r0 = static_cast<int>(a.r0), r1 = static_cast<int>(a.r1);
  const int nbx = static_cast<int>(bx), per_image = static_cast<int>(bx * by), img_lo = lo, img_hi = hi;
  const BatchKernelArgs b = batch_kernel_args(a);
  with_bool(!int_form_allowed(f), [&](auto fl) {
    with_bool(a.border == Border::Replicate, [&](auto rep) {
      k_residual<CH, decltype(fl)::value, decltype(rep)::value>
          <<<grid, block, 0, s>>>(a.src, a.pitch, rb, r0, r1, tp, img_lo, img_hi, nbx, per_image, b.stride, ctr,
                                  b.dims, b.active, b.last_frame);
    });
  });
}

}  // namespace

void launch_residual(const Filter& f, Channels ch, const StencilLaunch& a_in, uint64_t* counter, hipStream_t stream) {
  StencilLaunch a = a_in;
  PCONV_CHECK(a.depth == 8, "launch_residual: depth 16 not supported (no residual kernel for 16-bit samples)");
  check_image_set("launch_residual", a, channel_count(ch));  // on the rows as given
  // rows outside the global image are no part of the map (launch_stencil's clip)
  a.r0 = std::max(a.r0, -a.g_row0);
  a.r1 = std::min(a.r1, a.height - a.g_row0);
  if (a.r1 <= a.r0) return;
  // Geometry guards: every access of the launch must stay inside the frame.
  PCONV_CHECK(a.row_bytes >= 1, "launch_residual: empty rows");
  check_frame_access("launch_residual", a, a.src && counter, 1);
  PCONV_CHECK(reinterpret_cast<uintptr_t>(a.src) % 16 == 0, "launch_residual: frame rows must be 16-byte aligned");
  PCONV_CHECK(a.row_bytes < (int64_t(1) << 31) - 2048 && a.r1 - a.frame_lo < (int64_t(1) << 31) - 64 &&
                  a.r1 < (int64_t(1) << 31) - 64 && a.r0 > -(int64_t(1) << 30),
              "launch_residual: geometry exceeds 32-bit kernel indices");
  PCONV_CHECK(a.row_bytes % channel_count(ch) == 0, "launch_residual: row bytes are no whole pixels");
  with_channels(ch, [&](auto chn) { launch_ch<decltype(chn)::value>(f, a, counter, stream); });
  PCONV_HIP_CHECK(hipGetLastError());
}

}  // namespace pconv
