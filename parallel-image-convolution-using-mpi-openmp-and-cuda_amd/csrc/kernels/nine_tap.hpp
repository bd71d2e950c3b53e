// The nine-tap core of the single-step kernels (stencil.hip) and the residual
// kernel (residual.hip): a lane's 24-byte row window, one output byte from
// three such windows in the project's two arithmetic forms, and the host-side
// rules the two launchers share (which form a filter may take, which frame
// rows lie inside the image, the frame-access guards).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <utility>

#include "pconv/kernels.hpp"

namespace pconv {
namespace {

using u32 = uint32_t;

struct Taps9 {
  int t[9];
  float w[9];
  int shift;
};

inline Taps9 make_taps9(const Filter& f) {
  Taps9 tp;
  for (int i = 0; i < 9; ++i) {
    tp.t[i] = f.taps[i];
    tp.w[i] = f.weights[i];
  }
  tp.shift = f.shift;
  return tp;
}

// Row window of one lane: bytes [-4, 20) relative to its first owned byte
// (w[0] the dword on the left, w[1..4] the 16 owned bytes, w[5] on the right).
struct Row24 {
  u32 w[6];
};

__device__ __forceinline__ u32 byte_at(const u32 (&w)[6], int b) {  // b in [-4, 20)
  return (w[(b + 4) >> 2] >> (8 * ((b + 4) & 3))) & 0xffu;
}

// Mask of the bytes of a dword holding positions first .. first + 3 that lie below position n.
__device__ __forceinline__ u32 low_bytes(int n, int first) {
  const int keep = min(max(n - first, 0), 4);
  return keep >= 4 ? 0xffffffffu : ((1u << (8 * keep)) - 1u);
}

// v = output byte j (0..15) of the middle row from the row windows above (wa),
// at (wb) and below (wc) it, where CH and FLOAT are in scope: (sum tap*p) >>
// shift saturated at 255, or float32 multiply-then-add in row-major tap order
// (the reference's, one rounding each, no FMA) with a truncating, saturating
// store.  A statement, not a function: behind a call boundary the compiler
// pairs the sixteen bytes' operations differently and both kernels' code
// changes (k_generic9 float grey: 496 instructions against 569).
#define PCONV_NINE_TAP(v, wa, wb, wc, tp, j)                                                                          \
  if constexpr (FLOAT) {                                                                                              \
    _Pragma("clang fp contract(off)") float acc = 0.0f;                                                               \
    _Pragma("unroll") for (int l = 0; l < 3; ++l) acc =                                                               \
        __fadd_rn(acc, __fmul_rn(static_cast<float>(byte_at(wa, (j) + (l - 1) * CH)), (tp).w[l]));                    \
    _Pragma("unroll") for (int l = 0; l < 3; ++l) acc =                                                               \
        __fadd_rn(acc, __fmul_rn(static_cast<float>(byte_at(wb, (j) + (l - 1) * CH)), (tp).w[3 + l]));                \
    _Pragma("unroll") for (int l = 0; l < 3; ++l) acc =                                                               \
        __fadd_rn(acc, __fmul_rn(static_cast<float>(byte_at(wc, (j) + (l - 1) * CH)), (tp).w[6 + l]));                \
    v = acc > 0.0f ? (acc >= 255.0f ? 255u : static_cast<u32>(acc)) : 0u;                                             \
  } else {                                                                                                            \
    int acc = 0;                                                                                                      \
    _Pragma("unroll") for (int l = 0; l < 3; ++l) acc += (tp).t[l] * int(byte_at(wa, (j) + (l - 1) * CH));            \
    _Pragma("unroll") for (int l = 0; l < 3; ++l) acc += (tp).t[3 + l] * int(byte_at(wb, (j) + (l - 1) * CH));        \
    _Pragma("unroll") for (int l = 0; l < 3; ++l) acc += (tp).t[6 + l] * int(byte_at(wc, (j) + (l - 1) * CH));        \
    v = static_cast<u32>(min(acc >> (tp).shift, 255));                                                                \
  }

// An int-exact filter is bit-identical in either form by definition; the
// integer one needs its sums inside 32 bits.
inline bool int_form_allowed(const Filter& f) { return f.int_exact && f.abs_sum() * 255 < (1 << 30); }

// Frame rows [lo, hi) inside the global image, clamped to the frame (32-bit
// indices are the caller's check).
inline std::pair<int, int> image_rows_in_frame(const StencilLaunch& a) {
  return {static_cast<int>(std::max<int64_t>(-a.g_row0, a.frame_lo)),
          static_cast<int>(std::min<int64_t>(a.height - a.g_row0, a.frame_hi))};
}

// Geometry guards of every launch: each access must stay inside the frame.
// `reach` = rows read above and below the output rows.
inline void check_frame_access(const std::string& who, const StencilLaunch& a, bool buffers_ok, int64_t reach) {
  PCONV_CHECK(buffers_ok, who + ": bad buffers");
  PCONV_CHECK(a.r0 - reach >= a.frame_lo && a.r1 + reach <= a.frame_hi,
              who + ": rows [" + std::to_string(a.r0) + "," + std::to_string(a.r1) + ") +/- " + std::to_string(reach) +
                  " exceed frame [" + std::to_string(a.frame_lo) + "," + std::to_string(a.frame_hi) + ")");
  PCONV_CHECK(a.pitch % 16 == 0 && a.pitch >= kPadLeft + round_up<int64_t>(a.row_bytes, 16) + 16,
              who + ": pitch too small for 16-byte vector access");
}

}  // namespace
}  // namespace pconv
