// Temporal-blocked kernel for ANY 3x3 filter in the reference's float32
// semantics (box/9 and "edge_detection"/28 of mpi/mpi_convolution.c:90-100,
// custom filters): `steps` repetitions per launch, the tile resident in
// registers between steps — one HBM/Infinity-Cache round trip per launch
// instead of per repetition (k_generic9 in stencil.hip, one launch per rep).
//
// Numerics, per output byte and step, exactly the reference's
// (mpi/mpi_convolution.c:303-307):
//   acc = 0; for k in 0..2, l in 0..2: acc = fl(acc + fl(p[k][l] * w[k*3+l]))
//   out = trunc(acc) clamped to [0, 255]
// separate multiply and add (no contraction: the TU is built with
// -ffp-contract=off; products and sums are packed f32 ops, one rounding each),
// row-major tap order, truncation after EVERY step, zero outside the image at
// every step (Border::Zero) or the nearest image pixel (Border::Replicate: the
// out-of-image OPERAND is substituted, never a correction term added — float
// sums depend on their order).  UNIFORM filters (all nine weights equal, e.g. box) compute each
// input byte's product once per row instead of once per tap: fl(p * w) does
// not depend on the tap, so the chain of additions is unchanged.
//
// Tile: NW waves stacked vertically, wave w keeps M rows x 8 bytes per lane
// (a 512-byte strip per wave row) as packed bytes.  Horizontal neighbours at
// distance CH (<= 4) come from the adjacent lanes by DPP wave_shr / wave_shl;
// vertical neighbours across waves through LDS (double-buffered by step
// parity, one barrier per step).  The tile's halo (`steps` rows, ceil(steps *
// CH / 8) lanes per side) absorbs what enters from outside the tile.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "pconv/device.hpp"
#include "pconv/kernels.hpp"
#include "image_set.hpp"
#include "tuning.hpp"

namespace pconv {
namespace {

using u32 = uint32_t;

struct FloatTaps {
  float w[9];
};

__device__ __forceinline__ float ub(u32 x, int k) { return static_cast<float>((x >> (8 * k)) & 0xffu); }

// Pairs of floats (bytes j and j + 4 of a lane's 8): every operation on a pair
// is one packed f32 instruction (v_pk_mul_f32 / v_pk_add_f32), each half
// rounded exactly like its scalar twin.  The TU is built with
// -ffp-contract=off, so a product never fuses into the following add.
typedef float f2 __attribute__((ext_vector_type(2)));

// Replicate border, columns: what a lane of a strip that touches the image's
// left or right edge substitutes in its window e[0, 8 + 2 CH) (byte columns
// x - CH + t): in the lane holding column 0 the CH entries before it take the
// first pixel's bytes (e[t] = e[t + CH]); the CH entries from window index
// `nin` on — the first byte columns past the row — take the last pixel's
// (e[t] = e[t - CH]; they sit in the window of the lane holding the row's last
// byte and, when that pixel straddles two lanes, of the lane before it).
struct ColFix {
  bool left;  // this lane holds byte column 0
  int nin;    // window entries before the row's end: row_bytes - (x - CH)
};

// Row (8 bytes per lane) -> pairs E[j] = (byte j - CH, byte j + 4 - CH) for
// j in [0, 4 + 2 CH): bytes [-CH, 8 + CH) of the row (times w when UNIFORM:
// fl(p * w) of a substituted byte is the same product).
template <int CH, bool UNIFORM, bool REP = false>
__device__ __forceinline__ void expand(const u32 (&X)[2], float w, f2 (&E)[4 + 2 * CH], const ColFix* cf = nullptr) {
  const u32 l = __builtin_amdgcn_mov_dpp(X[1], 0x138, 0xf, 0xf, true);  // wave_shr:1 -> left lane's bytes 4..7
  const u32 r = __builtin_amdgcn_mov_dpp(X[0], 0x130, 0xf, 0xf, true);  // wave_shl:1 -> right lane's bytes 0..3
  float e[8 + 2 * CH];
#pragma unroll
  for (int j = 0; j < CH; ++j) e[j] = ub(l, 4 - CH + j);
#pragma unroll
  for (int j = 0; j < 8; ++j) e[CH + j] = ub(X[j >> 2], j & 3);
#pragma unroll
  for (int j = 0; j < CH; ++j) e[CH + 8 + j] = ub(r, j);
  if constexpr (REP) {
#pragma unroll
    for (int t = 0; t < CH; ++t) e[t] = cf->left ? e[t + CH] : e[t];
    // ascending t reads e[t - CH] before the right edge: never a substituted entry
#pragma unroll
    for (int t = CH; t < 8 + 2 * CH; ++t) e[t] = (t >= cf->nin && t < cf->nin + CH) ? e[t - CH] : e[t];
  }
#pragma unroll
  for (int j = 0; j < 4 + 2 * CH; ++j) E[j] = (f2){e[j], e[j + 4]};
  if constexpr (UNIFORM) {
    const f2 ww = (f2){w, w};
#pragma unroll
    for (int j = 0; j < 4 + 2 * CH; ++j) E[j] = E[j] * ww;
  }
}

// Output bytes j and j + 4 (j < 4) as floats holding trunc(acc): integers, so
// v_cvt_pk_u8_f32 packs them exactly whatever its rounding mode, saturating
// the ones outside [0, 255].  Reference order: row k (a: above, b: this row, c: below),
// then column l.
template <int CH, bool UNIFORM>
__device__ __forceinline__ f2 out_pair(const f2 (&a)[4 + 2 * CH], const f2 (&b)[4 + 2 * CH],
                                       const f2 (&c)[4 + 2 * CH], int j, const f2 (&w)[9]) {
  f2 acc;
  if constexpr (UNIFORM) {
    acc = a[j];  // 0 + fl(p*w) is exact
    acc = acc + a[j + CH];
    acc = acc + a[j + 2 * CH];
    acc = acc + b[j];
    acc = acc + b[j + CH];
    acc = acc + b[j + 2 * CH];
    acc = acc + c[j];
    acc = acc + c[j + CH];
    acc = acc + c[j + 2 * CH];
  } else {
    acc = a[j] * w[0];
    acc = acc + a[j + CH] * w[1];
    acc = acc + a[j + 2 * CH] * w[2];
    acc = acc + b[j] * w[3];
    acc = acc + b[j + CH] * w[4];
    acc = acc + b[j + 2 * CH] * w[5];
    acc = acc + c[j] * w[6];
    acc = acc + c[j + CH] * w[7];
    acc = acc + c[j + 2 * CH] * w[8];
  }
  // reference store: float -> uint8 truncation, clamped like the CPU oracle.
  // The clamp is the packer's: v_cvt_pk_u8_f32 saturates to [0, 255]
  // (measured: -1e9, -5, -0.5 -> 0; 256, 300, 1e9 -> 255;
  // tools/ubench/cvt_pk_u8.hip, profiles/r03/float/cvt_pk_u8.txt), and
  // cvt(trunc(x)) == trunc(clamp(x, 0, 255)) for every finite x, so no
  // v_med3_f32 (a VOP3, ~1.8 issue slots) per output.
  return (f2){__builtin_truncf(acc.x), __builtin_truncf(acc.y)};
}

// Replicate state of a lane / wave; the zero border carries nothing.
template <bool REP>
struct RepState {};
template <>
struct RepState<true> {
  ColFix cf;
  bool above_own, below_own;  // global row 0 / the last image row is this wave's first / last register row
};

// Replicate border, rows inside one wave (as edge_rows of the SWAR kernel):
// the register row just above global row 0 takes row 0's bytes, the one just
// below the last image row that row's.  After the load and after every step's
// re-zeroing, only in waves that hold out-of-image rows (zero on entry: the
// copy is an OR under a wave-uniform mask, no dynamic register indexing).
template <int M>
__device__ __forceinline__ void edge_rows_ft(u32 (&D)[M][2], int out_top, int out_bot) {
  out_top = __builtin_amdgcn_readfirstlane(out_top);  // wave-uniform by construction
  out_bot = __builtin_amdgcn_readfirstlane(out_bot);
  asm volatile("" : "+s"(out_top), "+s"(out_bot));  // masks recomputed per call, not kept live across the steps
#pragma unroll
  for (int i = 0; i + 1 < M; ++i) {
    const u32 take = i + 1 == out_top ? 0xffffffffu : 0u;
    D[i][0] |= D[i + 1][0] & take;
    D[i][1] |= D[i + 1][1] & take;
  }
#pragma unroll
  for (int i = M - 1; i >= 1; --i) {
    const u32 take = i == out_bot ? 0xffffffffu : 0u;
    D[i][0] |= D[i - 1][0] & take;
    D[i][1] |= D[i - 1][1] & take;
  }
}

// The `steps` repetitions of a wave's M register rows.  COLFIX (replicate
// border, strips that touch the image's left or right edge) substitutes the
// out-of-image columns of every expanded row; it is a template parameter, so
// that the other strips run the loop without a single select — as a run-time
// branch inside expand() it made the compiler spill (256 VGPRs + 214 spilled on
// k_float_temporal<3, true, 16, 8>).
template <int CH, bool UNIFORM, int M, int NW, bool REP, bool COLFIX>
__device__ __forceinline__ void ft_steps(u32 (&D)[M][2], uint2 (&lds)[2][NW][2][64], int steps, int w, int lane,
                                         float w0, const f2 (&wv)[9], bool edge_strip, u32 m0, u32 m1, int out_top,
                                         int out_bot, const RepState<REP>& rs) {
  for (int s = 0; s < steps; ++s) {
    const int par = s & 1;
    lds[par][w][0][lane] = make_uint2(D[0][0], D[0][1]);
    lds[par][w][1][lane] = make_uint2(D[M - 1][0], D[M - 1][1]);
    __syncthreads();
    u32 A[2], B[2];
    {
      int wa = w > 0 ? w - 1 : 0;
      int wb = w < NW - 1 ? w + 1 : w;
      int sa = 1, sb = 0;
      if constexpr (REP) {
        // the row above global row 0 is row 0 itself, the row below the last
        // image row is that row: this wave's own published boundary row
        if (rs.above_own) {
          wa = w;
          sa = 0;
        }
        if (rs.below_own) {
          wb = w;
          sb = 1;
        }
      }
      const uint2 a = lds[par][wa][sa][lane], b = lds[par][wb][sb][lane];
      A[0] = a.x;
      A[1] = a.y;
      B[0] = b.x;
      B[1] = b.y;
    }
    f2 ea[4 + 2 * CH], eb[4 + 2 * CH], ec[4 + 2 * CH];
    if constexpr (COLFIX) {
      expand<CH, UNIFORM, true>(A, w0, ea, &rs.cf);
      expand<CH, UNIFORM, true>(D[0], w0, eb, &rs.cf);
    } else {
      expand<CH, UNIFORM>(A, w0, ea);
      expand<CH, UNIFORM>(D[0], w0, eb);
    }
#pragma unroll
    for (int i = 0; i < M; ++i) {
      if constexpr (COLFIX) {
        if (i + 1 < M)
          expand<CH, UNIFORM, true>(D[i + 1], w0, ec, &rs.cf);
        else
          expand<CH, UNIFORM, true>(B, w0, ec, &rs.cf);
      } else {
        if (i + 1 < M)
          expand<CH, UNIFORM>(D[i + 1], w0, ec);
        else
          expand<CH, UNIFORM>(B, w0, ec);
      }
      u32 o0 = 0, o1 = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const f2 v = out_pair<CH, UNIFORM>(ea, eb, ec, j, wv);
        o0 = __builtin_amdgcn_cvt_pk_u8_f32(v.x, j, o0);
        o1 = __builtin_amdgcn_cvt_pk_u8_f32(v.y, j, o1);
      }
      D[i][0] = o0;
      D[i][1] = o1;
#pragma unroll
      for (int j = 0; j < 4 + 2 * CH; ++j) {
        ea[j] = eb[j];
        eb[j] = ec[j];
      }
    }
    if (edge_strip) {
#pragma unroll
      for (int i = 0; i < M; ++i) {
        D[i][0] &= m0;
        D[i][1] &= m1;
      }
    }
    if (out_top > 0 || out_bot < M) {
#pragma unroll
      for (int i = 0; i < M; ++i)
        if (i < out_top || i >= out_bot) {
          D[i][0] = 0;
          D[i][1] = 0;
        }
      if constexpr (REP) edge_rows_ft<M>(D, out_top, out_bot);
    }
  }

}

template <int CH, bool UNIFORM, int M, int NW, bool REP = false>
__global__ __launch_bounds__(64 * NW) void k_float_temporal(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                            int64_t pitch, int row_bytes, int r0, int r1, int steps,
                                                            int g_row0, int height, FloatTaps tp,
                                                            int64_t batch_stride, const ImageDims* __restrict__ dims,
                                                            const int32_t* __restrict__ active, unsigned last_frame) {
  __shared__ uint2 lds[2][NW][2][64];  // [parity][wave][top/bottom][lane]
  // Image of the batch: grid.z (scalar); it only moves the two base pointers.
  // Active images: grid.z is a slot and names its frame through the table (one
  // scalar load); the unsigned min keeps a wrong table inside the allocation's
  // batch_frames frames.  From here on img is a frame index.
  // The empty asm settles both sums here, in scalar registers: from this line
  // on the kernel holds what the single-image kernel held (two pointers), and
  // the compiler allocates the registers of everything below as it did then.
  unsigned img = blockIdx.z;
  if (active != nullptr) img = min(static_cast<unsigned>(active[img]), last_frame);
  src += static_cast<int64_t>(img) * batch_stride;
  dst += static_cast<int64_t>(img) * batch_stride;
  asm volatile("" : "+s"(src), "+s"(dst));
  // Mixed sizes: the image's own extent replaces the envelope's (one scalar
  // load; img is workgroup-uniform).  The min keeps a wrong table inside
  // the frame.  Everything below reads the two values as it reads the arguments.
  if (dims != nullptr) {
    const ImageDims d = dims[img];
    row_bytes = min(d.row_bytes, row_bytes);
    height = min(d.height, height);
    // A tile of the envelope's grid with no output in this image: gone before
    // its first load and before any barrier (workgroup-uniform: every wave of
    // the workgroup ends here).  The wave ends in an opaque asm, not a
    // `return`: with a second exit in its control flow the compiler gave the
    // uniform 16-row replicate instantiations one VGPR more, and
    // <1, true, 16, {4, 8}, true> went from 128 to 129 and lost a wave; so
    // written, all 60 instantiations keep their registers (PERFORMANCE.md 3.5).
    const int vl = 64 - 2 * ((steps * CH + 7) >> 3);
    if (static_cast<int>(blockIdx.x) * vl * 8 >= row_bytes ||
        r0 + static_cast<int>(blockIdx.y) * (NW * M - 2 * steps) + g_row0 >= height)
      asm volatile("s_endpgm" ::: "memory");
  }
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int hl = (steps * CH + 7) >> 3;  // halo lanes per side
  const int vlanes = 64 - 2 * hl;
  const int chunk = static_cast<int>(blockIdx.x) * vlanes - hl + lane;  // 8-byte column chunk of this lane
  const int x = chunk * 8;
  const int nchunks = (row_bytes + 7) >> 3;
  const bool col_in = chunk >= 0 && chunk < nchunks;
  const int vrows = NW * M - 2 * steps;
  const int tile_r0 = r0 + static_cast<int>(blockIdx.y) * vrows;
  const int row_base = tile_r0 - steps + w * M;
  const float w0 = tp.w[0];
  f2 wv[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) wv[k] = (f2){tp.w[k], tp.w[k]};

  // bytes of this lane inside the image row (0..8)
  const int valid = col_in ? min(row_bytes - x, 8) : 0;
  const u32 m0 = valid >= 4 ? 0xffffffffu : (valid <= 0 ? 0u : ((1u << (8 * valid)) - 1u));
  const u32 m1 = valid >= 8 ? 0xffffffffu : (valid <= 4 ? 0u : ((1u << (8 * (valid - 4))) - 1u));
  const bool edge_strip = blockIdx.x == 0 || static_cast<int>(blockIdx.x) * vlanes - hl + 64 >= nchunks;

  u32 D[M][2];
  const int lo_ok = max(r0 - steps, -g_row0), hi_ok = min(r1 + steps, height - g_row0);
#pragma unroll
  for (int i = 0; i < M; ++i) {
    const int fr = row_base + i;
    uint2 v = make_uint2(0, 0);
    if (col_in && fr >= lo_ok && fr < hi_ok) {
      // 8-byte aligned (pitch % 16 == 0, data column 0 is 16-byte aligned); the
      // partial last chunk reads into the zero pad columns of the frame row
      v = *reinterpret_cast<const uint2*>(src + static_cast<int64_t>(fr) * pitch + x);
    }
    D[i][0] = v.x & m0;
    D[i][1] = v.y & m1;
  }
  const int out_top = min(max(-g_row0 - row_base, 0), M);
  const int out_bot = min(max(height - g_row0 - row_base, 0), M);
  // replicate: column substitution state, and the register rows holding the
  // image's first / last row (wave-uniform; outside [0, M) when not in this wave)
  RepState<REP> rs;
  if constexpr (REP) {
    rs.cf = ColFix{x == 0, row_bytes - (x - CH)};
    rs.above_own = -g_row0 - row_base == 0;
    rs.below_own = height - 1 - g_row0 - row_base == M - 1;
    if (out_top > 0 || out_bot < M) edge_rows_ft<M>(D, out_top, out_bot);  // the loaded rows' out-of-image neighbours
  }

  if constexpr (REP) {
    if (edge_strip)
      ft_steps<CH, UNIFORM, M, NW, true, true>(D, lds, steps, w, lane, w0, wv, edge_strip, m0, m1, out_top, out_bot, rs);
    else
      ft_steps<CH, UNIFORM, M, NW, true, false>(D, lds, steps, w, lane, w0, wv, edge_strip, m0, m1, out_top, out_bot,
                                                rs);
  } else {
    // The zero border's loop, inline as it always was (routed through
    // ft_steps the compiler allocates its registers differently).
    for (int s = 0; s < steps; ++s) {
      const int par = s & 1;
      lds[par][w][0][lane] = make_uint2(D[0][0], D[0][1]);
      lds[par][w][1][lane] = make_uint2(D[M - 1][0], D[M - 1][1]);
      __syncthreads();
      u32 A[2], B[2];
      {
        const int wa = w > 0 ? w - 1 : 0;
        const int wb = w < NW - 1 ? w + 1 : w;
        const uint2 a = lds[par][wa][1][lane], b = lds[par][wb][0][lane];
        A[0] = a.x;
        A[1] = a.y;
        B[0] = b.x;
        B[1] = b.y;
      }
      f2 ea[4 + 2 * CH], eb[4 + 2 * CH], ec[4 + 2 * CH];
      expand<CH, UNIFORM>(A, w0, ea);
      expand<CH, UNIFORM>(D[0], w0, eb);
  #pragma unroll
      for (int i = 0; i < M; ++i) {
        if (i + 1 < M)
          expand<CH, UNIFORM>(D[i + 1], w0, ec);
        else
          expand<CH, UNIFORM>(B, w0, ec);
        u32 o0 = 0, o1 = 0;
  #pragma unroll
        for (int j = 0; j < 4; ++j) {
          const f2 v = out_pair<CH, UNIFORM>(ea, eb, ec, j, wv);
          o0 = __builtin_amdgcn_cvt_pk_u8_f32(v.x, j, o0);
          o1 = __builtin_amdgcn_cvt_pk_u8_f32(v.y, j, o1);
        }
        D[i][0] = o0;
        D[i][1] = o1;
  #pragma unroll
        for (int j = 0; j < 4 + 2 * CH; ++j) {
          ea[j] = eb[j];
          eb[j] = ec[j];
        }
      }
      if (edge_strip) {
  #pragma unroll
        for (int i = 0; i < M; ++i) {
          D[i][0] &= m0;
          D[i][1] &= m1;
        }
      }
      if (out_top > 0 || out_bot < M) {
  #pragma unroll
        for (int i = 0; i < M; ++i)
          if (i < out_top || i >= out_bot) {
            D[i][0] = 0;
            D[i][1] = 0;
          }
      }
    }
  }

  const bool lane_ok = col_in && lane >= hl && lane < 64 - hl;
  const int st_lo = max(tile_r0, r0), st_hi = min(min(tile_r0 + vrows, r1), height - g_row0);
#pragma unroll
  for (int i = 0; i < M; ++i) {
    const int fr = row_base + i;
    if (lane_ok && fr >= st_lo && fr < st_hi) {
      uint8_t* q = dst + static_cast<int64_t>(fr) * pitch + x;
      if (valid == 8) {
        *reinterpret_cast<uint2*>(q) = make_uint2(D[i][0], D[i][1]);
      } else {  // partial last chunk: never write past the row's last byte
        const u32 lo = D[i][0], hi = D[i][1];
        for (int b = 0; b < valid; ++b) q[b] = static_cast<uint8_t>((b < 4 ? lo : hi) >> (8 * (b & 3)));
      }
    }
  }
}

// Instantiated tile shapes (M rows per wave, NW waves), written in this table
// and nowhere else: float_shapes(), the launch dispatch (launch_ft_with:
// compiled for every row, so a row is an instantiation), the model's
// candidates and the tuner's all read it.  Largest tiles (least halo) first,
// and the order is behaviour: pick_ft_shape returns the first shape that fills
// the chip, and {16,4} and {8,8} tie on workgroup count.
constexpr FloatShape kFtShapes[] = {{16, 8}, {16, 4}, {8, 8}, {8, 4}, {4, 8}};
constexpr size_t kNumFtShapes = sizeof(kFtShapes) / sizeof(kFtShapes[0]);

// Row of the table that holds a shape; kNumFtShapes: not instantiated.
size_t ft_shape_index(int m, int nw) {
  size_t i = 0;
  while (i < kNumFtShapes && (kFtShapes[i].m != m || kFtShapes[i].nw != nw)) ++i;
  return i;
}

// Grid of one launch of a tile shape: the host's one copy of the quantities
// the kernel derives from (steps, CH, M, NW), for the launch, the model and
// the tuner's candidate test.
struct FtGeom {
  bool ok = false;  // the halo leaves valid output (vlanes, vrows > 0)
  int hl = 0;       // halo lanes per side
  int vlanes = 0;   // valid 8-byte output chunks per strip
  int vrows = 0;    // valid output rows per tile
  int64_t col_tiles = 0, row_tiles = 0;
  int64_t tiles = 0;  // workgroups: col_tiles x row_tiles x batch (grid.z)
};

FtGeom ft_geom(const FloatShape& sh, int ch, int steps, int64_t rows, int64_t row_bytes, int batch = 1) {
  FtGeom g;
  g.hl = (steps * ch + 7) / 8;
  g.vlanes = 64 - 2 * g.hl;
  g.vrows = sh.m * sh.nw - 2 * steps;
  g.ok = g.vlanes > 0 && g.vrows > 0;
  if (!g.ok) return g;
  g.col_tiles = ceil_div<int64_t>(ceil_div<int64_t>(row_bytes, 8), g.vlanes);
  g.row_tiles = ceil_div<int64_t>(rows, g.vrows);
  g.tiles = g.col_tiles * g.row_tiles * batch;
  return g;
}

// Tile shape when nothing is tuned (one-shot CLI, a capture before tuning):
// the largest tile (least halo) whose grid fills the chip — at least 3/4 of
// a workgroup per CU — and whose last round of workgroups is at least 3/4
// full.  Fits the sweep (gpurun_out/r03/g/float_sweep.jsonl): 1920x2520 RGB
// at 4 steps -> 16x8 (252 workgroups: 8.0 us/rep, best), at 8 steps -> 16x4
// (9.5, best 9.5); grey at 8 steps -> 16x4 (3.6, best 3.5); 8192^2 RGB ->
// 16x8 (best).  set_float_shape(M, NW) forces one.
std::atomic<int> g_ft_force_m{0}, g_ft_force_nw{0};

FloatShape pick_ft_shape(int steps, int ch, int64_t rows, int64_t row_bytes, int batch = 1) {
  if (const int fm = g_ft_force_m.load(std::memory_order_relaxed)) {
    const size_t i = ft_shape_index(fm, g_ft_force_nw.load(std::memory_order_relaxed));
    if (i < kNumFtShapes) return kFtShapes[i];
  }
  static int cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) !=
                                                 hipSuccess)
      n = 256;
    return std::max(1, n);
  }();
  FloatShape most = kFtShapes[kNumFtShapes - 1];  // the smallest tile
  int64_t most_wgs = -1;
  for (const auto& c : kFtShapes) {
    const FtGeom g = ft_geom(c, ch, steps, rows, row_bytes, batch);
    if (!g.ok) continue;
    const int64_t wgs = g.tiles;
    const int64_t rounds = ceil_div<int64_t>(wgs, cus);
    if (4 * wgs >= 3 * static_cast<int64_t>(cus) && 4 * wgs >= 3 * rounds * cus) return c;
    if (wgs > most_wgs) {
      most_wgs = wgs;
      most = c;
    }
  }
  return most;  // a small frame: the shape with the most workgroups
}

// The most recent launch issued below, for last_float_launch(): m << 8 | nw.
std::atomic<int> g_ft_last_launch{0};

template <int CH, bool UNIFORM, int M, int NW>
void launch_ft_shape(const StencilLaunch& a, const FloatTaps& tp, hipStream_t s) {
  const int images = a.images.images();
  const BatchKernelArgs b = batch_kernel_args(a);
  const FtGeom g = ft_geom(FloatShape{M, NW}, CH, a.steps, a.r1 - a.r0, a.row_bytes, images);
  PCONV_CHECK(g.ok, "float temporal kernel: steps too large for the tile");
  PCONV_CHECK(g.tiles < (int64_t(1) << 31), "float temporal kernel: too many tiles (batch x tiles per image)");
  const dim3 grid(static_cast<unsigned>(g.col_tiles), static_cast<unsigned>(g.row_tiles),
                  static_cast<unsigned>(images));
  const auto kern = a.border == Border::Replicate ? &k_float_temporal<CH, UNIFORM, M, NW, true>
                                                  : &k_float_temporal<CH, UNIFORM, M, NW, false>;
  kern<<<grid, dim3(64 * NW), 0, s>>>(
      a.src, a.dst, a.pitch, static_cast<int>(a.row_bytes), static_cast<int>(a.r0), static_cast<int>(a.r1), a.steps,
      static_cast<int>(a.g_row0), static_cast<int>(std::min<int64_t>(a.height, int64_t(1) << 30)), tp,
      b.stride, b.dims, b.active, b.last_frame);
  g_ft_last_launch.store(M << 8 | NW, std::memory_order_relaxed);
}

template <int CH, bool UNIFORM>
void launch_ft_with(const StencilLaunch& a, const FloatTaps& tp, hipStream_t s, FloatShape sh) {
  const bool known = with_index<kNumFtShapes>(ft_shape_index(sh.m, sh.nw), [&](auto i) {
    constexpr FloatShape S = kFtShapes[decltype(i)::value];
    launch_ft_shape<CH, UNIFORM, S.m, S.nw>(a, tp, s);
  });
  PCONV_CHECK(known, "float temporal kernel: unsupported tile shape");
}

// Empirical shape tuning, as for the SWAR kernel (stencil_swar.hip): on the
// first launch of a geometry every shape that runs it is timed on the REAL
// launch (fastest_candidate, tuning.hpp) and the fastest is cached per
// (channels, uniform, steps, rows, row bytes, batch, live workgroups of a
// mixed-size launch under the model's shape; 0: uniform).  The
// shape is a large lever on these small frames and not monotonic in the
// model (1920x2520 RGB box, 4 steps: 8.0 us/rep with 16x8 tiles, 9.2-10.4
// with the others; gpurun_out/r03/g/float_sweep.jsonl).  Never while the
// stream is being captured: the engine tunes a step's launches first.
struct FtKey {
  int ch;
  bool uniform;
  int steps;
  int64_t rows, row_bytes;
  int batch;
  int64_t live;
  bool operator<(const FtKey& o) const {
    return std::tie(ch, uniform, steps, rows, row_bytes, batch, live) <
           std::tie(o.ch, o.uniform, o.steps, o.rows, o.row_bytes, o.batch, o.live);
  }
};
std::mutex g_ft_mu;
std::map<FtKey, FloatShape> g_ft_tuned;

template <int CH, bool UNIFORM>
FloatShape tuned_ft_shape(const StencilLaunch& a, const FloatTaps& tp, hipStream_t s) {
  const int64_t rows = a.r1 - a.r0;
  const int images = a.images.images();
  const FloatShape model = pick_ft_shape(a.steps, CH, rows, a.row_bytes, images);
  if (g_ft_force_m.load(std::memory_order_relaxed) || !shape_tuning_enabled()) return model;
  // (the model saw the envelope: an early-exiting workgroup is charged as a full one)
  const FtGeom mg = ft_geom(model, CH, a.steps, rows, a.row_bytes, images);
  const FtKey key{CH, UNIFORM, a.steps, rows, a.row_bytes, images,
                  live_workgroups(a, int64_t(mg.vlanes) * 8, mg.vrows, 1)};
  {
    std::lock_guard<std::mutex> lk(g_ft_mu);
    auto it = g_ft_tuned.find(key);
    if (it != g_ft_tuned.end()) return it->second;
  }
  // (an active-image launch never tunes: its own cached entry above, else the model; stencil_swar.hip)
  if (stream_capturing(s) || a.images.has_table()) return model;
  std::vector<FloatShape> ok;
  for (const auto& c : kFtShapes)
    if (ft_geom(c, CH, a.steps, rows, a.row_bytes).ok) ok.push_back(c);
  PCONV_CHECK(!ok.empty(), "float temporal kernel: steps too large for every tile shape");
  const FloatShape best =
      ok[fastest_candidate(ok.size(), s, [&](size_t i) { launch_ft_with<CH, UNIFORM>(a, tp, s, ok[i]); })];
  std::lock_guard<std::mutex> lk(g_ft_mu);
  g_ft_tuned.emplace(key, best);
  return best;
}

template <int CH, bool UNIFORM>
void launch_ft(const StencilLaunch& a, const FloatTaps& tp, hipStream_t s, bool launch) {
  const FloatShape sh = tuned_ft_shape<CH, UNIFORM>(a, tp, s);
  if (launch) launch_ft_with<CH, UNIFORM>(a, tp, s, sh);
}

void float_temporal(const Filter& f, Channels ch, const StencilLaunch& a, hipStream_t stream, bool launch) {
  PCONV_CHECK(a.depth == 8, "launch_float_temporal: depth 16 not supported (the gaussian on the temporal kernel only)");
  PCONV_CHECK(a.steps >= 1 && a.steps <= kMaxFusedSteps, "float temporal kernel: steps out of range");
  PCONV_CHECK(a.height < (int64_t(1) << 30) && a.g_row0 < (int64_t(1) << 30), "float temporal kernel: rows exceed 2^30");
  PCONV_CHECK(a.row_bytes > 0 && a.row_bytes < (int64_t(1) << 30), "float temporal kernel: row bytes out of range");
  PCONV_CHECK(a.images.images() <= 65535,
              "launch_float_temporal: batch " + std::to_string(a.images.images()) + " exceeds grid.z (65535)");
  FloatTaps tp;
  bool uniform = true;
  for (int i = 0; i < 9; ++i) {
    tp.w[i] = f.weights[i];
    uniform = uniform && f.weights[i] == f.weights[0];
  }
  with_channels(ch, [&](auto chn) {
    constexpr int CH = decltype(chn)::value;
    if (uniform)
      launch_ft<CH, true>(a, tp, stream, launch);
    else
      launch_ft<CH, false>(a, tp, stream, launch);
  });
}

}  // namespace

void launch_float_temporal_checked(const Filter& f, Channels ch, const StencilLaunch& a, hipStream_t stream) {
  float_temporal(f, ch, a, stream, true);
}

void launch_float_temporal(const Filter& f, Channels ch, const StencilLaunch& a, hipStream_t stream) {
  check_image_set("launch_float_temporal", a, channel_count(ch));
  float_temporal(f, ch, a, stream, true);
}

void prepare_float_temporal(const Filter& f, Channels ch, const StencilLaunch& a, hipStream_t stream) {
  check_image_set("launch_float_temporal", a, channel_count(ch));
  float_temporal(f, ch, a, stream, false);
}

std::vector<FloatShape> float_shapes() {
  return std::vector<FloatShape>(std::begin(kFtShapes), std::end(kFtShapes));
}

FloatShape last_float_launch() {
  const int v = g_ft_last_launch.load(std::memory_order_relaxed);
  return FloatShape{v >> 8, v & 0xff};
}

void set_float_shape(int m, int nw) {
  g_ft_force_m.store(m > 0 ? m : 0, std::memory_order_relaxed);
  g_ft_force_nw.store(m > 0 ? nw : 0, std::memory_order_relaxed);
}

void clear_float_tuning() {
  std::lock_guard<std::mutex> lk(g_ft_mu);
  g_ft_tuned.clear();
}

std::vector<std::pair<std::vector<int64_t>, FloatShape>> float_tuned() {
  std::lock_guard<std::mutex> lk(g_ft_mu);
  std::vector<std::pair<std::vector<int64_t>, FloatShape>> out;
  for (const auto& kv : g_ft_tuned)
    out.push_back({{kv.first.ch, kv.first.uniform ? 1 : 0, kv.first.steps, kv.first.rows, kv.first.row_bytes,
                    kv.first.batch, kv.first.live},
                   kv.second});
  return out;
}

}  // namespace pconv
