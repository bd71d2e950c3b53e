// Temporal-blocked gaussian for 16-bit samples (StencilLaunch::depth == 16).
//
// The step is stencil_swar.hip's, unchanged (swar_device.hpp: horiz_b,
// edge_rows, swar_step, run_steps): plain 32-bit adds on "fields", DPP lane
// crossing, boundary rows through LDS, interior rows first, the paired step
// form, the replicate border's corrections.  What differs is what a register
// holds: ONE sample, zero-extended into its own u32 (field width 1), so the
// truncation needs no mask and nothing can carry out of a field:
//   a step sum                  <= 16 x 65535       < 2^20,
//   a sum of x16 intermediates  <= 16 x 16 x 65535  < 2^28,
//   the replicate border adds an edge sample where the zero border adds 0.
// out = (sum w p) >> 4 equals the reference's float32 evaluation for 16-bit
// samples too (every product exact, every partial sum a multiple of 1/16
// below 2^16: 20 significant bits), docs/ARCHITECTURE.md 1.
//
// Layout: per row a lane holds NP samples of one column strip (no A/B strip
// pairing), loaded as one 8- or 16-byte chunk and split with shift / AND; the
// tap distance is CH samples.  hl = ceil(steps CH / NP) halo lanes per side,
// (64 - 2 hl) NP valid samples per strip, M NW - 2 steps valid rows per tile.
// Columns are counted in SAMPLES below (row_bytes / 2 per row).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "pconv/device.hpp"
#include "image_set.hpp"
#include "swar.hpp"
#include "swar_device.hpp"
#include "tuning.hpp"

namespace pconv {
namespace {

template <int NP>
struct Chunk16;  // raw bytes of one lane's NP samples
template <>
struct Chunk16<4> {
  using T = uint2;
  __device__ static T zero() { return make_uint2(0, 0); }
};
template <>
struct Chunk16<8> {
  using T = uint4;
  __device__ static T zero() { return make_uint4(0, 0, 0, 0); }
};

template <int NP>
__device__ __forceinline__ void words_of(const typename Chunk16<NP>::T& v, u32 (&w)[NP / 2]) {
  w[0] = v.x;
  w[1] = v.y;
  if constexpr (NP == 8) {
    w[2] = v.z;
    w[3] = v.w;
  }
}

// One sample per register, cut to the chunk's valid samples (cm: all ones or
// zero per register).  The cut stands here, where the chunk is consumed, and
// not in the branch that loads it (stencil_swar.hip, mask_chunk): what follows
// a row is the zero pad only when the image is the envelope.
template <int NP>
__device__ __forceinline__ void unpack16(const typename Chunk16<NP>::T& v, const u32 (&cm)[NP], u32 (&D)[NP]) {
  u32 w[NP / 2];
  words_of<NP>(v, w);
#pragma unroll
  for (int j = 0; j < NP / 2; ++j) {
    D[2 * j] = (w[j] & 0xffffu) & cm[2 * j];
    D[2 * j + 1] = (w[j] >> 16) & cm[2 * j + 1];
  }
}

template <int NP>
__device__ __forceinline__ typename Chunk16<NP>::T pack16(const u32 (&D)[NP]) {
  u32 w[NP / 2];
#pragma unroll
  for (int j = 0; j < NP / 2; ++j) w[j] = D[2 * j] | (D[2 * j + 1] << 16);
  if constexpr (NP == 8)
    return make_uint4(w[0], w[1], w[2], w[3]);
  else
    return make_uint2(w[0], w[1]);
}

// EdgeFix masks of a lane whose samples sit at columns p + k of a row of
// `row_samples`: all ones or zero per register.
template <int CH, int NP>
__device__ __forceinline__ void edge_masks16(EdgeFix<CH, NP, true>& e, int p, int row_samples) {
#pragma unroll
  for (int k = 0; k < CH; ++k) e.eml[k] = p == 0 ? 0xffffffffu : 0u;
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    const int c = p + k;
    e.emr[k] = (c >= row_samples - CH && c < row_samples && c >= 0) ? 0xffffffffu : 0u;
  }
}

template <int CH, int NP, int M>
__device__ __forceinline__ void edge_fix16(EdgeFix<CH, NP, true>& ef, int base, int lane, int row_samples, int row_base,
                                           int g_row0, int height) {
  edge_masks16<CH, NP>(ef, base + lane * NP, row_samples);
  ef.h = base <= 0 || (base < row_samples && base + 64 * NP > row_samples - CH);
  ef.above_own = -g_row0 - row_base == 0;
  ef.below_own = height - 1 - g_row0 - row_base == M - 1;
}
template <int CH, int NP, int M>
__device__ __forceinline__ void edge_fix16(EdgeFix<CH, NP, false>&, int, int, int, int, int, int) {}

template <int CH, int NP, int M, int NW, int FORM, bool REP = false>
__global__ __launch_bounds__(64 * NW) void k_swar16(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                    int64_t pitch, int row_bytes, int r0, int r1, int steps,
                                                    int g_row0, int height, int row_tiles, int xcd_swizzle,
                                                    int tiles_per_image, int64_t batch_stride,
                                                    const ImageDims* __restrict__ dims,
                                                    const int32_t* __restrict__ active, unsigned last_frame) {
  static_assert(NP == 4 || NP == 8, "a lane loads 8 or 16 bytes");
  constexpr int NQ = NP / 4;
  using CT = typename Chunk16<NP>::T;
  // [parity][wave][boundary rows: top, bottom][quad][lane]
  __shared__ uint4 lds[2][NW][2][NQ][64];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int hl = (steps * CH + NP - 1) / NP;  // halo lanes per side
  const int vs = (64 - 2 * hl) * NP;          // valid output samples per strip
  const int vrows = NW * M - 2 * steps;
  // The image-set preamble is k_swar's (stencil_swar.hip): the XCD-aware tile
  // order over images x tiles_per_image, the active table with the unsigned
  // min, the dims clamp and early exit, the frame offset in 64 bits.
  int tile = static_cast<int>(blockIdx.x);
  if (xcd_swizzle) {
    const int nwg = static_cast<int>(gridDim.x);
    const int q = nwg >> 3, rem = nwg & 7, xcd = tile & 7, local = tile >> 3;
    tile = xcd * q + min(xcd, rem) + local;
  }
  {
    int img = tile / tiles_per_image;
    tile -= img * tiles_per_image;
    if (active != nullptr) img = static_cast<int>(min(static_cast<unsigned>(active[img]), last_frame));
    src += static_cast<int64_t>(img) * batch_stride;
    dst += static_cast<int64_t>(img) * batch_stride;
    if (dims != nullptr) {
      const ImageDims d = dims[img];
      row_bytes = min(d.row_bytes, row_bytes);
      height = min(d.height, height);
      const int col0 = tile / row_tiles;
      if (col0 * vs >= (row_bytes >> 1) || r0 + (tile - col0 * row_tiles) * vrows + g_row0 >= height) return;
    }
  }
  const int row_samples = row_bytes >> 1;
  const int col = tile / row_tiles, rtile = tile - col * row_tiles;
  const int base = col * vs - hl * NP;  // a multiple of NP: a lane lies left of column 0 or at / right of it
  const int x = base + lane * NP;
  const int valid = x >= 0 ? min(max(row_samples - x, 0), NP) : 0;
  const bool needs_mask = base < 0 || base + 64 * NP > row_samples;
  u32 cm[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) cm[k] = k < valid ? 0xffffffffu : 0u;

  const int tile_r0 = r0 + rtile * vrows;
  const int row_base = tile_r0 - steps + w * M;
  const int lo_ok = max(r0 - steps, -g_row0), hi_ok = min(r1 + steps, height - g_row0);

  u32 D[M][NP];
#pragma unroll
  for (int i = 0; i < M; ++i) {
    const int fr = row_base + i;
    const bool rok = fr >= lo_ok && fr < hi_ok;
    CT v = Chunk16<NP>::zero();
    if (rok && valid > 0) v = *reinterpret_cast<const CT*>(src + static_cast<int64_t>(fr) * pitch + 2 * x);
    unpack16<NP>(v, cm, D[i]);
  }
  const int out_top = min(max(-g_row0 - row_base, 0), M);
  const int out_bot = min(max(height - g_row0 - row_base, 0), M);

  EdgeFix<CH, NP, REP> ef;
  edge_fix16<CH, NP, M>(ef, base, lane, row_samples, row_base, g_row0, height);

  run_steps<CH, NP, M, NW, FORM, REP, 1>(D, lds, steps, w, lane, needs_mask, cm, out_top, out_bot, ef);

  const bool st = lane >= hl && lane < 64 - hl && valid > 0;
  const int st_lo = max(tile_r0, r0), st_hi = min(min(tile_r0 + vrows, r1), height - g_row0);
#pragma unroll
  for (int i = 0; i < M; ++i) {
    const int fr = row_base + i;
    if (st && fr >= st_lo && fr < st_hi) {
      uint8_t* q = dst + static_cast<int64_t>(fr) * pitch + 2 * x;
      // Whole chunks as one store; the row's last partial chunk sample by
      // sample (dst may be a packed buffer with nothing after the row).
      if (valid == NP) {
        *reinterpret_cast<CT*>(q) = pack16<NP>(D[i]);
      } else {
#pragma unroll
        for (int k = 0; k < NP; ++k)
          if (k < valid) reinterpret_cast<uint16_t*>(q)[k] = static_cast<uint16_t>(D[i][k]);
      }
    }
  }
}

// Instantiated tile shapes (samples per lane, rows per wave, waves), written
// here and nowhere else; largest tile (least halo) first, and the order is
// behaviour: pick_shape16 returns the first row whose grid fills the chip.
constexpr SwarShape kTiles16[] = {{8, 8, 8}, {4, 16, 4}, {4, 8, 8}, {4, 4, 8}, {4, 2, 16}};
constexpr size_t kNumTiles16 = sizeof(kTiles16) / sizeof(kTiles16[0]);

size_t tile16_index(const SwarShape& s) {
  size_t i = 0;
  while (i < kNumTiles16 && (kTiles16[i].lw != s.lw || kTiles16[i].m != s.m || kTiles16[i].nw != s.nw)) ++i;
  return i;
}

// Grid of one launch of a shape: the host's one copy of what the kernel
// derives from (steps, CH, NP, M, NW).
struct Geom16 {
  bool ok = false;  // the halo leaves valid output and a lane holds a whole pixel
  int vs = 0;       // valid output samples per strip
  int vrows = 0;    // valid output rows per tile
  int64_t nstrips = 0, row_tiles = 0, tiles_per_image = 0;
  int64_t tiles = 0;  // workgroups: images x tiles_per_image
};

Geom16 geom16(const SwarShape& sh, int ch, int steps, int64_t rows, int64_t row_bytes, int images = 1) {
  Geom16 g;
  const int hl = (steps * ch + sh.lw - 1) / sh.lw;
  g.vs = (64 - 2 * hl) * sh.lw;
  g.vrows = sh.m * sh.nw - 2 * steps;
  g.ok = g.vs > 0 && g.vrows > 0 && sh.lw >= ch;
  if (!g.ok) return g;
  g.nstrips = ceil_div<int64_t>(row_bytes / 2, g.vs);
  g.row_tiles = ceil_div<int64_t>(rows, g.vrows);
  g.tiles_per_image = g.nstrips * g.row_tiles;
  g.tiles = g.tiles_per_image * images;
  return g;
}

// A lane's chunk is 2 lw bytes at a multiple of that from a row's column 0:
// both frames, the pitch and the frame stride must keep it aligned.
bool aligned16(const SwarShape& sh, const StencilLaunch& a) {
  const uintptr_t lb = 2 * static_cast<uintptr_t>(sh.lw);
  return reinterpret_cast<uintptr_t>(a.src) % lb == 0 && reinterpret_cast<uintptr_t>(a.dst) % lb == 0 &&
         static_cast<uintptr_t>(a.pitch) % lb == 0 && static_cast<uintptr_t>(a.images.stride) % lb == 0;
}

bool runs16(const SwarShape& sh, int ch, const StencilLaunch& a) {
  return geom16(sh, ch, a.steps, a.r1 - a.r0, a.row_bytes).ok && aligned16(sh, a);
}

template <int CH, size_t I>
void launch_tile16(const StencilLaunch& a, hipStream_t s, int form) {
  constexpr SwarShape S = kTiles16[I];
  const char* who = "swar16 temporal kernel";
  const Geom16 g = geom16(S, CH, a.steps, a.r1 - a.r0, a.row_bytes, a.images.images());
  const BatchKernelArgs b = batch_kernel_args(a);
  PCONV_CHECK(g.ok, std::string(who) + ": steps too large for the tile");
  PCONV_CHECK(aligned16(S, a), std::string(who) + ": src, dst, pitch and batch_stride must be multiples of " +
                                   std::to_string(2 * S.lw) + " bytes for a tile of " + std::to_string(S.lw) +
                                   " samples per lane");
  PCONV_CHECK(g.tiles < (int64_t(1) << 31), std::string(who) + ": too many tiles (batch x tiles per image)");
  static_assert(S.lw >= CH, "a lane holds a whole pixel");
  {
    using F = decltype(&k_swar16<CH, S.lw, S.m, S.nw, 0>);
    const bool rep = a.border == Border::Replicate;
    const F kern = rep ? (form >= 1 ? static_cast<F>(&k_swar16<CH, S.lw, S.m, S.nw, 1, true>)
                                    : static_cast<F>(&k_swar16<CH, S.lw, S.m, S.nw, 0, true>))
                       : (form >= 1 ? static_cast<F>(&k_swar16<CH, S.lw, S.m, S.nw, 1>)
                                    : static_cast<F>(&k_swar16<CH, S.lw, S.m, S.nw, 0>));
    const int hmax = static_cast<int>(std::min<int64_t>(a.height, int64_t(1) << 30));
    kern<<<dim3(static_cast<unsigned>(g.tiles)), dim3(64 * S.nw), 0, s>>>(
        a.src, a.dst, a.pitch, static_cast<int>(a.row_bytes), static_cast<int>(a.r0), static_cast<int>(a.r1), a.steps,
        static_cast<int>(a.g_row0), hmax, static_cast<int>(g.row_tiles), swar_xcd_swizzle() ? 1 : 0,
        static_cast<int>(g.tiles_per_image), b.stride, b.dims, b.active, b.last_frame);
  }
}

struct Choice16 {
  SwarShape shape{0, 0, 0};
  int form = 1;
};

void launch_choice16(const StencilLaunch& a, Channels ch, hipStream_t stream, const Choice16& c) {
  const bool known = with_channels(ch, [&](auto chn) {
    return with_index<kNumTiles16>(tile16_index(c.shape),
                                   [&](auto i) { launch_tile16<decltype(chn)::value, decltype(i)::value>(a, stream, c.form); });
  });
  PCONV_CHECK(known, "swar16 temporal kernel: unsupported tile shape");
}

std::mutex g_shape16_mu;
bool g_have_shape16 = false;
SwarShape g_shape16;

bool override_shape16(SwarShape& out) {
  std::lock_guard<std::mutex> lk(g_shape16_mu);
  if (g_have_shape16) out = g_shape16;
  return g_have_shape16;
}

// Shape when nothing is tuned, as the float kernel picks its own
// (stencil_float.hip, pick_ft_shape): the first row, largest tile first, whose
// grid gives at least 3/4 of the CUs a workgroup and whose last round of
// workgroups is at least 3/4 full; a small frame takes the shape with the most
// workgroups.  Not a fitted model: docs/PERFORMANCE.md 3.7.
SwarShape pick_shape16(int ch, const StencilLaunch& a) {
  static int cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
      n = 256;
    return std::max(1, n);
  }();
  SwarShape most{0, 0, 0};
  int64_t most_wgs = -1;
  for (const auto& c : kTiles16) {
    if (!runs16(c, ch, a)) continue;
    const int64_t wgs = geom16(c, ch, a.steps, a.r1 - a.r0, a.row_bytes, a.images.images()).tiles;
    const int64_t rounds = ceil_div<int64_t>(wgs, cus);
    if (4 * wgs >= 3 * static_cast<int64_t>(cus) && 4 * wgs >= 3 * rounds * cus) return c;
    if (wgs > most_wgs) {
      most_wgs = wgs;
      most = c;
    }
  }
  PCONV_CHECK(most.m > 0, "swar16 temporal kernel: no tile shape runs the launch (steps too large, or src / dst / "
                          "pitch not 8-byte aligned)");
  return most;
}

// First-use tuning, keyed as the SWAR tuner's entries are: channels, steps,
// rows, row bytes, images, live workgroups of a mixed-size launch under the
// pick's shape (0: uniform).  Every shape that runs the launch x both step
// forms is timed on the real launch.  Never on a capturing stream, never for a
// launch with an active table.
struct Key16 {
  int ch, steps;
  int64_t rows, row_bytes;
  int batch;
  int64_t live;
  bool operator<(const Key16& o) const {
    return std::tie(ch, steps, rows, row_bytes, batch, live) <
           std::tie(o.ch, o.steps, o.rows, o.row_bytes, o.batch, o.live);
  }
};
std::mutex g_tune16_mu;
std::map<Key16, Choice16> g_tuned16;

Choice16 tuned_choice16(const StencilLaunch& a, Channels ch, hipStream_t stream) {
  const int c = channel_count(ch), images = a.images.images();
  const int mode = swar_alt_mode();
  Choice16 pick;
  pick.form = mode >= 0 ? mode : 1;
  if (override_shape16(pick.shape)) return pick;  // launch_tile16 names what a forced shape cannot run
  pick.shape = pick_shape16(c, a);
  if (!shape_tuning_enabled()) return pick;
  const Geom16 pg = geom16(pick.shape, c, a.steps, a.r1 - a.r0, a.row_bytes, images);
  // (live_workgroups counts bytes: a strip of vs samples is 2 vs bytes wide)
  const Key16 key{c, a.steps, a.r1 - a.r0, a.row_bytes, images, live_workgroups(a, int64_t(2) * pg.vs, pg.vrows, 1)};
  {
    std::lock_guard<std::mutex> lk(g_tune16_mu);
    auto it = g_tuned16.find(key);
    if (it != g_tuned16.end() && aligned16(it->second.shape, a)) {
      Choice16 r = it->second;
      if (mode >= 0) r.form = mode;
      return r;
    }
  }
  if (stream_capturing(stream) || a.images.has_table()) return pick;
  std::vector<Choice16> cands;
  for (const auto& t : kTiles16)
    if (runs16(t, c, a))
      for (int form = 0; form <= 1; ++form)
        if (mode < 0 || mode == form) cands.push_back(Choice16{t, form});
  const Choice16 best =
      cands[fastest_candidate(cands.size(), stream, [&](size_t i) { launch_choice16(a, ch, stream, cands[i]); })];
  std::lock_guard<std::mutex> lk(g_tune16_mu);
  g_tuned16[key] = best;
  return best;
}

}  // namespace

std::vector<SwarShape> swar16_shapes() { return std::vector<SwarShape>(std::begin(kTiles16), std::end(kTiles16)); }

void set_swar16_shape(int lw, int m, int nw) {
  std::lock_guard<std::mutex> lk(g_shape16_mu);
  if (lw == 0) {
    g_have_shape16 = false;
    return;
  }
  const SwarShape s{lw, m, nw};
  PCONV_CHECK(tile16_index(s) < kNumTiles16, "set_swar16_shape: shape not instantiated");
  g_shape16 = s;
  g_have_shape16 = true;
}

void clear_swar16_tuning() {
  std::lock_guard<std::mutex> lk(g_tune16_mu);
  g_tuned16.clear();
}

std::vector<std::pair<std::vector<int64_t>, SwarShape>> swar16_tuned() {
  std::lock_guard<std::mutex> lk(g_tune16_mu);
  std::vector<std::pair<std::vector<int64_t>, SwarShape>> out;
  for (const auto& kv : g_tuned16)
    out.push_back({{kv.first.ch, kv.first.steps, kv.first.rows, kv.first.row_bytes, kv.second.form, kv.first.batch,
                    kv.first.live},
                   kv.second.shape});
  return out;
}

void prepare_swar16(const StencilLaunch& a, Channels ch, hipStream_t stream) { (void)tuned_choice16(a, ch, stream); }

void launch_swar16(const StencilLaunch& a, Channels ch, hipStream_t stream) {
  launch_choice16(a, ch, stream, tuned_choice16(a, ch, stream));
}

}  // namespace pconv
