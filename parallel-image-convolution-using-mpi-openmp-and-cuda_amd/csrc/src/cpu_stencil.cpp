// CPU stencil oracle + OpenMP backend (see cpu_stencil.hpp).
//
// Compiled with -ffp-contract=off: the float path must be multiply-then-add
// with one rounding each, in row-major tap order, like the x86 gcc reference
// (mpi/mpi_convolution.c:303-307, :313-318).
#include "pconv/cpu_stencil.hpp"

#include <omp.h>
#include <sched.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <sstream>
#include <string>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

namespace pconv {

namespace {

inline uint8_t sat_trunc(float v) {
  // float -> uint8_t truncation; out-of-range values (only possible for custom
  // filters with negative taps) saturate instead of the reference's UB.
  if (!(v > 0.0f)) return 0;
  if (v >= 255.0f) return 255;
  return static_cast<uint8_t>(static_cast<int>(v));
}

// (Σ tap·p) >> 4 with taps [1,2,1]⊗[1,2,1]: the vertical sums of the row once
// into a 16-bit scratch row (every sum <= 1020; the full sum <= 4080 < 2^16),
// then the horizontal pass — two passes of 16-bit lanes the compiler
// vectorises.  Built twice: the x86-64 baseline and an AVX2 clone picked at
// run time (the GPU boxes' and this container's CPUs have AVX2; no -march
// flag, so the binary still runs anywhere).
#define PCONV_ROW_BINOMIAL_BODY                                                               \
  for (int64_t x = -CH; x < n + CH; ++x) v[x + CH] = static_cast<uint16_t>(a[x] + 2 * b[x] + c[x]); \
  for (int64_t x = 0; x < n; ++x)                                                             \
    o[x] = static_cast<uint8_t>(static_cast<uint16_t>(v[x] + 2 * v[x + CH] + v[x + 2 * CH]) >> 4);

template <int CH>
void row_binomial_base(const uint8_t* a, const uint8_t* b, const uint8_t* c, uint8_t* o, int64_t n, uint16_t* v) {
  PCONV_ROW_BINOMIAL_BODY
}

template <int CH>
__attribute__((target("avx2"))) void row_binomial_avx2(const uint8_t* a, const uint8_t* b, const uint8_t* c,
                                                       uint8_t* o, int64_t n, uint16_t* v) {
  PCONV_ROW_BINOMIAL_BODY
}
#undef PCONV_ROW_BINOMIAL_BODY

template <int CH>
void row_binomial(const uint8_t* a, const uint8_t* b, const uint8_t* c, uint8_t* o, int64_t n) {
  static const bool avx2 = __builtin_cpu_supports("avx2");
  thread_local std::vector<uint16_t> scratch;
  if (scratch.size() < static_cast<size_t>(n + 2 * CH)) scratch.resize(static_cast<size_t>(n + 2 * CH));
  if (avx2)
    row_binomial_avx2<CH>(a, b, c, o, n, scratch.data());
  else
    row_binomial_base<CH>(a, b, c, o, n, scratch.data());
}

// The same two passes on 16-bit samples (depth 16): a vertical sum is at most
// 4 x 65535, the full sum 16 x 65535 < 2^20, so the scratch row is 32 bits
// wide.  Baseline build only.
template <int CH>
void row_binomial(const uint16_t* a, const uint16_t* b, const uint16_t* c, uint16_t* o, int64_t n) {
  thread_local std::vector<uint32_t> scratch;
  if (scratch.size() < static_cast<size_t>(n + 2 * CH)) scratch.resize(static_cast<size_t>(n + 2 * CH));
  uint32_t* v = scratch.data();
  for (int64_t x = -CH; x < n + CH; ++x) v[x + CH] = uint32_t{a[x]} + 2 * uint32_t{b[x]} + uint32_t{c[x]};
  for (int64_t x = 0; x < n; ++x) o[x] = static_cast<uint16_t>((v[x] + 2 * v[x + CH] + v[x + 2 * CH]) >> 4);
}

// Integer-exact custom filters (non-negative taps, power-of-two divisor).
#define PCONV_ROW_INT_BODY                                                                          \
  const int t0 = t[0], t1 = t[1], t2 = t[2], t3 = t[3], t4 = t[4], t5 = t[5], t6 = t[6], t7 = t[7], \
            t8 = t[8];                                                                              \
  for (int64_t x = 0; x < n; ++x) {                                                                 \
    const int acc = t0 * a[x - CH] + t1 * a[x] + t2 * a[x + CH] + t3 * b[x - CH] + t4 * b[x] +       \
                    t5 * b[x + CH] + t6 * c[x - CH] + t7 * c[x] + t8 * c[x + CH];                   \
    o[x] = static_cast<uint8_t>(std::min(acc >> s, 255));                                            \
  }

template <int CH>
void row_int_base(const int* t, int s, const uint8_t* a, const uint8_t* b, const uint8_t* c, uint8_t* o, int64_t n) {
  PCONV_ROW_INT_BODY
}

template <int CH>
__attribute__((target("avx2"))) void row_int_avx2(const int* t, int s, const uint8_t* a, const uint8_t* b,
                                                  const uint8_t* c, uint8_t* o, int64_t n) {
  PCONV_ROW_INT_BODY
}
#undef PCONV_ROW_INT_BODY

template <int CH>
void row_int(const Filter& f, const uint8_t* a, const uint8_t* b, const uint8_t* c, uint8_t* o, int64_t n) {
  static const bool avx2 = __builtin_cpu_supports("avx2");
  if (avx2)
    row_int_avx2<CH>(f.taps.data(), f.shift, a, b, c, o, n);
  else
    row_int_base<CH>(f.taps.data(), f.shift, a, b, c, o, n);
}

// Float filters: per output, acc = 0; acc += fl(p * w) over the nine taps in
// row-major order (the reference's sequence, one rounding per op, no FMA:
// -ffp-contract=off, and the AVX2 clone does not enable FMA).  Outputs are
// independent, so vectorising across x keeps every output's order.
#define PCONV_ROW_FLOAT_BODY                                                                  \
  const float w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4], w5 = w[5], w6 = w[6], w7 = w[7], \
              w8 = w[8];                                                                      \
  for (int64_t x = 0; x < n; ++x) {                                                           \
    float acc = 0.0f;                                                                         \
    acc = acc + static_cast<float>(a[x - CH]) * w0;                                           \
    acc = acc + static_cast<float>(a[x]) * w1;                                                \
    acc = acc + static_cast<float>(a[x + CH]) * w2;                                           \
    acc = acc + static_cast<float>(b[x - CH]) * w3;                                           \
    acc = acc + static_cast<float>(b[x]) * w4;                                                \
    acc = acc + static_cast<float>(b[x + CH]) * w5;                                           \
    acc = acc + static_cast<float>(c[x - CH]) * w6;                                           \
    acc = acc + static_cast<float>(c[x]) * w7;                                                \
    acc = acc + static_cast<float>(c[x + CH]) * w8;                                           \
    o[x] = sat_trunc(acc);                                                                    \
  }

template <int CH>
void row_float_base(const float* w, const uint8_t* a, const uint8_t* b, const uint8_t* c, uint8_t* o, int64_t n) {
  PCONV_ROW_FLOAT_BODY
}

template <int CH>
__attribute__((target("avx2"))) void row_float_avx2(const float* w, const uint8_t* a, const uint8_t* b,
                                                    const uint8_t* c, uint8_t* o, int64_t n) {
  PCONV_ROW_FLOAT_BODY
}
#undef PCONV_ROW_FLOAT_BODY

template <int CH>
void row_float(const Filter& f, const uint8_t* a, const uint8_t* b, const uint8_t* c, uint8_t* o, int64_t n) {
  static const bool avx2 = __builtin_cpu_supports("avx2");
  if (avx2)
    row_float_avx2<CH>(f.weights.data(), a, b, c, o, n);
  else
    row_float_base<CH>(f.weights.data(), a, b, c, o, n);
}

// Replicate border: row `p` (n bytes) with its first and last pixel repeated
// once on either side, in `buf` (n + 2 CH bytes); returns the column-0 pointer.
// The source frame is only read: its pad columns and ghost rows stay as they are.
template <int CH, class T>
const T* edge_padded(const T* p, int64_t n, T* buf) {
  std::memcpy(buf + CH, p, static_cast<size_t>(n) * sizeof(T));
  for (int k = 0; k < CH; ++k) {
    buf[k] = p[k];
    buf[CH + n + k] = p[n - CH + k];
  }
  return buf + CH;
}

// One output row from its three input rows (column -CH .. n + CH readable).
// 16-bit samples: the gaussian only (cpu_step refuses the others by name).
template <int CH>
void eval_row(const Filter&, const uint16_t* a, const uint16_t* b, const uint16_t* c, uint16_t* o, int64_t n) {
  row_binomial<CH>(a, b, c, o, n);
}
template <int CH>
void eval_row(const Filter& f, const uint8_t* a, const uint8_t* b, const uint8_t* c, uint8_t* o, int64_t n) {
  if (f.binomial121)
    row_binomial<CH>(a, b, c, o, n);
  else if (f.int_exact)
    row_int<CH>(f, a, b, c, o, n);
  else
    row_float<CH>(f, a, b, c, o, n);
}

// Replicate border, frame row r: the three input rows with the taps clamped
// to the GLOBAL image — the row above global row 0 is row 0, the row below
// the last is the last; columns through padded copies, so the same row
// kernels (integer / float, baseline / AVX2) serve.
// Frame row r as samples of type T (uint8_t, or uint16_t at depth 16: a frame's
// data column 0 and pitch are 16-byte multiples, so the rows are aligned).
template <class T>
const T* row_ptr(const FrameLayout& lay, const uint8_t* frame, int64_t r) {
  return reinterpret_cast<const T*>(frame + lay.offset(r));
}

template <int CH, class T>
void replicate_rows(const FrameLayout& lay, const uint8_t* src, int64_t r, int64_t g_row0, int64_t height,
                    const T*& a, const T*& b, const T*& c) {
  const int64_t n = lay.row_bytes / static_cast<int64_t>(sizeof(T));
  thread_local std::vector<T> rows3;
  const size_t w = static_cast<size_t>(n + 2 * CH);
  if (rows3.size() < 3 * w) rows3.resize(3 * w);
  const int64_t g = g_row0 + r;
  const T* pb = row_ptr<T>(lay, src, r);
  const T* pa = g - 1 >= 0 ? row_ptr<T>(lay, src, r - 1) : pb;
  const T* pc = g + 1 < height ? row_ptr<T>(lay, src, r + 1) : pb;
  a = edge_padded<CH>(pa, n, rows3.data());
  c = edge_padded<CH>(pc, n, rows3.data() + 2 * w);
  b = edge_padded<CH>(pb, n, rows3.data() + w);
}

// The three input rows of frame row r (columns -CH .. n + CH readable).
// Replicate: replicate_rows.  Zero: the frame's rows as they are (its ghost
// rows and pad columns are the border), unless zero_outside: then a row
// outside the global image is a row of zeros, whatever the frame holds there.
template <int CH, class T>
void input_rows(const FrameLayout& lay, const uint8_t* src, int64_t r, Border border, int64_t g_row0, int64_t height,
                bool zero_outside, const T*& a, const T*& b, const T*& c) {
  a = row_ptr<T>(lay, src, r - 1);
  b = row_ptr<T>(lay, src, r);
  c = row_ptr<T>(lay, src, r + 1);
  if (border == Border::Replicate) {
    replicate_rows<CH>(lay, src, r, g_row0, height, a, b, c);
  } else if (zero_outside) {
    const int64_t g = g_row0 + r;
    if (g - 1 < 0 || g + 1 >= height) {
      thread_local std::vector<T> zeros;
      const size_t w = static_cast<size_t>(lay.row_bytes / sizeof(T) + 2 * CH);
      if (zeros.size() < w) zeros.assign(w, 0);
      if (g - 1 < 0) a = zeros.data() + CH;
      if (g + 1 >= height) c = zeros.data() + CH;
    }
  }
}

// Sum of body(r) over rows [r0, r1) of n bytes each: serial, or an OpenMP
// team.  Below ~32 KiB a pass over the rows is a few microseconds on one
// core: the team's fork/join costs as much, and on a loaded host a preempted
// team member stalls the barrier for a whole scheduler slice.
template <class Body>
uint64_t sum_rows(int64_t r0, int64_t r1, int64_t n, CpuBackend be, Body&& body) {
  uint64_t total = 0;
  if (be == CpuBackend::OpenMP) {
    const bool team = (r1 - r0) * n >= (int64_t{32} << 10);
#pragma omp parallel for schedule(static) reduction(+ : total) if (team)
    for (int64_t r = r0; r < r1; ++r) total += body(r);
  } else {
    for (int64_t r = r0; r < r1; ++r) total += body(r);
  }
  return total;
}

template <int CH, class T = uint8_t>
void step_rows(const Filter& f, const FrameLayout& lay, const uint8_t* src, uint8_t* dst, int64_t r0, int64_t r1,
               CpuBackend be, Border border, int64_t g_row0, int64_t height) {
  (void)sum_rows(r0, r1, lay.row_bytes, be, [&](int64_t r) -> uint64_t {
    const T *a, *b, *c;
    input_rows<CH>(lay, src, r, border, g_row0, height, false, a, b, c);
    eval_row<CH>(f, a, b, c, reinterpret_cast<T*>(dst + lay.offset(r)), lay.row_bytes / static_cast<int64_t>(sizeof(T)));
    return 0;
  });
}

// step_rows' evaluation into a scratch row, compared with the source row and
// counted.
template <int CH>
uint64_t residual_rows(const Filter& f, const FrameLayout& lay, const uint8_t* src, int64_t r0, int64_t r1,
                       CpuBackend be, Border border, int64_t g_row0, int64_t height) {
  const int64_t n = lay.row_bytes;
  return sum_rows(r0, r1, n, be, [&](int64_t r) -> uint64_t {
    thread_local std::vector<uint8_t> scratch;
    if (scratch.size() < static_cast<size_t>(n)) scratch.resize(static_cast<size_t>(n));
    const uint8_t *a, *b, *c;
    input_rows<CH>(lay, src, r, border, g_row0, height, true, a, b, c);
    uint8_t* o = scratch.data();
    eval_row<CH>(f, a, b, c, o, n);
    uint64_t cnt = 0;
    for (int64_t x = 0; x < n; ++x) cnt += o[x] != b[x];
    return cnt;
  });
}

// fn(std::integral_constant<int, bytes per pixel>) for the channel layout.
template <class F>
auto with_channels(Channels ch, F&& fn) {
  using std::integral_constant;
  return ch == Channels::Grey ? fn(integral_constant<int, 1>{})
                              : ch == Channels::Rgb ? fn(integral_constant<int, 3>{}) : fn(integral_constant<int, 4>{});
}

}  // namespace

uint64_t cpu_residual(const Filter& f, Channels ch, const FrameLayout& lay, const uint8_t* src_frame, int64_t r0,
                      int64_t r1, CpuBackend be, Border border, int64_t g_row0, int64_t height) {
  if (height < 0) height = g_row0 + lay.rows;  // the frame's owned rows end the image
  r0 = std::max(r0, -g_row0);
  r1 = std::min(r1, height - g_row0);
  if (r1 <= r0) return 0;
  PCONV_CHECK(r0 >= -lay.halo + 1 && r1 <= lay.rows + lay.halo - 1, "cpu_residual: rows out of frame");
  return with_channels(ch, [&](auto chn) {
    return residual_rows<decltype(chn)::value>(f, lay, src_frame, r0, r1, be, border, g_row0, height);
  });
}

void cpu_step(const Filter& f, Channels ch, const FrameLayout& lay, const uint8_t* src_frame, uint8_t* dst_frame,
              int64_t r0, int64_t r1, CpuBackend be, Border border, int64_t g_row0, int64_t height, int depth) {
  PCONV_CHECK(depth == 8 || depth == 16, "cpu_step: depth must be 8 or 16");
  if (depth == 16) {
    PCONV_CHECK(f.binomial121, "cpu_step: depth 16 runs the gaussian filter only, not '" + f.name + "'");
    PCONV_CHECK(lay.row_bytes % (2 * channel_count(ch)) == 0, "cpu_step: row bytes are no whole depth-16 pixels");
  }
  PCONV_CHECK(r0 >= -lay.halo + 1 && r1 <= lay.rows + lay.halo - 1 && r0 <= r1, "cpu_step: rows out of frame");
  if (height < 0) height = g_row0 + lay.rows;  // the frame's owned rows end the image
  if (border != Border::Zero)
    PCONV_CHECK(r0 >= r1 || (g_row0 + r0 >= 0 && g_row0 + r1 <= height),
                "cpu_step: a non-zero border computes rows of the global image only");
  with_channels(ch, [&](auto chn) {
    if (depth == 16)
      step_rows<decltype(chn)::value, uint16_t>(f, lay, src_frame, dst_frame, r0, r1, be, border, g_row0, height);
    else
      step_rows<decltype(chn)::value>(f, lay, src_frame, dst_frame, r0, r1, be, border, g_row0, height);
  });
}

void cpu_fused_launch(const Filter& f, Channels ch, const FrameLayout& lay, const uint8_t* src_frame,
                      uint8_t* dst_frame, int64_t lo, int64_t hi, int steps, int64_t g_row0, int64_t height,
                      CpuBackend be, Border border, int depth) {
  PCONV_CHECK(steps >= 1 && lo <= hi, "cpu_fused_launch: bad arguments");
  PCONV_CHECK(lo - steps >= -lay.halo && hi + steps <= lay.rows + lay.halo, "cpu_fused_launch: rows exceed frame");
  if (lo == hi) return;
  if (steps == 1) {
    // Single step never writes rows outside the image: clip like the kernels' caller.
    const int64_t a = std::max(lo, -g_row0), b = std::min(hi, height - g_row0);
    if (a < b) cpu_step(f, ch, lay, src_frame, dst_frame, a, b, be, border, g_row0, height, depth);
    return;
  }
  const size_t n = static_cast<size_t>(lay.bytes());
  std::vector<uint8_t> A(src_frame, src_frame + n), B(src_frame, src_frame + n);
  uint8_t* cur = A.data();
  uint8_t* nxt = B.data();
  for (int j = 1; j <= steps; ++j) {
    const int64_t ext = steps - j;
    const int64_t a = std::max(lo - ext, -g_row0), b = std::min(hi + ext, height - g_row0);
    if (a < b) cpu_step(f, ch, lay, cur, nxt, a, b, be, border, g_row0, height, depth);
    std::swap(cur, nxt);
  }
  for (int64_t r = lo; r < hi; ++r) {
    const bool inside = g_row0 + r >= 0 && g_row0 + r < height;
    if (inside)
      std::memcpy(dst_frame + lay.offset(r), cur + lay.offset(r), lay.row_bytes);
    else
      std::memset(dst_frame + lay.offset(r), 0, lay.row_bytes);
  }
}

namespace {

int cgroup_cpu_quota() {
  // cgroup v2: "max 100000" or "<quota> <period>"; v1: cfs_quota_us / cfs_period_us.
  if (FILE* f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {
    char q[32] = {0};
    long long period = 0;
    const int n = std::fscanf(f, "%31s %lld", q, &period);
    std::fclose(f);
    if (n == 2 && std::strcmp(q, "max") != 0 && period > 0) {
      const long long quota = std::atoll(q);
      if (quota > 0) return static_cast<int>((quota + period - 1) / period);
    }
    return 0;
  }
  long long quota = -1, period = 0;
  if (FILE* f = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {
    if (std::fscanf(f, "%lld", &quota) != 1) quota = -1;
    std::fclose(f);
  }
  if (FILE* f = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) {
    if (std::fscanf(f, "%lld", &period) != 1) period = 0;
    std::fclose(f);
  }
  return quota > 0 && period > 0 ? static_cast<int>((quota + period - 1) / period) : 0;
}

}  // namespace

int default_cpu_threads() {
  cpu_set_t set;
  CPU_ZERO(&set);
  int n = sched_getaffinity(0, sizeof(set), &set) == 0 ? CPU_COUNT(&set) : omp_get_num_procs();
  const int q = cgroup_cpu_quota();
  if (q > 0) n = std::min(n, q);
  if (n > 2) n -= 1;
  return std::max(1, n);
}

int configure_cpu_threads(int share) {
  if (std::getenv("OMP_NUM_THREADS")) return omp_get_max_threads();
  const int n = std::max(1, default_cpu_threads() / std::max(1, share));
  omp_set_num_threads(n);
  return n;
}

namespace {

// OpenMP team of a whole-image call, restored on exit: `threads`, or
// default_cpu_threads() when neither it nor OMP_NUM_THREADS says.
struct TeamScope {
  int saved = omp_get_max_threads();
  bool set = false;
  TeamScope(CpuBackend be, int threads) {
    if (be == CpuBackend::OpenMP && threads <= 0 && !std::getenv("OMP_NUM_THREADS")) threads = default_cpu_threads();
    set = be == CpuBackend::OpenMP && threads > 0;
    if (set) omp_set_num_threads(threads);
  }
  ~TeamScope() {
    if (set) omp_set_num_threads(saved);
  }
};

}  // namespace

HostFrames::HostFrames(const Filter& f, const ImageGeom& geom, CpuBackend be, Border border)
    : f_(f), geom_(geom), be_(be), border_(border) {
  geom_.validate();
  lay_ = FrameLayout::make(geom_.row_bytes(), geom_.height, 1);
}

void HostFrames::load(const std::function<void(uint8_t* row0, int64_t pitch)>& fill) {
  cur_.assign(static_cast<size_t>(lay_.bytes()), 0);
  nxt_.assign(static_cast<size_t>(lay_.bytes()), 0);
  fill(cur_.data() + lay_.offset(0), lay_.pitch);
}

void HostFrames::load(const uint8_t* in) {
  const int64_t rb = lay_.row_bytes;
  load([&](uint8_t* row0, int64_t pitch) {
    for (int64_t r = 0; r < geom_.height; ++r) std::memcpy(row0 + r * pitch, in + r * rb, static_cast<size_t>(rb));
  });
}

void HostFrames::release() {
  std::vector<uint8_t>().swap(cur_);
  std::vector<uint8_t>().swap(nxt_);
}

void HostFrames::step() {
  cpu_step(f_, geom_.channels, lay_, cur_.data(), nxt_.data(), 0, geom_.height, be_, border_, 0, geom_.height,
           geom_.depth);
  cur_.swap(nxt_);  // newest result is always in `cur_` (fixes SURVEY §A3)
}

uint64_t HostFrames::residual() const {
  PCONV_CHECK(geom_.depth == 8, "residual: depth 16 not supported (no fixed-point check for 16-bit samples)");
  return cpu_residual(f_, geom_.channels, lay_, cur_.data(), 0, geom_.height, be_, border_, 0, geom_.height);
}

void HostFrames::copy_out(uint8_t* out) const {
  const int64_t rb = lay_.row_bytes;
  for (int64_t r = 0; r < geom_.height; ++r)
    std::memcpy(out + r * rb, cur_.data() + lay_.offset(r), static_cast<size_t>(rb));
}

void HostFrames::copy_out_decimated(uint8_t* out, int factor) const {
  if (factor == 1) return copy_out(out);
  const ImageGeom og = decimated_geom(geom_, factor);
  const int64_t pb = geom_.pixel_bytes(), orb = og.row_bytes(), hop = pb * factor;
  const bool omp = be_ == CpuBackend::OpenMP;
#pragma omp parallel for schedule(static) if (omp)
  for (int64_t y = 0; y < og.height; ++y) {
    const uint8_t* s = cur_.data() + lay_.offset(y * factor);
    uint8_t* d = out + y * orb;
    for (int64_t x = 0; x < og.width; ++x) std::memcpy(d + x * pb, s + x * hop, static_cast<size_t>(pb));
  }
}

StableStats HostFrames::run_until_stable(int max_reps, int check_every) {
  PCONV_CHECK(max_reps >= 0, "repetitions must be >= 0");
  PCONV_CHECK(check_every >= 1, "check_every must be >= 1");
  StableStats st;
  do {
    const int k = std::min(check_every, max_reps - st.reps_done);
    for (int t = 0; t < k; ++t) step();
    st.reps_done += k;
    st.residual = residual();
    ++st.checks;
    st.converged = st.residual == 0;
  } while (!st.converged && st.reps_done < max_reps);
  return st;
}

void cpu_convolve(const Filter& f, const ImageGeom& geom, const uint8_t* in, uint8_t* out, int reps, CpuBackend be,
                  int threads, Border border, int decimate) {
  HostFrames fr(f, geom, be, border);
  PCONV_CHECK(reps >= 0, "repetitions must be >= 0");
  check_decimate(decimate);
  fr.load(in);
  TeamScope team(be, threads);
  for (int t = 0; t < reps; ++t) fr.step();
  fr.copy_out_decimated(out, decimate);
}

// ---- unsharp mask --------------------------------------------------------------

int unsharp_k(double amount) {
  const double k = amount * 16.0;
  std::ostringstream got;
  got << amount;
  PCONV_CHECK(k >= 1.0 && k <= 255.0 && k == std::floor(k),
              "unsharp amount must be a multiple of 1/16 in [0.0625, 15.9375], got " + got.str());
  return static_cast<int>(k);
}

void check_unsharp(int k, int64_t threshold, int depth) {
  PCONV_CHECK(k >= 1 && k <= 255,
              "unsharp amount must be a multiple of 1/16 in [0.0625, 15.9375], got " + std::to_string(k) + "/16");
  const int64_t mx = depth == 16 ? 65535 : 255;
  PCONV_CHECK(threshold >= 0 && threshold <= mx, "unsharp threshold must be an integer in [0, " + std::to_string(mx) +
                                                     "], got " + std::to_string(threshold));
}

namespace {

template <typename T>
void unsharp_rows(const T* x, const T* b, T* out, int64_t n, int k, int t, bool omp) {
  constexpr int32_t mx = std::numeric_limits<T>::max();
#pragma omp parallel for schedule(static) if (omp)
  for (int64_t i = 0; i < n; ++i) {
    const int32_t xs = x[i], bs = b[i], d = xs - bs;
    // floor(num / 16), what the kernel's arithmetic >> 4 gives, written without
    // shifting a negative value
    const int32_t num = xs * (16 + k) - bs * k + 8;
    const int32_t q = num >= 0 ? num / 16 : -((-num + 15) / 16);
    out[i] = static_cast<T>((d < 0 ? -d : d) < t ? xs : std::min(std::max(q, int32_t(0)), mx));
  }
}

}  // namespace

void cpu_unsharp(const ImageGeom& geom, const uint8_t* orig, const uint8_t* blurred, uint8_t* out, int k,
                 int threshold, CpuBackend be, int threads) {
  geom.validate();
  check_unsharp(k, threshold, geom.depth);
  TeamScope team(be, threads);
  const bool omp = be == CpuBackend::OpenMP;
  const int64_t n = geom.bytes() / (geom.depth / 8);
  if (geom.depth == 16) {
    // the callers' buffers are uint16 arrays: 2-byte aligned
    PCONV_CHECK(reinterpret_cast<uintptr_t>(orig) % 2 == 0 && reinterpret_cast<uintptr_t>(blurred) % 2 == 0 &&
                    reinterpret_cast<uintptr_t>(out) % 2 == 0,
                "cpu_unsharp: depth 16 buffers must be 2-byte aligned");
    unsharp_rows(reinterpret_cast<const uint16_t*>(orig), reinterpret_cast<const uint16_t*>(blurred),
                 reinterpret_cast<uint16_t*>(out), n, k, threshold, omp);
  } else {
    unsharp_rows(orig, blurred, out, n, k, threshold, omp);
  }
}

void cpu_unsharp_convolve(const Filter& f, const ImageGeom& geom, const uint8_t* in, uint8_t* out, int reps, int k,
                          int threshold, CpuBackend be, int threads, Border border) {
  check_unsharp(k, threshold, geom.depth);
  if (out == in) {
    // in place: the blurred image needs a buffer of its own beside the original
    std::vector<uint8_t> blurred(static_cast<size_t>(geom.bytes()));
    cpu_convolve(f, geom, in, blurred.data(), reps, be, threads, border);
    cpu_unsharp(geom, in, blurred.data(), out, k, threshold, be, threads);
    return;
  }
  cpu_convolve(f, geom, in, out, reps, be, threads, border);
  cpu_unsharp(geom, in, out, out, k, threshold, be, threads);
}

uint64_t cpu_image_residual(const Filter& f, const ImageGeom& geom, const uint8_t* in, CpuBackend be, int threads,
                            Border border) {
  HostFrames fr(f, geom, be, border);
  fr.load(in);
  TeamScope team(be, threads);
  return fr.residual();
}

StableStats cpu_convolve_until_stable(const Filter& f, const ImageGeom& geom, const uint8_t* in, uint8_t* out,
                                      int max_reps, int check_every, CpuBackend be, int threads, Border border) {
  HostFrames fr(f, geom, be, border);
  fr.load(in);
  TeamScope team(be, threads);
  const StableStats st = fr.run_until_stable(max_reps, check_every);
  fr.copy_out(out);
  return st;
}

}  // namespace pconv
