// CPU stencil: the serial oracle and the OpenMP backend.
//
// Reference: Convolution() loops a rectangular region of the padded local block
// (mpi/mpi_convolution.c:288-299) and calls ConvolutionforGrey/RGB per pixel
// (:301-322), a float MAC over a `float**` filter.  The OpenMP build adds
// `#pragma omp parallel for ... collapse(3)` on a 2-deep nest
// (open-mp/omp_convolution.c:292,297), which does not compile.
//
// Here the CPU path works on the same FrameLayout as the GPU (zero pad ring),
// computes any row range of a frame, and has two arithmetic modes:
//   * integer  (Σ tap·p) >> shift   when filter.int_exact   (bit-exact, §0.1)
//   * float32  mul-then-add in reference tap order, truncating store.
// The OpenMP variant parallelises the row loop (correct `collapse`-free form).
#pragma once

#include <cstdint>
#include <functional>
#include <vector>

#include "pconv/filter.hpp"
#include "pconv/image.hpp"

namespace pconv {

enum class CpuBackend { Serial, OpenMP };

// Frame pointers here are the frame BASE (row -halo, column -kPadLeft).
// One step: for owned rows [r0, r1) of the frame, dst = conv(src).  Pixels whose
// global row lies outside [0, image_height) are treated as zero by the caller's
// frame (ghost rows hold zeros at the global image edges).
// With Border::Replicate the taps clamp to the global image instead (g_row0 =
// global row of frame row 0, height = global image height, < 0: the frame's
// owned rows end the image): [r0, r1) must lie inside the image, ghost rows
// and pad columns beyond it are never read and the source frame is not
// modified.
void cpu_step(const Filter& f, Channels ch, const FrameLayout& lay, const uint8_t* src_frame,
              uint8_t* dst_frame, int64_t r0, int64_t r1, CpuBackend be, Border border = Border::Zero,
              int64_t g_row0 = 0, int64_t height = -1, int depth = 8);
// depth 16 (cpu_step, cpu_fused_launch, HostFrames through its geometry): the
// frame's rows hold unsigned 16-bit samples in host byte order (row_bytes =
// width x channels x 2), out = (sum w p) >> 4 in 32-bit integers; the gaussian
// only, any other filter is refused by name.

// Reference semantics of one fused launch (what the temporal GPU kernel
// computes): `steps` repetitions starting from src rows [lo-steps, hi+steps),
// rows outside the global image [0, height) held at zero after every step
// (Border::Zero) or never read (Border::Replicate, whatever the frame holds
// there); writes rows [lo, hi) of dst only.  g_row0 = global row of frame row 0.
void cpu_fused_launch(const Filter& f, Channels ch, const FrameLayout& lay, const uint8_t* src_frame,
                      uint8_t* dst_frame, int64_t lo, int64_t hi, int steps, int64_t g_row0, int64_t height,
                      CpuBackend be, Border border = Border::Zero, int depth = 8);

// A whole image on the host: its two zero-padded ping-pong frames
// (FrameLayout::make(row_bytes, height, 1); the reference's calloc'd buffers,
// mpi/mpi_convolution.c:104-124) and the loops over them.  Every whole-image
// CPU path is built on it; the OpenMP team is the caller's.
class HostFrames {
 public:
  HostFrames(const Filter& f, const ImageGeom& geom, CpuBackend be, Border border = Border::Zero);
  // Allocate both frames zeroed and fill the newest one: from contiguous rows
  // (pitch == row_bytes), or by fill(row 0 column 0, pitch).
  void load(const uint8_t* in);
  void load(const std::function<void(uint8_t* row0, int64_t pitch)>& fill);
  void release();  // free both frames (load() brings them back)
  void step();     // one repetition; its result is the newest frame
  // cpu_residual of the newest frame.
  uint64_t residual() const;
  // The newest frame as contiguous rows.
  void copy_out(uint8_t* out) const;
  // Every factor-th pixel of every factor-th row of the newest frame (phase 0)
  // as contiguous rows: ceil(height / factor) rows of ceil(width / factor)
  // whole pixels.  Factor 1 is copy_out.
  void copy_out_decimated(uint8_t* out, int factor) const;
  // Chunks of `check_every` repetitions (the last one shorter), residual()
  // after each, at most max_reps repetitions; the final check is made even at
  // max_reps (repetitions 0: the input itself is checked).
  StableStats run_until_stable(int max_reps, int check_every);

 private:
  Filter f_;
  ImageGeom geom_;
  CpuBackend be_;
  Border border_;
  FrameLayout lay_;
  std::vector<uint8_t> cur_, nxt_;
};

// reps steps on a contiguous image (pitch == row_bytes), zero-padded semantics
// unless `border` says otherwise.
// Ping-pongs internally; result written to `out` (may alias `in`).
// decimate = s > 1: `out` receives out[Y][X] = result[Y * s][X * s] instead,
// decimated_geom(geom, s).bytes() bytes (image.hpp).
void cpu_convolve(const Filter& f, const ImageGeom& geom, const uint8_t* in, uint8_t* out,
                  int reps, CpuBackend be, int threads = 0, Border border = Border::Zero, int decimate = 1);

// Unsharp mask (the CPU twin of launch_unsharp, kernels.hpp): per sample of
// three tight images of `geom` (pitch == row_bytes, depth 16: host byte order),
// with x from `orig`, b from `blurred`, d = x - b and max = 255 | 65535,
//   out = x                                           if |d| < threshold
//   out = clamp((x (16 + k) - b k + 8) >> 4, 0, max)  otherwise
// in 32-bit integers (arithmetic shift).  `out` may be `blurred` or `orig`
// (a sample is read before it is written).
void cpu_unsharp(const ImageGeom& geom, const uint8_t* orig, const uint8_t* blurred, uint8_t* out, int k,
                 int threshold, CpuBackend be, int threads = 0);
// cpu_convolve followed by cpu_unsharp against the input: x + (k / 16)(x -
// blur(x)).  `out` may alias `in`.
void cpu_unsharp_convolve(const Filter& f, const ImageGeom& geom, const uint8_t* in, uint8_t* out, int reps, int k,
                          int threshold, CpuBackend be, int threads = 0, Border border = Border::Zero);
// The argument checks every backend shares.  unsharp_k: amount x 16 as an exact
// integer in [1, 255], else "unsharp amount must be a multiple of 1/16 in
// [0.0625, 15.9375], got ...".  check_unsharp: k in [1, 255] and threshold in
// [0, max of the depth], else an error of the same shape.
int unsharp_k(double amount);
void check_unsharp(int k, int64_t threshold, int depth);

// Residual of the iterated map (the CPU twin of launch_residual): the number
// of bytes in rows [r0, r1) of the frame that one more repetition would
// change.  cpu_step's row kernels into a scratch row, compared and counted —
// no second frame.  Rows outside the global image [0, height) read as zeros
// (Border::Zero, whatever the frame holds there) or clamp (Border::Replicate);
// [r0, r1) is clipped to the image.  height < 0: the owned rows end the image.
uint64_t cpu_residual(const Filter& f, Channels ch, const FrameLayout& lay, const uint8_t* src_frame, int64_t r0,
                      int64_t r1, CpuBackend be, Border border = Border::Zero, int64_t g_row0 = 0,
                      int64_t height = -1);
// The same for a contiguous image (pitch == row_bytes).
uint64_t cpu_image_residual(const Filter& f, const ImageGeom& geom, const uint8_t* in, CpuBackend be, int threads = 0,
                            Border border = Border::Zero);

// cpu_convolve that stops at the fixed point: chunks of `check_every`
// repetitions (the last one shorter), a residual check after each chunk, at
// most max_reps repetitions; the final check is made even at max_reps.
StableStats cpu_convolve_until_stable(const Filter& f, const ImageGeom& geom, const uint8_t* in, uint8_t* out,
                                      int max_reps, int check_every, CpuBackend be, int threads = 0,
                                      Border border = Border::Zero);

// OpenMP team size when the user set none (OMP_NUM_THREADS unset, no
// --threads): the CPUs this process may run on (affinity mask), capped by the
// cgroup CPU quota (a container or GPU-box slice sees every CPU of the
// machine but may use only its quota), minus one when more than two remain —
// a fork/join team that claims EVERY available CPU while anything else runs
// spins into the scheduler (measured 10 ms per parallel region with 8
// threads on 8 busy vCPUs vs 5 us with 7).
int default_cpu_threads();
// Apply default_cpu_threads() unless OMP_NUM_THREADS is set; `share` divides
// the CPUs between that many processes (ranks on one node).  Returns the team size.
int configure_cpu_threads(int share = 1);

}  // namespace pconv
