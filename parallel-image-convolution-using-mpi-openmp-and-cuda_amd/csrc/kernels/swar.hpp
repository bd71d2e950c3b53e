// Internal interface of the SWAR-32 temporal kernel (kernels/stencil_swar.hip).
#pragma once

#include <hip/hip_runtime_api.h>

#include "pconv/kernels.hpp"

namespace pconv {

// Latency model of one launch (cycles) and the shape it picks; the grid is
// `batch` images of rows x row_bytes (ImageSet::images()).
double swar_launch_cycles(SwarShape s, int steps, int ch, int64_t rows, int64_t row_bytes, int batch = 1);
SwarShape pick_swar_shape(int steps, int ch, int64_t rows, int64_t row_bytes, int batch = 1);

// Enqueue the fused gaussian for `a.steps` repetitions.  Shape: forced
// (set_swar_shape), else tuned on first use (the model's best candidates
// timed on this launch; set_shape_tuning(false): model only), else the model's
// pick while a graph is being captured.  Shapes, forcing and the tuned table:
// pconv/kernels.hpp.
void launch_swar(const StencilLaunch& a, Channels ch, hipStream_t stream);
// Tune (if needed) without enqueueing the launch — before a graph capture.
void prepare_swar(const StencilLaunch& a, Channels ch, hipStream_t stream);

// VGPRs per lane and LDS bytes of one instantiation as the runtime reports
// them (measured = false: no device, model estimate).
struct SwarResources {
  int vgpr = 0;
  int lds = 0;
  bool measured = false;
};
SwarResources swar_resources(SwarShape s, int ch);
// XCD-aware tile order of the SWAR kernels (default on).
void set_xcd_swizzle(bool on);
// Step form: -1 tuned per launch geometry (default), 0 truncate every step,
// 1 steps in pairs with a scale-16 intermediate (larger modes clamp to 1).
void set_swar_alt(int mode);
// Buffer-op tile kernel (k_swar_pf): -1 among the tuned candidates
// (default), 0 never, 1 forced; with the mode forced, a shape set by
// set_swar_shape that it instantiates is used as is (tests).
void set_prefetch_mode(int mode);
// The two settings as the 16-bit kernel's launches read them (stencil_swar16.hip).
bool swar_xcd_swizzle();
int swar_alt_mode();

// The 16-bit gaussian (kernels/stencil_swar16.hip): a.depth == 16, every step
// count up to kMaxFusedSteps.  Shape: forced (set_swar16_shape), else tuned on
// first use over the shapes that run the launch x both step forms, else the
// first shape whose grid fills the chip.
void launch_swar16(const StencilLaunch& a, Channels ch, hipStream_t stream);
void prepare_swar16(const StencilLaunch& a, Channels ch, hipStream_t stream);
void clear_swar16_tuning();

}  // namespace pconv
