// fpx_step_prep.hip -- translation unit of k_prep (fpx_r8p1.o, fpx_r4p1.o; fpx_tu.hpp).  Nothing but the kernels and the
// table that hands their host-stub addresses to the engine (fpx::step_kernel_*, fpx_engine.hip).
#define FPX_TU_PART 1
#include "fpx_tu.hpp"
#include "fpx_device.hpp"
#include "fpx_step_common.hpp"
#include "fpx_step_prep.hpp"

namespace fpx {
#if FPX_TU_REAL != 4
const void *step_kernel_prep_f64(bool drydep, bool init, bool polar, bool nest) { return prep_table<double>(drydep, init, polar, nest); }
#endif
#if FPX_TU_REAL != 8
const void *step_kernel_prep_f32(bool drydep, bool init, bool polar, bool nest) { return prep_table<float>(drydep, init, polar, nest); }
#endif
}  // namespace fpx
