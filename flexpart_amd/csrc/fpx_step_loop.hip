// fpx_step_loop.hip -- translation unit of k_pbl_loop and k_pbl_finish (fpx_r8p2.o, fpx_r4p2.o; fpx_tu.hpp).  Nothing but the kernels and the
// table that hands their host-stub addresses to the engine (fpx::step_kernel_*, fpx_engine.hip).
#define FPX_TU_PART 2
#include "fpx_tu.hpp"
#include "fpx_device.hpp"
#include "fpx_step_common.hpp"
#include "fpx_step_loop.hpp"

namespace fpx {
#if FPX_TU_REAL != 4
const void *step_kernel_loop_f64(bool lean, int turbswitch, int cblflag, int rng_mode, bool susp, bool *is_lean) { return loop_table<double>(lean, turbswitch, cblflag, rng_mode, susp, is_lean); }
const void *step_kernel_finish_f64(bool drydep, bool polar, bool nest) { return finish_table<double>(drydep, polar, nest); }
#endif
#if FPX_TU_REAL != 8
const void *step_kernel_loop_f32(bool lean, int turbswitch, int cblflag, int rng_mode, bool susp, bool *is_lean) { return loop_table<float>(lean, turbswitch, cblflag, rng_mode, susp, is_lean); }
const void *step_kernel_finish_f32(bool drydep, bool polar, bool nest) { return finish_table<float>(drydep, polar, nest); }
#endif
}  // namespace fpx
