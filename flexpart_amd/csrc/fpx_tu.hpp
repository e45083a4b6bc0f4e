// fpx_tu.hpp -- how the library is split into translation units.
//
// Three sources, each compiled once per arithmetic type, in parallel (__graft_entry__.build_library): six objects.
//   part 0  fpx_engine.hip     the host side (Engine<R>, the C ABI) and every kernel except the three of the step;
//   part 1  fpx_step_prep.hip  k_prep (16 instances per type);
//   part 2  fpx_step_loop.hip  k_pbl_loop + k_pbl_finish.
// A source names its part itself (#define FPX_TU_PART before the first include).  Parts 1 and 2 export their kernels as
// tables of host-stub addresses (fpx::step_kernel_*), which is how the engine launches them anyway.
//   -DFPX_TU_REAL=8|4   the arithmetic type of the unit: 8 = fp64 (and, in part 0, the C ABI), 4 = the reference-typed
//                        fp32 engine (reached through fpx::make_engine_f32); without the flag (0) a source holds both
//                        types (tools/kernel_resources.sh).
// Everything inside namespace fpx lives in an inline namespace named after the unit (tu_r8_p0 .. tu_r4_p2), so the objects
// share no symbol except the ones declared outside FPX_TU_OPEN .. FPX_TU_CLOSE (the error string, EngineBase, the
// factory and the kernel tables).  A feature header included by anything else (the tests that compile a device body as
// host code) sees no part and gets the namespace tu_r0_pall.
#pragma once
#ifndef FPX_TU_REAL
#define FPX_TU_REAL 0
#endif
#define FPX_TU_CAT2(a, b, c) a##b##_p##c
#define FPX_TU_CAT(a, b, c) FPX_TU_CAT2(a, b, c)
#if FPX_TU_REAL != 0 && FPX_TU_REAL != 4 && FPX_TU_REAL != 8
#error "FPX_TU_REAL must be 0, 4 or 8"
#endif
#ifndef FPX_TU_PART
#define FPX_TU_OPEN inline namespace FPX_TU_CAT(tu_r, FPX_TU_REAL, all) {
#else
#define FPX_TU_OPEN inline namespace FPX_TU_CAT(tu_r, FPX_TU_REAL, FPX_TU_PART) {
#endif
#define FPX_TU_CLOSE }
